"""The W4A16 prefill products of the C ABI (include/srgpt.h: srgpt_gemm_w4, srgpt_gemm_w4_norm, srgpt_gemm_w4_swiglu,
srgpt_gemm_w4_rope_kv_append, srgpt_gemm_w4_in_kernel) without a GPU: the names are declared, exported and prototyped, and every
argument error is found on the host before any launch."""
import os
import re
import subprocess

from tests.util import ROOT

NAMES = ("srgpt_gemm_w4", "srgpt_gemm_w4_norm", "srgpt_gemm_w4_swiglu", "srgpt_gemm_w4_rope_kv_append", "srgpt_gemm_w4_in_kernel")
P = 256  # a non-null, 16-byte aligned "pointer": nothing is dereferenced before the checks


def test_new_symbols_are_exported_under_abi_9():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    assert lib.srgpt_abi_version() == _lib.ABI_VERSION == 9
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srgpt.h")).read(), flags=re.S)
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in include/srgpt.h"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= {ln.split()[-1] for ln in out.splitlines() if ln.split()}


def test_wrappers_exist():
    from spatialrgpt_amd import ops

    for name in ("gemm_w4", "gemm_w4_norm", "gemm_w4_swiglu", "gemm_w4_rope_kv_append", "gemm_w4_in_kernel"):
        assert callable(getattr(ops, name))


def _gemm_w4(lib, A=P, W4=P, sc=P, C=P, M=33, N=72, K=64, lda=None, expand=None, ws=None, ws_bytes=0):
    return lib.srgpt_gemm_w4(A, W4, sc, None, C, M, N, K, K if lda is None else lda, N, 0, expand, ws, ws_bytes, None)


def test_gemm_w4_validates_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    for missing in ("A", "W4", "sc", "C"):  # NULL scales must not pass as "a bf16 matrix"
        assert _gemm_w4(lib, **{missing: None}) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error(), missing
    assert _gemm_w4(lib, K=48) == _lib.ERR_ARG and b"multiple" in lib.srgpt_last_error()  # half a block (and no 16-byte rows)
    assert _gemm_w4(lib, K=96 + 16) == _lib.ERR_ARG and b"multiple of 32" in lib.srgpt_last_error()  # 16-byte rows, half a block
    assert _gemm_w4(lib, M=0) == _lib.ERR_ARG and b"shape" in lib.srgpt_last_error()
    assert _gemm_w4(lib, A=P + 8) == _lib.ERR_ARG and b"16-byte" in lib.srgpt_last_error()
    assert _gemm_w4(lib, W4=P + 2) == _lib.ERR_ARG and b"4-byte" in lib.srgpt_last_error()
    assert _gemm_w4(lib, lda=60) == _lib.ERR_ARG
    # expansion shapes without the scratch: K % 64 == 32, the 256 x 256 tiles, the whole-M kernel (no device: 256 CUs are assumed)
    assert lib.srgpt_gemm_w4_in_kernel(33, 72, 64, 0, 0, 0) == 1
    for M, N, K in ((33, 72, 96), (576, 600, 2048), (259, 6144, 4096)):
        ws = dict(ws=P, ws_bytes=32 * M * N)
        assert lib.srgpt_gemm_w4_in_kernel(M, N, K, 0, 1, ws["ws_bytes"]) == 0
        assert _gemm_w4(lib, M=M, N=N, K=K, **ws) == _lib.ERR_ARG and b"scratch" in lib.srgpt_last_error(), (M, N, K)
        assert _gemm_w4(lib, M=M, N=N, K=K, expand=P + 8, **ws) == _lib.ERR_ARG and b"scratch" in lib.srgpt_last_error(), (M, N, K)
    # without a workspace the 259-row q/k/v product is not split, leaves the whole-M kernel, and multiplies its codes
    assert lib.srgpt_gemm_w4_in_kernel(259, 6144, 4096, 0, 0, 0) == 1


def test_the_composites_validate_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    # srgpt_gemm_w4_norm(A, W4, wscale8, residual, C, M, N, K, expand, ws, ws_bytes, norm_w, Y, eps, stream)
    norm = lambda **k: lib.srgpt_gemm_w4_norm(k.get("A", P), k.get("W4", P), k.get("sc", P), None, k.get("C", P), 33, 72, k.get("K", 64),  # noqa: E731
                                              k.get("expand"), None, 0, k.get("norm_w", P), k.get("Y", 2 * P), 1e-5, None)
    for missing in ("A", "W4", "sc", "C", "norm_w", "Y"):
        assert norm(**{missing: None}) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error(), missing
    assert norm(Y=P) == _lib.ERR_ARG and b"alias" in lib.srgpt_last_error()
    assert norm(K=96) == _lib.ERR_ARG and b"scratch" in lib.srgpt_last_error()
    assert norm(K=80) == _lib.ERR_ARG and b"multiple of 32" in lib.srgpt_last_error()
    # srgpt_gemm_w4_swiglu(A, Wgu4, wscale8, out, M, I, K, gu_scratch, expand, ws, ws_bytes, stream)
    swi = lambda **k: lib.srgpt_gemm_w4_swiglu(k.get("A", P), k.get("W4", P), k.get("sc", P), k.get("out", P), k.get("M", 37), k.get("I", 1408),  # noqa: E731
                                               k.get("K", 512), k.get("gu", P), k.get("expand"), None, 0, None)
    for missing in ("A", "W4", "sc", "out"):
        assert swi(**{missing: None}) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error(), missing
    assert swi(gu=None) == _lib.ERR_ARG and b"scratch" in lib.srgpt_last_error()
    assert swi(K=80) == _lib.ERR_ARG and b"multiple of 32" in lib.srgpt_last_error()
    assert lib.srgpt_gemm_w4_in_kernel(259, 8192, 256, 1, 0, 0) == 0  # the fused form runs on the whole-M kernel: it expands
    assert swi(M=259, I=8192, K=256, gu=None) == _lib.ERR_ARG and b"scratch" in lib.srgpt_last_error()
    assert lib.srgpt_gemm_w4_in_kernel(37, 1408, 512, 1, 0, 0) == 1
    # srgpt_gemm_w4_rope_kv_append(A, W4, wscale8, qkv, K, expand, ws, ws_bytes, kcache, vcache, pos0, cos, sin, B, T, Hq, Hkv, D, max_pos, stream)
    rope = lambda **k: lib.srgpt_gemm_w4_rope_kv_append(k.get("A", P), k.get("W4", P), k.get("sc", P), k.get("qkv", P), k.get("K", 512), None, None, 0,  # noqa: E731
                                                        k.get("kc", P), k.get("vc", P), None, k.get("cos", P), k.get("sin", P), 1,
                                                        k.get("T", 37), 8, 2, k.get("D", 64), 64, None)
    for missing in ("A", "W4", "sc", "qkv", "kc", "vc", "cos", "sin"):
        assert rope(**{missing: None}) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error(), missing
    assert rope(T=65) == _lib.ERR_ARG and b"shape" in lib.srgpt_last_error()  # past max_pos
    assert rope(D=63) == _lib.ERR_ARG and b"shape" in lib.srgpt_last_error()
    assert rope(K=544) == _lib.ERR_ARG and b"scratch" in lib.srgpt_last_error()  # K % 64 == 32
    # srgpt_gemm_w4_in_kernel answers 0 for shapes no entry point takes
    assert lib.srgpt_gemm_w4_in_kernel(0, 72, 64, 0, 0, 0) == 0 and lib.srgpt_gemm_w4_in_kernel(33, 72, 48, 0, 0, 0) == 0
