"""The packed MXFP4 decode layout's additions to the C ABI (include/srgpt.h: srgpt_mxfp4_packed_bytes, srgpt_pack_mxfp4,
srgpt_unpack_mxfp4, srgpt_gemv_w4p, srgpt_mxfp4_bind / _unbind / _bound), without a GPU: declared, exported and listed; argument
errors found on the host before any launch; the size formula of the header; srgpt_llm_weights did not grow."""
import ctypes
import os
import re
import subprocess

from tests.util import ROOT

NEW = ("srgpt_mxfp4_packed_bytes", "srgpt_pack_mxfp4", "srgpt_unpack_mxfp4", "srgpt_gemv_w4p", "srgpt_mxfp4_bind", "srgpt_mxfp4_unbind",
       "srgpt_mxfp4_bound")


def test_new_names_are_declared_exported_and_listed_under_abi_9():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    assert lib.srgpt_abi_version() == _lib.ABI_VERSION == 9
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srgpt.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and name in exported, name
        params = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^)]*)\)" % name, hdr)
        assert params, name + " is not declared in include/srgpt.h"
        assert len(params.group(1).split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert re.search(r"#define\s+SRGPT_MXFP4_GRANULE\s+16\b", hdr)


def test_weight_struct_did_not_grow():
    from spatialrgpt_amd import _lib

    names = [f[0] for f in _lib.LlmWeights._fields_]
    assert names[-1] == "wdown4_scale"  # the packed copies reach the step through the binding table, not through the struct
    assert ctypes.sizeof(_lib.LlmWeights) == _lib.LlmWeights.pk_rows_qkv.offset + 16 + 8 * ctypes.sizeof(ctypes.c_void_p)


def test_packed_bytes_is_the_headers_formula():
    """ceil(rows / G) * (K / 128) * 68 G bytes, rows = 2 N with swiglu; 0 outside the domain"""
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    G = 16

    def want(N, K, sw):
        rows = 2 * N if sw else N
        return (rows + G - 1) // G * (K // 128) * 68 * G

    for N, K, sw in ((1, 128, 0), (16, 128, 0), (17, 384, 0), (64, 1408, 0), (16, 128, 1), (48, 384, 1), (6144, 4096, 0),
                     (4096, 4096, 0), (14336, 4096, 1), (4096, 14336, 0)):
        assert lib.srgpt_mxfp4_packed_bytes(N, K, sw) == want(N, K, sw), (N, K, sw)
    # the 8B model's copies: 0.53125 bytes per weight (codes + scales, no padding at these shapes)
    assert lib.srgpt_mxfp4_packed_bytes(14336, 4096, 1) == 2 * 14336 * 4096 * 17 // 32
    for N, K, sw in ((0, 128, 0), (16, 0, 0), (16, 96, 0), (16, 64, 0), (16, 4096 + 32, 0), (24, 128, 1), (1, 128, 1), (-1, 128, 0)):
        assert lib.srgpt_mxfp4_packed_bytes(N, K, sw) == 0, (N, K, sw)


def test_entry_points_validate_on_the_host():
    """argument errors are detected before any launch (and before the device is asked anything): safe without a GPU"""
    from spatialrgpt_amd import _lib

    lib = _lib.load()

    def w4p(x=16, packed=16, norm=None, res=None, out=16, batch=2, N=16, K=128, swiglu=0, f32=0, ss_in=None, ss_out=None):
        return lib.srgpt_gemv_w4p(x, packed, norm, 0.0, res, out, batch, N, K, swiglu, f32, ss_in, ss_out, None)

    for missing in ("x", "packed", "out"):
        assert w4p(**{missing: None}) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error(), missing
    assert w4p(K=96) == _lib.ERR_ARG and b"multiple of 128" in lib.srgpt_last_error()
    assert w4p(N=24, swiglu=1) == _lib.ERR_ARG and b"granule" in lib.srgpt_last_error()  # a SwiGLU half off the granule
    assert w4p(swiglu=1, res=16) == _lib.ERR_ARG and b"swiglu" in lib.srgpt_last_error()
    assert w4p(swiglu=1, f32=1) == _lib.ERR_ARG and b"swiglu" in lib.srgpt_last_error()
    assert w4p(ss_in=16) == _lib.ERR_ARG and b"norm_w" in lib.srgpt_last_error()  # published statistics without the RMSNorm
    assert w4p(ss_out=16, f32=1) == _lib.ERR_ARG and b"statistics" in lib.srgpt_last_error()
    assert w4p(batch=0) == _lib.ERR_ARG and b"shape" in lib.srgpt_last_error()
    assert w4p(N=0) == _lib.ERR_ARG and b"shape" in lib.srgpt_last_error()
    for args in ((None, 16, 16), (16, None, 16), (16, 16, None)):
        assert lib.srgpt_pack_mxfp4(*args, 16, 128, 0, None) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error()
        assert lib.srgpt_unpack_mxfp4(*args, 16, 128, 0, None) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error()
    for fn in (lib.srgpt_pack_mxfp4, lib.srgpt_unpack_mxfp4):
        assert fn(16, 16, 16, 16, 96, 0, None) == _lib.ERR_ARG and b"multiple of 128" in lib.srgpt_last_error()
        assert fn(16, 16, 16, 24, 128, 1, None) == _lib.ERR_ARG and b"granule" in lib.srgpt_last_error()
        assert fn(16, 16, 16, 0, 128, 0, None) == _lib.ERR_ARG and b"shape" in lib.srgpt_last_error()
