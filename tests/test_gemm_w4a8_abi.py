"""W4A8 (e4m3 activations x MXFP4 weights on the block-scaled MFMA) at the C ABI and the Python surface, without a GPU:
srgpt_gemm_w4a8 is declared, exported and listed with srgpt_gemm_w8a8's arguments; its argument errors and the prefill's width check
come back from the host before any launch; llm_weight_format="mxfp4_w4a8" is "mxfp4" + fp8_act on PreparedWeights and goes down from
the loader; the LLM workspace is the "mxfp4" one without the bf16 expansion scratch and with the activation bytes and scales."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests.util import ROOT


def test_symbol_is_declared_exported_and_listed_with_the_w8a8_arguments():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    assert lib.srgpt_abi_version() == _lib.ABI_VERSION == 9
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srgpt.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}

    def params(name):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name + " is not declared in include/srgpt.h"
        return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]

    name = "srgpt_gemm_w4a8"
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and name in exported
    # srgpt_gemm_w8a8's list with the weight operand (codes, E8M0 bytes) in place of (fp8 bytes, fp32 row scales)
    want = [p.replace("const void* W8", "const void* W4").replace("const float* wscale", "const void* wscale8") for p in params("srgpt_gemm_w8a8")]
    assert params(name) == want
    assert _lib._SIGNATURES[name] == _lib._SIGNATURES["srgpt_gemm_w8a8"] and len(want) == len(_lib._SIGNATURES[name][1])


def test_argument_errors_come_back_before_any_launch():
    """the pattern of tests/test_gemm_w4_direct_abi.py::test_direct_entries_validate_like_the_plain_ones: pointers are never followed"""
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    fn = lib.srgpt_gemm_w4a8
    P = 4096  # an address with every alignment the entry asks for

    def call(A8=P, ascale=P, W4=P, wscale8=P, C=P, M=4, N=4, K=256, lda=None, ldc=None):
        return fn(A8, ascale, W4, wscale8, None, None, C, M, N, K, K if lda is None else lda, N if ldc is None else ldc, 0, None, 0, None)

    for null in ("A8", "ascale", "W4", "wscale8", "C"):
        assert call(**{null: None}) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error(), null
    assert call(K=192) == _lib.ERR_UNSUPPORTED and b"multiple of 128" in lib.srgpt_last_error()
    assert call(K=128) == _lib.ERR_UNSUPPORTED and b">= 256" in lib.srgpt_last_error()
    assert call(K=256, lda=128) == _lib.ERR_ARG and b"lda < K" in lib.srgpt_last_error()
    assert call(N=8, ldc=4) == _lib.ERR_ARG and b"ldc < N" in lib.srgpt_last_error()
    assert call(K=256, lda=264) == _lib.ERR_UNSUPPORTED  # lda % 16
    for off in (1, 2, 4, 8):  # misaligned codes: the kernel stages them in 16-byte pieces
        assert call(W4=P + off) == _lib.ERR_UNSUPPORTED and b"aligned" in lib.srgpt_last_error(), off
    assert call(A8=P + 8) == _lib.ERR_UNSUPPORTED and call(wscale8=P + 2) == _lib.ERR_UNSUPPORTED
    # the same codes srgpt_gemm_w8a8 returns for the same mistakes
    g8 = lib.srgpt_gemm_w8a8
    assert g8(P, P, None, P, None, None, P, 4, 4, 256, 256, 4, 0, None, 0, None) == _lib.ERR_ARG
    assert g8(P, P, P, P, None, None, P, 4, 4, 192, 192, 4, 0, None, 0, None) == _lib.ERR_UNSUPPORTED
    assert g8(P, P, P, P, None, None, P, 4, 4, 256, 128, 4, 0, None, 0, None) == _lib.ERR_ARG


def _mxfp4_struct(_lib, hidden, inter, heads, head_dim):
    w = _lib.LlmWeights()
    w.dtype, w.hidden, w.inter, w.layers, w.heads, w.kv_heads, w.head_dim, w.vocab = _lib.BF16, hidden, inter, 1, heads, heads, head_dim, 100
    some = (_lib.vp * 1)(4096)
    for f in ("wqkv4", "wqkv4_scale", "wo4", "wo4_scale", "wgu4", "wgu4_scale", "wdown4", "wdown4_scale"):
        setattr(w, f, some)
    w.lm_head8 = w.lm_head_scale = 4096
    return w, some


def test_prefill_refuses_widths_the_w4a8_product_does_not_take():
    """wqkv4 + fp8_act = 1 with hidden 64: SRGPT_ERR_UNSUPPORTED before any launch, the message names the multiple of 128; the same
    struct with fp8_act = 0 is past that check (it is "mxfp4")"""
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    w, keep = _mxfp4_struct(_lib, 64, 128, 2, 32)
    st = _lib.LlmState()
    for f in ("kcache", "vcache", "pos", "tok", "out_ids", "step", "ws", "logits"):
        setattr(st, f, 4096)
    st.batch, st.max_pos, st.max_new, st.ws_tokens = 1, 64, 4, 32
    w.fp8_act = 1
    rc = lib.srgpt_llm_prefill(ctypes.byref(w), ctypes.byref(st), 4096, 8, None, None, None)
    assert rc == _lib.ERR_UNSUPPORTED and b"multiples of 128" in lib.srgpt_last_error()
    rc = lib.srgpt_llm_prefill_append(ctypes.byref(w), ctypes.byref(st), 4096, 8, None, 4, None, None, None)
    assert rc == _lib.ERR_UNSUPPORTED and b"multiples of 128" in lib.srgpt_last_error()
    # mxfp4_direct is still validated, and not consulted otherwise: 1 with these weights is no error of its own
    w.mxfp4_direct = 2
    assert lib.srgpt_llm_prefill(ctypes.byref(w), ctypes.byref(st), 4096, 8, None, None, None) == _lib.ERR_ARG
    w.mxfp4_direct = 1
    assert lib.srgpt_llm_prefill(ctypes.byref(w), ctypes.byref(st), 4096, 8, None, None, None) == _lib.ERR_UNSUPPORTED


def test_prepared_weights_report_mxfp4_with_fp8_act():
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.weights import PreparedWeights

    cfg = SrgptConfig(hidden=256, inter=384, heads=4, kv_heads=2)
    assert (cfg.heads * cfg.head_dim) % 128 == 0
    w = PreparedWeights(cfg, {}, "cpu", torch.bfloat16, parts=(), llm_weight_format="mxfp4_w4a8")
    assert w.llm_weight_format == "mxfp4" and w.fp8_act is True and w.mxfp4_prefill_direct is False
    w = PreparedWeights(cfg, {}, "cpu", torch.bfloat16, parts=(), llm_weight_format="mxfp4_w4a8", mxfp4_packed=True, decode_pass_rows=32)
    assert w.llm_weight_format == "mxfp4" and w.fp8_act is True
    # the neighbours did not move
    w = PreparedWeights(cfg, {}, "cpu", torch.bfloat16, parts=(), llm_weight_format="mxfp4")
    assert w.llm_weight_format == "mxfp4" and w.fp8_act is False
    w = PreparedWeights(cfg, {}, "cpu", torch.bfloat16, parts=(), llm_weight_format="fp8_w8a8")
    assert w.llm_weight_format == "fp8" and w.fp8_act is True


def test_value_errors_of_the_format():
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.weights import PreparedWeights

    ok = SrgptConfig(hidden=256, inter=384, heads=4, kv_heads=2)
    with pytest.raises(ValueError, match="bf16"):
        PreparedWeights(ok, {}, "cpu", torch.float32, parts=(), llm_weight_format="mxfp4_w4a8")
    for bad in (dict(hidden=320, inter=384, heads=5, kv_heads=5), dict(hidden=256, inter=416, heads=4, kv_heads=2)):
        with pytest.raises(ValueError, match="multiples of 128"):
            PreparedWeights(SrgptConfig(**bad), {}, "cpu", torch.bfloat16, parts=(), llm_weight_format="mxfp4_w4a8")
    with pytest.raises(ValueError, match="mxfp4_prefill_direct"):  # the option would do nothing: no product of this format expands
        PreparedWeights(ok, {}, "cpu", torch.bfloat16, parts=(), llm_weight_format="mxfp4_w4a8", mxfp4_prefill_direct=True)
    with pytest.raises(ValueError, match="unknown llm_weight_format"):
        PreparedWeights(ok, {}, "cpu", torch.bfloat16, parts=(), llm_weight_format="mxfp4_w8a8")


def test_loader_passes_the_format_through(monkeypatch):
    import spatialrgpt_amd.builder as builder
    import spatialrgpt_amd.model as model
    from spatialrgpt_amd.config import SrgptConfig

    seen = []

    class Stub:
        def __init__(self, *a, **kw):
            seen.append(kw)

    monkeypatch.setattr(builder, "read_checkpoint", lambda *a, **kw: (SrgptConfig(), {}))
    monkeypatch.setattr(builder, "load_tokenizer", lambda *a, **kw: None)
    monkeypatch.setattr(builder, "load_image_processor", lambda *a, **kw: None)
    monkeypatch.setattr(builder, "_read_json", lambda p: {})
    monkeypatch.setattr(model, "LlavaLlamaModel", Stub)
    builder.load_pretrained_model("nowhere", "tiny", llm_weight_format="mxfp4_w4a8", mxfp4_packed=True, decode_pass_rows=32)
    assert [(kw["llm_weight_format"], kw["mxfp4_packed"], kw["decode_pass_rows"], kw["mxfp4_prefill_direct"]) for kw in seen] == \
        [("mxfp4_w4a8", True, 32, False)]


def test_workspace_drops_the_expansion_scratch_and_holds_the_activation_bytes():
    """From the layout include/srgpt.h and DESIGN.md section 4 document, not from the code: every region of the workspace is rounded up
    to 256 bytes; "mxfp4" ends with the bf16 expansion scratch of the largest layer matrix; fp8_act adds [rows, max K] e4m3 bytes and
    [rows] fp32 scales, rows = batch * max_tokens, max K over hidden, inter and heads * head_dim."""
    from spatialrgpt_amd import _lib
    from spatialrgpt_amd.config import SrgptConfig

    lib = _lib.load()

    def up(n):
        return (n + 255) // 256 * 256

    small = SrgptConfig(hidden=512, inter=1408, heads=8, kv_heads=2)
    for cfg, B, T in ((small, 1, 37), (small, 3, 37), (SrgptConfig.vila15_8b(), 1, 259), (SrgptConfig.vila15_8b(), 8, 259)):
        w, keep = _mxfp4_struct(_lib, cfg.hidden, cfg.inter, cfg.heads, cfg.head_dim)
        w.kv_heads, w.layers, w.vocab = cfg.kv_heads, cfg.layers, cfg.vocab
        plain = lib.srgpt_llm_ws_bytes(ctypes.byref(w), B, T)
        w.fp8_act = 1
        got = lib.srgpt_llm_ws_bytes(ctypes.byref(w), B, T)
        hqd, qkvw = cfg.heads * cfg.head_dim, (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim
        scratch = 2 * max(qkvw * cfg.hidden, cfg.hidden * hqd, 2 * cfg.inter * cfg.hidden, cfg.hidden * cfg.inter)
        rows, kmax = B * T, max(cfg.hidden, cfg.inter, hqd)
        assert got == plain - up(scratch) + up(rows * kmax) + up(rows * 4), (cfg.hidden, B, T)
        assert got < plain
    assert scratch == 2 * 2 * 14336 * 4096  # the 8B geometry: 235 MB that "mxfp4_w4a8" does not take
