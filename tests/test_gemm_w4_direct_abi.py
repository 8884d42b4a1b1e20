"""The `_direct` W4 products' additions to the C ABI (include/srgpt.h: srgpt_gemm_w4_direct, _norm_direct, _swiglu_direct,
_rope_kv_append_direct, srgpt_gemm_w4_direct_in_kernel, srgpt_llm_weights::mxfp4_direct) and to the Python surface, without a GPU:
declared, exported and listed with the signatures of their plain counterparts; the struct mirrors the header and did not move a
field; argument errors come back from the host before any launch; the loader hands the option down and refuses it for another
weight format."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests.util import ROOT

PAIRS = {"srgpt_gemm_w4_direct": "srgpt_gemm_w4", "srgpt_gemm_w4_norm_direct": "srgpt_gemm_w4_norm",
         "srgpt_gemm_w4_swiglu_direct": "srgpt_gemm_w4_swiglu", "srgpt_gemm_w4_rope_kv_append_direct": "srgpt_gemm_w4_rope_kv_append",
         "srgpt_gemm_w4_direct_in_kernel": "srgpt_gemm_w4_in_kernel"}


def test_new_names_are_declared_exported_and_listed_under_abi_9():
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

    for name, plain in PAIRS.items():
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and name in exported, name
        assert params(name) == params(plain), name + " does not take its plain counterpart's arguments"
        assert _lib._SIGNATURES[name] == _lib._SIGNATURES[plain] and len(params(name)) == len(_lib._SIGNATURES[name][1]), name


def test_weight_struct_field_fills_padding_without_moving_a_field():
    from spatialrgpt_amd import _lib

    names = [f[0] for f in _lib.LlmWeights._fields_]
    src = open(os.path.join(ROOT, "include", "srgpt.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} srgpt_llm_weights;", src).group(1), flags=re.S)
    decl = [re.findall(r"([A-Za-z_0-9]+)\s*$", part.strip())[0] for d in body.split(";") if d.strip() for part in d.split(",")]
    assert decl == names and "mxfp4_direct" in names
    W = _lib.LlmWeights
    # eight ints and a float, then the int in the four bytes that padded rms_eps in front of the first pointer
    assert W.rms_eps.offset == 32 and W.mxfp4_direct.offset == W.rms_eps.offset + 4 and W.mxfp4_direct.size == 4
    assert W.rope_cos.offset == 40
    assert W.fp8_act.offset == 40 + 21 * 8 and W.decode_pass_rows.offset == W.fp8_act.offset + 4  # 5 + 6 + 2 + 8 pointers between
    assert ctypes.sizeof(W) == W.pk_rows_qkv.offset + 16 + 8 * ctypes.sizeof(ctypes.c_void_p) == 40 + 21 * 8 + 8 + 4 * 8 + 16 + 8 * 8
    assert _lib.LlmWeights().mxfp4_direct == 0  # zero-initialised = the plain entries


def test_llm_entry_points_refuse_a_bad_mxfp4_direct():
    """2 (or any value but 0 / 1), and 1 without MXFP4 weights: SRGPT_ERR_ARG on the host before any launch -- safe without a GPU"""
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    w, st = _lib.LlmWeights(), _lib.LlmState()
    w.dtype, w.hidden, w.inter, w.layers, w.heads, w.kv_heads, w.head_dim, w.vocab = _lib.BF16, 64, 128, 1, 2, 2, 32, 100
    for f in ("kcache", "vcache", "pos", "tok", "out_ids", "step", "ws", "logits"):
        setattr(st, f, 16)
    st.batch, st.max_pos, st.max_new, st.ws_tokens = 1, 64, 4, 32
    some = (_lib.vp * 1)(16)
    for bad, with_codes in ((2, False), (-1, False), (1, False), (2, True), (7, True)):
        w.mxfp4_direct = bad
        w.wqkv4 = some if with_codes else None
        rc = lib.srgpt_llm_decode_step(ctypes.byref(w), ctypes.byref(st), None)
        assert rc == _lib.ERR_ARG and b"mxfp4_direct" in lib.srgpt_last_error(), (bad, with_codes)
        rc = lib.srgpt_llm_decode_step_ex(ctypes.byref(w), ctypes.byref(st), 0, None)
        assert rc == _lib.ERR_ARG and b"mxfp4_direct" in lib.srgpt_last_error(), (bad, with_codes)
        graph = _lib.vp()
        rc = lib.srgpt_llm_decode_graph_create(ctypes.byref(w), ctypes.byref(st), None, ctypes.byref(graph))
        assert rc == _lib.ERR_ARG and b"mxfp4_direct" in lib.srgpt_last_error() and not graph.value, (bad, with_codes)
        rc = lib.srgpt_llm_prefill(ctypes.byref(w), ctypes.byref(st), 16, 8, None, None, None)
        assert rc == _lib.ERR_ARG and b"mxfp4_direct" in lib.srgpt_last_error(), (bad, with_codes)
        rc = lib.srgpt_llm_prefill_append(ctypes.byref(w), ctypes.byref(st), 16, 8, None, 4, None, None, None)
        assert rc == _lib.ERR_ARG and b"mxfp4_direct" in lib.srgpt_last_error(), (bad, with_codes)


def test_direct_entries_validate_like_the_plain_ones():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    for fn in (lib.srgpt_gemm_w4_direct, lib.srgpt_gemm_w4):
        assert fn(16, None, 16, None, 16, 4, 4, 64, 64, 4, 0, None, None, 0, None) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error()
        assert fn(16, 16, None, None, 16, 4, 4, 64, 64, 4, 0, None, None, 0, None) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error()
        assert fn(None, 16, 16, None, 16, 4, 4, 64, 64, 4, 0, None, None, 0, None) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error()
    for fn in (lib.srgpt_gemm_w4_norm_direct, lib.srgpt_gemm_w4_norm):
        assert fn(16, None, 16, None, 16, 4, 4, 64, None, None, 0, 16, 32, 1e-5, None) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error()
    for fn in (lib.srgpt_gemm_w4_swiglu_direct, lib.srgpt_gemm_w4_swiglu):
        assert fn(16, 16, None, 16, 4, 4, 64, None, None, None, 0, None) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error()
    for fn in (lib.srgpt_gemm_w4_rope_kv_append_direct, lib.srgpt_gemm_w4_rope_kv_append):
        assert fn(16, None, 16, 16, 64, None, None, 0, 16, 16, None, 16, 16, 1, 4, 2, 1, 16, 8, None) == _lib.ERR_ARG
        assert b"null" in lib.srgpt_last_error()
    for fn in (lib.srgpt_gemm_w4_direct_in_kernel, lib.srgpt_gemm_w4_in_kernel):  # shapes outside the domain answer 0 before the device is asked
        assert fn(0, 64, 64, 0, 0, 0) == 0 and fn(4, 64, 48, 0, 0, 0) == 0


def test_option_is_refused_for_other_formats_before_any_device_work():
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.weights import PreparedWeights

    for fmt in ("native", "fp8", "fp8_w8a8"):
        with pytest.raises(ValueError, match="mxfp4_prefill_direct"):
            PreparedWeights(SrgptConfig(), {}, "cpu", torch.bfloat16, parts=(), llm_weight_format=fmt, mxfp4_prefill_direct=True)
    w = PreparedWeights(SrgptConfig(), {}, "cpu", torch.bfloat16, parts=(), llm_weight_format="mxfp4", mxfp4_prefill_direct=True)
    assert w.mxfp4_prefill_direct is True
    assert PreparedWeights(SrgptConfig(), {}, "cpu", torch.bfloat16, parts=()).mxfp4_prefill_direct is False


def test_loader_hands_the_option_down(monkeypatch):
    """load_pretrained_model(..., mxfp4_prefill_direct=) -> LlavaLlamaModel(..., mxfp4_prefill_direct=); the model hands it to
    SrgptEngine, the engine to PreparedWeights, which writes srgpt_llm_weights::mxfp4_direct (tests/test_gpu_mxfp4_prefill_direct.py
    reads it there)"""
    import inspect

    import spatialrgpt_amd.builder as builder
    import spatialrgpt_amd.model as model
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine

    seen = []

    class Stub:
        def __init__(self, *a, **kw):
            seen.append(kw)

    for fn in (model.LlavaLlamaModel.__init__, SrgptEngine.__init__, builder.load_model):
        assert inspect.signature(fn).parameters["mxfp4_prefill_direct"].default is False
    assert isinstance(SrgptEngine.mxfp4_prefill_direct, property) and SrgptEngine.mxfp4_prefill_direct.fset is None
    monkeypatch.setattr(builder, "read_checkpoint", lambda *a, **kw: (SrgptConfig(), {}))
    monkeypatch.setattr(builder, "load_tokenizer", lambda *a, **kw: None)
    monkeypatch.setattr(builder, "load_image_processor", lambda *a, **kw: None)
    monkeypatch.setattr(builder, "_read_json", lambda p: {})
    monkeypatch.setattr(model, "LlavaLlamaModel", Stub)
    builder.load_pretrained_model("nowhere", "tiny", llm_weight_format="mxfp4", mxfp4_prefill_direct=True)
    builder.load_pretrained_model("nowhere", "tiny")
    assert [(kw["llm_weight_format"], kw["mxfp4_prefill_direct"]) for kw in seen] == [("mxfp4", True), ("native", False)]
