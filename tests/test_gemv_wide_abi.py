"""The wide weight pass's additions to the C ABI (include/srgpt.h: srgpt_gemv_rowss_wide, srgpt_gemv_w4p_wide,
srgpt_gemv_wide_pass_rows, srgpt_llm_weights::decode_pass_rows) and to the Python surface, without a GPU: declared, exported and
listed; the struct mirrors the header and did not move a field; argument errors come back from the host before any launch; the
loader hands the option down and refuses a bad value."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests.util import ROOT

NEW = ("srgpt_gemv_rowss_wide", "srgpt_gemv_w4p_wide", "srgpt_gemv_wide_pass_rows")


def test_new_names_are_declared_exported_and_listed_under_abi_9():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    assert lib.srgpt_abi_version() == _lib.ABI_VERSION == 9
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srgpt.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and name in exported, name
        params = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, hdr)
        assert params, name + " is not declared in include/srgpt.h"
        assert len(params.group(1).split(",")) == len(_lib._SIGNATURES[name][1]), name
    # the wide entries take the arguments of their 16-row forms
    assert _lib._SIGNATURES["srgpt_gemv_rowss_wide"] == _lib._SIGNATURES["srgpt_gemv_rowss"]
    assert _lib._SIGNATURES["srgpt_gemv_w4p_wide"] == _lib._SIGNATURES["srgpt_gemv_w4p"]


def test_weight_struct_field_in_header_order_without_moving_a_field():
    from spatialrgpt_amd import _lib

    names = [f[0] for f in _lib.LlmWeights._fields_]
    src = open(os.path.join(ROOT, "include", "srgpt.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} srgpt_llm_weights;", src).group(1), flags=re.S)
    decl = [re.findall(r"([A-Za-z_0-9]+)\s*$", part.strip())[0] for d in body.split(";") if d.strip() for part in d.split(",")]
    assert decl == names and "decode_pass_rows" in names
    # an int in the four bytes that padded fp8_act in front of the next pointer: every other field where it was, the same size
    W = _lib.LlmWeights
    assert W.decode_pass_rows.offset == W.fp8_act.offset + 4 and W.decode_pass_rows.size == 4
    assert W.wqkv8p.offset == W.fp8_act.offset + 8
    assert ctypes.sizeof(W) == W.pk_rows_qkv.offset + 16 + 8 * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.LlmWeights().decode_pass_rows == 0  # zero-initialised = passes of 16 rows


def test_wide_entries_validate_like_their_16_row_forms():
    """argument errors are detected on the host before any launch (and before the device is asked anything): safe without a GPU"""
    from spatialrgpt_amd import _lib

    lib = _lib.load()

    def rowss(fn, x=16, W=None, W8=16, sc=16, res=None, out=16, batch=20, N=16, K=64, swiglu=0, f32=0, packed=0):
        return fn(x, W, W8, sc, None, 0.0, res, out, batch, N, K, swiglu, f32, None, None, packed, None)

    def w4p(fn, x=16, packed=16, norm=None, res=None, out=16, batch=20, N=16, K=128, swiglu=0, f32=0, ss_in=None, ss_out=None):
        return fn(x, packed, norm, 0.0, res, out, batch, N, K, swiglu, f32, ss_in, ss_out, None)

    for fn in (lib.srgpt_gemv_rowss_wide, lib.srgpt_gemv_rowss):  # the same answers from both
        for missing in ("x", "out"):
            assert rowss(fn, **{missing: None}) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error(), missing
        assert rowss(fn, W8=None) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error()  # neither bf16 nor fp8 weights
        assert rowss(fn, sc=None) == _lib.ERR_ARG and b"row scales" in lib.srgpt_last_error()
        assert rowss(fn, packed=5) == _lib.ERR_ARG and b"packed_rows" in lib.srgpt_last_error()
        assert rowss(fn, packed=4, K=96) == _lib.ERR_ARG and b"packed layout" in lib.srgpt_last_error()
        assert rowss(fn, swiglu=1, res=16) == _lib.ERR_ARG and b"swiglu" in lib.srgpt_last_error()
        assert rowss(fn, swiglu=1, f32=1) == _lib.ERR_ARG and b"swiglu" in lib.srgpt_last_error()
        assert rowss(fn, batch=0) == _lib.ERR_ARG and b"shape" in lib.srgpt_last_error()
        assert rowss(fn, K=12) == _lib.ERR_ARG and b"shape" in lib.srgpt_last_error()
    for fn in (lib.srgpt_gemv_w4p_wide, lib.srgpt_gemv_w4p):
        for missing in ("x", "packed", "out"):
            assert w4p(fn, **{missing: None}) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error(), missing
        assert w4p(fn, K=96) == _lib.ERR_ARG and b"multiple of 128" in lib.srgpt_last_error()
        assert w4p(fn, N=24, swiglu=1) == _lib.ERR_ARG and b"granule" in lib.srgpt_last_error()
        assert w4p(fn, swiglu=1, res=16) == _lib.ERR_ARG and b"swiglu" in lib.srgpt_last_error()
        assert w4p(fn, ss_in=16) == _lib.ERR_ARG and b"norm_w" in lib.srgpt_last_error()
        assert w4p(fn, ss_out=16, f32=1) == _lib.ERR_ARG and b"statistics" in lib.srgpt_last_error()
        assert w4p(fn, batch=0) == _lib.ERR_ARG and b"shape" in lib.srgpt_last_error()


def test_pass_rows_query_is_the_routes_answer():
    from spatialrgpt_amd import _lib, ops

    lib = _lib.load()
    for batch in (2, 9, 16):  # 16 rows or fewer: the 16-row route
        assert lib.srgpt_gemv_wide_pass_rows(batch, 0, 0, 0, 4096, 4096, 0, 0) == 16
        assert lib.srgpt_gemv_wide_pass_rows(batch, 0, 16, 1, 4096, 4096, 1, 0) == 16
    for batch in (17, 32, 33, 64):
        for fp8, packed, w4 in ((0, 0, 0), (1, 0, 0), (1, 4, 0), (1, 16, 0), (0, 16, 1)):
            got = lib.srgpt_gemv_wide_pass_rows(batch, fp8, packed, w4, 4096, 4096, 0, 0)
            assert got in (16, 32), (batch, fp8, packed, w4, got)
            assert got == ops.gemv_wide_pass_rows(batch, 4096, 4096, fp8=bool(fp8), packed_rows=packed, w4=bool(w4))
    assert lib.srgpt_gemv_wide_pass_rows(1, 1, 0, 0, 4096, 4096, 0, 0) == 1  # one fp8 row: the VALU kernel's chunk


def test_a_step_entry_refuses_other_pass_rows():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    w, st = _lib.LlmWeights(), _lib.LlmState()
    w.dtype, w.hidden, w.inter, w.layers, w.heads, w.kv_heads, w.head_dim, w.vocab = _lib.BF16, 64, 128, 1, 2, 2, 32, 100
    for f in ("kcache", "vcache", "pos", "tok", "out_ids", "step", "ws", "logits"):
        setattr(st, f, 16)
    st.batch, st.max_pos, st.max_new, st.ws_tokens = 20, 64, 4, 32
    for bad in (24, 8, 1, -1, 64):
        w.decode_pass_rows = bad
        rc = lib.srgpt_llm_decode_step(ctypes.byref(w), ctypes.byref(st), None)
        assert rc == _lib.ERR_ARG and b"decode_pass_rows" in lib.srgpt_last_error(), bad
        rc = lib.srgpt_llm_decode_step_ex(ctypes.byref(w), ctypes.byref(st), 0, None)
        assert rc == _lib.ERR_ARG and b"decode_pass_rows" in lib.srgpt_last_error(), bad
        graph = _lib.vp()
        rc = lib.srgpt_llm_decode_graph_create(ctypes.byref(w), ctypes.byref(st), None, ctypes.byref(graph))
        assert rc == _lib.ERR_ARG and b"decode_pass_rows" in lib.srgpt_last_error() and not graph.value, bad


def test_bad_option_values_raise_before_any_device_work():
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.weights import PreparedWeights

    for bad in (0, 8, 24, 64, True, None, "32"):
        with pytest.raises(ValueError, match="decode_pass_rows"):
            PreparedWeights(SrgptConfig(), {}, "cpu", torch.bfloat16, parts=(), decode_pass_rows=bad)


def test_loader_hands_the_option_down(monkeypatch):
    """load_pretrained_model(..., decode_pass_rows=) -> LlavaLlamaModel(..., decode_pass_rows=) (the model hands it to SrgptEngine, the
    engine to PreparedWeights, which writes srgpt_llm_weights::decode_pass_rows: tests/test_gpu_wide_step.py reads it there)"""
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
    builder.load_pretrained_model("nowhere", "tiny", decode_pass_rows=32)
    builder.load_pretrained_model("nowhere", "tiny")
    assert [kw["decode_pass_rows"] for kw in seen] == [32, 16]
