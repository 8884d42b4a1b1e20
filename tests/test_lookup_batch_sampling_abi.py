"""CPU: the C surface of prompt-lookup decoding for SAMPLED batches (srgpt_sample_seq_rows, srgpt_sample_full_seq_rows,
srgpt_llm_lookup_batch_sample_ws_bytes, srgpt_llm_lookup_step_batch_ex, srgpt_llm_lookup_graph_create_batch_ex) -- declared, bound and
exported as additions under ABI 9, the workspace formula, and the refusals on the host before any launch (fake non-null pointers that
are never dereferenced, in the manner of tests/test_append_abi.py and tests/test_lookup_batch_abi.py, whose blocks these are)."""
import ctypes
import os
import re
import subprocess

from tests.test_lookup_batch_abi import _state_and_block, _variant, _weights
from tests.util import ROOT

NEW_SYMBOLS = ("srgpt_sample_seq_rows", "srgpt_sample_full_seq_rows", "srgpt_llm_lookup_batch_sample_ws_bytes",
               "srgpt_llm_lookup_step_batch_ex", "srgpt_llm_lookup_graph_create_batch_ex")
P = ctypes.POINTER


def test_symbols_are_declared_bound_and_exported():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "srgpt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    table = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in table.splitlines() if ln.split()}
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and name in exported, name
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(params.split(",")) == len(_lib._SIGNATURES[name][1]), name
    # both stand-alone samplers take the parameter block as const: the counter is the accept's to move
    for name in NEW_SYMBOLS[:2]:
        assert "const srgpt_sampling* sp" in re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1), name
    assert lib.srgpt_abi_version() == _lib.ABI_VERSION == 9  # additions under ABI 9; no struct changed
    from spatialrgpt_amd import ops

    assert callable(ops.sample_seq_rows) and callable(ops.sample_full_seq_rows)


def test_sample_workspace_is_the_samplers_formula_for_B_x_T_rows():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    w = _weights()
    size = lib.srgpt_llm_lookup_batch_sample_ws_bytes
    for B, T in ((1, 2), (2, 2), (2, 4), (4, 4), (3, 5), (8, 2), (1, 16)):
        R = B * T
        assert size(ctypes.byref(w), B, T, _lib.SAMPLER_TOPK64) == lib.srgpt_sample_ws_bytes(R) == 2 * R * 128 * 64 * 4 + 2 * R * 128 * 4 + 256
        assert size(ctypes.byref(w), B, T, _lib.SAMPLER_FULL) == lib.srgpt_sample_full_ws_bytes(R, w.vocab) == R * (4 * w.vocab + 16 + 128 * 8)
    for B, T in ((0, 2), (-1, 2), (2, 1), (2, 0), (2, -4), (2, 9), (9, 2), (17, 2), (1, 17), (5, 4)):
        for kind in (_lib.SAMPLER_TOPK64, _lib.SAMPLER_FULL):
            assert size(ctypes.byref(w), B, T, kind) == -1, (B, T, kind)
    for kind in (2, -1, 7):
        assert size(ctypes.byref(w), 2, 4, kind) == -1, kind
    assert size(ctypes.cast(None, P(_lib.LlmWeights)), 2, 4, _lib.SAMPLER_TOPK64) == -1


def test_batched_ex_entry_points_refuse_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    w = _weights()
    st, lk = _state_and_block()
    sampled = _variant(st, sampling=256)
    by = ctypes.byref
    graph = ctypes.c_void_p()
    entries = {"step": lambda w_, s_, l_, kind=0, ws=256: lib.srgpt_llm_lookup_step_batch_ex(w_, s_, l_, kind, ws, None),
               "graph": lambda w_, s_, l_, kind=0, ws=256: lib.srgpt_llm_lookup_graph_create_batch_ex(w_, s_, l_, kind, ws, None, by(graph))}
    for name, call in entries.items():
        for s_ in (st, sampled):
            # an unknown sampler kind, greedy or sampled, workspace or not
            for kind in (2, -1):
                assert call(by(w), by(s_), by(lk), kind) == _lib.ERR_ARG and b"unknown sampler kind" in lib.srgpt_last_error(), (name, kind)
            # every refusal of srgpt_llm_lookup_step_batch but the greedy-only one
            assert call(by(w), by(s_), ctypes.cast(None, P(_lib.LookupBatch))) == _lib.ERR_ARG, name
            assert call(ctypes.cast(None, P(_lib.LlmWeights)), by(s_), by(lk)) == _lib.ERR_ARG, name
            assert call(by(w), by(_variant(s_, pos=None)), by(lk)) == _lib.ERR_ARG and b"null buffers" in lib.srgpt_last_error()
            for T in (1, 0, -3):
                assert call(by(w), by(s_), by(_variant(lk, T=T))) == _lib.ERR_ARG and b"rows" in lib.srgpt_last_error(), (name, T)
            for bad in (dict(ws=None), dict(logits=None), dict(stats=None), dict(steps=None), dict(n_prompt=None), dict(prompt_ids=None)):
                assert call(by(w), by(s_), by(_variant(lk, **bad))) == _lib.ERR_ARG, (name, bad)
                assert b"null buffers" in lib.srgpt_last_error(), (name, bad)
            assert call(by(w), by(s_), by(_variant(lk, ld_prompt=-1))) == _lib.ERR_ARG and b"ld_prompt" in lib.srgpt_last_error()
            for n in (0, 9):
                assert call(by(w), by(s_), by(_variant(lk, max_ngram=n))) == _lib.ERR_ARG and b"max_ngram" in lib.srgpt_last_error()
            w1 = _weights(heads=4, kv_heads=4)  # G = 1: only the row bound refuses
            for batch, T in ((1, 17), (17, 2), (2, 9), (5, 4)):
                assert call(by(w1), by(_variant(s_, batch=batch)), by(_variant(lk, T=T))) == _lib.ERR_UNSUPPORTED, (name, batch, T)
                msg = lib.srgpt_last_error()
                assert f"batch {batch} x T={T}".encode() in msg and f"{batch * T} rows exceed the 16 rows".encode() in msg, msg
            assert call(by(w), by(s_), by(_variant(lk, T=5))) == _lib.ERR_UNSUPPORTED and b"columns" in lib.srgpt_last_error()
            assert call(by(_variant(w, vocab=262145)), by(s_), by(lk), 1) == _lib.ERR_UNSUPPORTED and b"vocabulary" in lib.srgpt_last_error()
        # sampling set and no sampler workspace, for both kinds
        for kind in (_lib.SAMPLER_TOPK64, _lib.SAMPLER_FULL):
            assert call(by(w), by(sampled), by(lk), kind, None) == _lib.ERR_ARG and b"sample_ws" in lib.srgpt_last_error(), (name, kind)
    assert graph.value is None
    assert lib.srgpt_llm_lookup_graph_create_batch_ex(by(w), by(st), by(lk), 0, None, None, None) == _lib.ERR_ARG


def test_the_plain_batched_entry_points_still_refuse_sampling():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    w = _weights()
    st, lk = _state_and_block()
    sampled = _variant(st, sampling=256)
    graph = ctypes.c_void_p()
    assert lib.srgpt_llm_lookup_step_batch(ctypes.byref(w), ctypes.byref(sampled), ctypes.byref(lk), None) == _lib.ERR_UNSUPPORTED
    assert b"greedy only (st->sampling is set: a sampled batch has one Philox counter" in lib.srgpt_last_error()
    assert lib.srgpt_llm_lookup_graph_create_batch(ctypes.byref(w), ctypes.byref(sampled), ctypes.byref(lk), None,
                                                   ctypes.byref(graph)) == _lib.ERR_UNSUPPORTED
    assert b"greedy only" in lib.srgpt_last_error() and graph.value is None


def test_seq_rows_samplers_refuse_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    good = dict(logits=256, sp=256, steps=256, tok=256, ws=256, B=2, T=4, V=1000)
    for bad in (dict(logits=None), dict(sp=None), dict(steps=None), dict(tok=None), dict(ws=None), dict(B=0), dict(B=-2), dict(T=0),
                dict(T=-1), dict(V=0), dict(V=-5)):
        a = dict(good, **bad)
        assert lib.srgpt_sample_seq_rows(a["logits"], a["sp"], a["steps"], a["tok"], a["ws"], a["B"], a["T"], a["V"], None) == _lib.ERR_ARG, bad
        assert lib.srgpt_sample_full_seq_rows(a["logits"], a["sp"], a["steps"], a["tok"], None, a["ws"], a["B"], a["T"], a["V"],
                                              None) == _lib.ERR_ARG, bad
    assert lib.srgpt_sample_seq_rows(256, 256, 256, 256, 256, 2, 4, 262145, None) == _lib.ERR_UNSUPPORTED
    assert lib.srgpt_sample_full_seq_rows(256, 256, 256, 256, None, 256, 2, 4, 262145, None) == _lib.ERR_UNSUPPORTED
