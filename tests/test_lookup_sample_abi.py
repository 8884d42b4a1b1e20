"""CPU: the C surface of prompt-lookup decoding under sampling (srgpt_sample_rows, srgpt_sample_full_rows,
srgpt_llm_lookup_sample_ws_bytes, srgpt_llm_lookup_step_ex, srgpt_llm_lookup_graph_create_ex) -- declared, bound and exported as
additions under ABI 9, the workspace formula, and the refusals on the host before any launch (fake non-null pointers that are never
dereferenced, in the manner of tests/test_lookup_abi.py)."""
import ctypes
import os
import re
import subprocess

from tests.util import ROOT

NEW_SYMBOLS = ("srgpt_sample_rows", "srgpt_sample_full_rows", "srgpt_llm_lookup_sample_ws_bytes", "srgpt_llm_lookup_step_ex",
               "srgpt_llm_lookup_graph_create_ex")
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
    assert lib.srgpt_abi_version() == _lib.ABI_VERSION == 9  # additions under ABI 9
    # the ops wrappers and the switch exist
    from spatialrgpt_amd import ops
    from spatialrgpt_amd.generation import plan_lookup  # noqa: F401

    assert callable(ops.sample_rows) and callable(ops.sample_full_rows)


def _weights(_lib, **kw):
    w = _lib.LlmWeights()
    w.dtype, w.hidden, w.inter, w.layers, w.heads, w.kv_heads, w.head_dim, w.vocab = _lib.BF16, 512, 1024, 2, 8, 2, 128, 4000
    for k, v in kw.items():
        setattr(w, k, v)
    return w


def test_sample_workspace_is_the_samplers_formula_for_T_rows():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    w = _weights(_lib)
    for T in (2, 4, 16):
        # top-k-64: candidate keys and indices [T][128][64] x 4 bytes each, the slices' maxima and their indices [T][128], the error word
        assert lib.srgpt_llm_lookup_sample_ws_bytes(ctypes.byref(w), T, _lib.SAMPLER_TOPK64) == 2 * T * 128 * 64 * 4 + 2 * T * 128 * 4 + 256
        assert lib.srgpt_llm_lookup_sample_ws_bytes(ctypes.byref(w), T, _lib.SAMPLER_TOPK64) == lib.srgpt_sample_ws_bytes(T)
        # full: keys [T][V], a threshold block of 16 bytes per row, the slices' maxima and their indices
        assert lib.srgpt_llm_lookup_sample_ws_bytes(ctypes.byref(w), T, _lib.SAMPLER_FULL) == T * (4 * 4000 + 16 + 128 * 8)
        assert lib.srgpt_llm_lookup_sample_ws_bytes(ctypes.byref(w), T, _lib.SAMPLER_FULL) == lib.srgpt_sample_full_ws_bytes(T, 4000)
    for T in (1, 0, -1, 17):
        for kind in (_lib.SAMPLER_TOPK64, _lib.SAMPLER_FULL):
            assert lib.srgpt_llm_lookup_sample_ws_bytes(ctypes.byref(w), T, kind) == -1, (T, kind)
    for kind in (2, -1, 7):
        assert lib.srgpt_llm_lookup_sample_ws_bytes(ctypes.byref(w), 4, kind) == -1, kind
    assert lib.srgpt_llm_lookup_sample_ws_bytes(ctypes.cast(None, P(_lib.LlmWeights)), 4, _lib.SAMPLER_TOPK64) == -1


def _blocks(_lib):
    st = _lib.LlmState()
    st.batch, st.max_pos, st.max_new, st.ws_tokens = 1, 512, 16, 32
    for f in ("kcache", "vcache", "pos", "tok", "out_ids", "step", "ws", "logits"):
        setattr(st, f, 256)  # never dereferenced: every check below fails before a launch
    lk = _lib.Lookup()
    lk.T, lk.max_ngram, lk.prompt_ids, lk.n_prompt, lk.ws, lk.logits, lk.stats = 4, 2, 256, 7, 256, 256, 256
    return st, lk


def _variant(obj, **kw):
    c = type(obj)()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(obj), ctypes.sizeof(obj))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_ex_entry_points_refuse_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    w = _weights(_lib)
    st, lk = _blocks(_lib)
    sampled = _variant(st, sampling=256)
    graph = ctypes.c_void_p()
    entries = {"step": lambda w_, s_, l_, kind, ws: lib.srgpt_llm_lookup_step_ex(w_, s_, l_, kind, ws, None),
               "graph": lambda w_, s_, l_, kind, ws: lib.srgpt_llm_lookup_graph_create_ex(w_, s_, l_, kind, ws, None, ctypes.byref(graph))}
    for name, call in entries.items():
        for s_ in (st, sampled):
            # an unknown sampler kind, greedy or sampled, workspace or not
            for kind in (2, -1):
                assert call(ctypes.byref(w), ctypes.byref(s_), ctypes.byref(lk), kind, 256) == _lib.ERR_ARG, (name, kind)
                assert b"unknown sampler kind" in lib.srgpt_last_error(), name
            # every refusal of the greedy entry point but the greedy-only one
            assert call(ctypes.byref(w), ctypes.byref(s_), ctypes.cast(None, P(_lib.Lookup)), 0, 256) == _lib.ERR_ARG, name
            assert call(ctypes.cast(None, P(_lib.LlmWeights)), ctypes.byref(s_), ctypes.byref(lk), 0, 256) == _lib.ERR_ARG, name
            assert call(ctypes.byref(w), ctypes.byref(_variant(s_, batch=2)), ctypes.byref(lk), 0, 256) == _lib.ERR_ARG
            assert b"batch 2" in lib.srgpt_last_error(), name
            for T in (1, 0):
                assert call(ctypes.byref(w), ctypes.byref(s_), ctypes.byref(_variant(lk, T=T)), 0, 256) == _lib.ERR_ARG and b"rows" in lib.srgpt_last_error()
            for bad in (dict(ws=None), dict(logits=None), dict(stats=None)):
                assert call(ctypes.byref(w), ctypes.byref(s_), ctypes.byref(_variant(lk, **bad)), 0, 256) == _lib.ERR_ARG, (name, bad)
                assert b"null buffers" in lib.srgpt_last_error(), (name, bad)
            assert call(ctypes.byref(w), ctypes.byref(s_), ctypes.byref(_variant(lk, T=5)), 0, 256) == _lib.ERR_UNSUPPORTED
            assert b"columns" in lib.srgpt_last_error(), name
            assert call(ctypes.byref(_variant(w, vocab=262145)), ctypes.byref(s_), ctypes.byref(lk), 1, 256) == _lib.ERR_UNSUPPORTED
            assert b"vocabulary" in lib.srgpt_last_error(), name
        # sampling set and no sampler workspace, for both kinds
        for kind in (_lib.SAMPLER_TOPK64, _lib.SAMPLER_FULL):
            assert call(ctypes.byref(w), ctypes.byref(sampled), ctypes.byref(lk), kind, None) == _lib.ERR_ARG, (name, kind)
            assert b"sample_ws" in lib.srgpt_last_error(), (name, kind)
    assert graph.value is None
    assert lib.srgpt_llm_lookup_graph_create_ex(ctypes.byref(w), ctypes.byref(st), ctypes.byref(lk), 0, None, None, None) == _lib.ERR_ARG


def test_the_plain_entry_points_still_refuse_sampling():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    w = _weights(_lib)
    st, lk = _blocks(_lib)
    sampled = _variant(st, sampling=256)
    graph = ctypes.c_void_p()
    assert lib.srgpt_llm_lookup_step(ctypes.byref(w), ctypes.byref(sampled), ctypes.byref(lk), None) == _lib.ERR_UNSUPPORTED
    assert b"greedy only" in lib.srgpt_last_error()
    assert lib.srgpt_llm_lookup_graph_create(ctypes.byref(w), ctypes.byref(sampled), ctypes.byref(lk), None, ctypes.byref(graph)) == _lib.ERR_UNSUPPORTED
    assert b"greedy only" in lib.srgpt_last_error() and graph.value is None


def test_rows_samplers_refuse_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    for bad in (dict(logits=None), dict(sp=None), dict(tok=None), dict(ws=None), dict(T=0), dict(V=0)):
        a = dict(dict(logits=256, sp=256, tok=256, ws=256, T=4, V=1000), **bad)
        assert lib.srgpt_sample_rows(a["logits"], a["sp"], a["tok"], a["ws"], a["T"], a["V"], None) == _lib.ERR_ARG, bad
        assert lib.srgpt_sample_full_rows(a["logits"], a["sp"], a["tok"], None, a["ws"], a["T"], a["V"], None) == _lib.ERR_ARG, bad
    assert lib.srgpt_sample_rows(256, 256, 256, 256, 4, 262145, None) == _lib.ERR_UNSUPPORTED
    assert lib.srgpt_sample_full_rows(256, 256, 256, None, 256, 4, 262145, None) == _lib.ERR_UNSUPPORTED
