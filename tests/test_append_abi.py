"""CPU: the append prefill's C surface (srgpt_attention_append, srgpt_llm_prefill_append) -- declared, bound and exported as
additions under ABI 9, and their refusals on the host before any launch (fake non-null pointers that are never dereferenced, in the
manner of tests/test_logits_proc_abi.py).  srgpt_attention_append takes attn_prefill_route unchanged (csrc/attn_route.h says so), so
there is no route of its own to pin."""
import ctypes
import os
import re

from tests.util import ROOT

NEW_SYMBOLS = ("srgpt_attention_append", "srgpt_llm_prefill_append")


def test_symbols_are_declared_bound_and_exported():
    import subprocess

    from spatialrgpt_amd import _lib

    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srgpt.h")).read(), flags=re.S)
    table = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in table.splitlines() if ln.split()}
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and name in exported, name
    assert lib.srgpt_abi_version() == _lib.ABI_VERSION == 9  # additions under ABI 9
    # the declared parameter lists and the bound ones have the same length
    for name in NEW_SYMBOLS:
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(params.split(",")) == len(_lib._SIGNATURES[name][1]), name


def test_attention_append_refuses_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    ok = dict(q=256, k=256, v=256, o=256, B=2, Tq=5, Tk=40, Hq=4, Hkv=2, D=16, q_pos0=256, kv_len=None, dtype=_lib.F32)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.srgpt_attention_append(a["q"], a["k"], a["v"], a["o"], a["B"], a["Tq"], a["Tk"], a["Hq"], a["Hkv"], a["D"],
                                          5 * 64, 64, 16, 2 * 64 * 16, 16, 64 * 16, 2 * 64 * 16, 16, 64 * 16, 0.25, a["q_pos0"],
                                          a["kv_len"], a["dtype"], None)

    for bad in (dict(q=None), dict(k=None), dict(v=None), dict(o=None)):
        assert call(**bad) == _lib.ERR_ARG and b"null pointer" in lib.srgpt_last_error(), bad
    assert call(q_pos0=None) == _lib.ERR_ARG and b"q_pos0 is null" in lib.srgpt_last_error()
    for bad in (dict(B=0), dict(Tq=0), dict(Tk=0), dict(Tk=-3), dict(Hq=0), dict(Hkv=0), dict(Hkv=3), dict(D=0), dict(D=257)):
        assert call(**bad) == _lib.ERR_ARG and b"bad shape" in lib.srgpt_last_error(), bad
    assert call(dtype=7) == _lib.ERR_ARG and b"bad dtype" in lib.srgpt_last_error()


def test_prefill_append_refuses_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    P = ctypes.POINTER
    null_w, null_st = ctypes.cast(None, P(_lib.LlmWeights)), ctypes.cast(None, P(_lib.LlmState))
    assert lib.srgpt_llm_prefill_append(null_w, null_st, 256, 4, None, 0, None, None, None) == _lib.ERR_ARG
    assert b"null" in lib.srgpt_last_error()
    w = _lib.LlmWeights()
    w.dtype, w.hidden, w.inter, w.layers, w.heads, w.kv_heads, w.head_dim, w.vocab = _lib.BF16, 64, 128, 1, 4, 2, 16, 32000
    st = _lib.LlmState()
    st.batch, st.max_pos, st.max_new, st.ws_tokens = 2, 64, 8, 16
    for f in ("kcache", "vcache", "pos", "tok", "out_ids", "step", "ws", "logits"):
        setattr(st, f, 256)  # never dereferenced: every check below fails before a launch

    def call(x=256, T=4, h_pos_max=10, state=st):
        return lib.srgpt_llm_prefill_append(ctypes.byref(w), ctypes.byref(state), x, T, None, h_pos_max, None, None, None)

    assert call(x=None) == _lib.ERR_ARG and b"inputs_embeds is null" in lib.srgpt_last_error()
    for T in (0, -1, 17):  # T <= 0, T > ws_tokens
        assert call(T=T) == _lib.ERR_ARG and b"outside 1 .. ws_tokens=16" in lib.srgpt_last_error(), T
    for h in (-1, -100):
        assert call(h_pos_max=h) == _lib.ERR_ARG and b"is negative" in lib.srgpt_last_error(), h
    for T, h in ((4, 61), (16, 49), (1, 64), (4, 2 ** 31 - 2)):  # h_pos_max + T > max_pos (the sum does not wrap)
        assert call(T=T, h_pos_max=h) == _lib.ERR_ARG and b"exceeds max_pos=64" in lib.srgpt_last_error(), (T, h)
    null_buf = _lib.LlmState()
    ctypes.memmove(ctypes.byref(null_buf), ctypes.byref(st), ctypes.sizeof(st))
    null_buf.pos = None
    assert call(state=null_buf) == _lib.ERR_ARG and b"null buffers" in lib.srgpt_last_error()
