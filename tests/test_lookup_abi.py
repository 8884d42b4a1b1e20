"""CPU: the C surface of prompt-lookup decoding (srgpt_decode_attention_multi, srgpt_lookup_draft / _accept, srgpt_llm_lookup_*) --
declared, bound and exported as additions under ABI 9, and their refusals on the host before any launch (fake non-null pointers
that are never dereferenced, in the manner of tests/test_append_abi.py)."""
import ctypes
import os
import re
import subprocess

from tests.util import ROOT

NEW_SYMBOLS = ("srgpt_decode_attn_multi_ws_floats", "srgpt_decode_attention_multi", "srgpt_lookup_draft", "srgpt_lookup_accept",
               "srgpt_llm_lookup_ws_bytes", "srgpt_llm_lookup_step", "srgpt_llm_lookup_graph_create", "srgpt_llm_lookup_sync_state")


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
    # the parameter block's fields, in the header's order
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} srgpt_lookup;", text).group(1), flags=re.S)
    fields = [re.findall(r"([A-Za-z_0-9]+)\s*$", d.strip())[0] for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.Lookup._fields_]


def test_workspace_sizes():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    assert lib.srgpt_decode_attn_multi_ws_floats(1, 4, 32, 128) == 4 * 32 * 64 * 130 + 32
    assert lib.srgpt_decode_attn_multi_ws_floats(2, 3, 8, 16) == 2 * 3 * 8 * 64 * 18 + 2 * 8
    w = _lib.LlmWeights()
    w.dtype, w.hidden, w.inter, w.layers, w.heads, w.kv_heads, w.head_dim, w.vocab = _lib.BF16, 512, 1024, 2, 4, 1, 128, 4000
    a256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for T in (2, 4, 16):
        want = (a256(T * 512 * 2) + a256(T * 6 * 128 * 2) + a256(T * 512 * 2) + a256(T * 1024 * 2) + a256(2 * T * 512 * 4) +
                a256((T * 4 * 64 * 130 + 4) * 4) + 2 * a256(T * 128 * 4) + 2 * a256(T * 8) + 256)
        assert lib.srgpt_llm_lookup_ws_bytes(ctypes.byref(w), T) == want, T
    for T in (1, 0, 17):
        assert lib.srgpt_llm_lookup_ws_bytes(ctypes.byref(w), T) == -1
    assert lib.srgpt_llm_lookup_ws_bytes(ctypes.cast(None, ctypes.POINTER(_lib.LlmWeights)), 4) == -1


def test_decode_attention_multi_refuses_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    ok = dict(qkv=256, kc=256, vc=256, pos=256, ct=256, st=256, out=256, ws=256, B=1, T=4, Hq=8, Hkv=2, D=128, max_pos=512, dtype=_lib.BF16)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.srgpt_decode_attention_multi(a["qkv"], a["kc"], a["vc"], a["pos"], a["ct"], a["st"], a["out"], a["ws"], a["B"], a["T"],
                                                a["Hq"], a["Hkv"], a["D"], a["max_pos"], a["dtype"], None)

    for name in ("qkv", "kc", "vc", "pos", "ct", "st", "out", "ws"):
        assert call(**{name: None}) == _lib.ERR_ARG and b"null pointer" in lib.srgpt_last_error(), name
    for bad in (dict(B=0), dict(T=0), dict(T=-2), dict(Hq=0), dict(Hkv=0), dict(Hkv=3), dict(D=0), dict(D=258), dict(D=33), dict(max_pos=0)):
        assert call(**bad) == _lib.ERR_ARG and b"bad shape" in lib.srgpt_last_error(), bad
    assert call(dtype=7) == _lib.ERR_ARG and b"bad dtype" in lib.srgpt_last_error()
    # T * G beyond the 16 columns of the MFMA kernel: G = 4 -> T <= 4, G = 1 -> 16, G = 8 -> 2
    for Hq, Hkv, T in ((8, 2, 5), (4, 4, 17), (8, 1, 3), (4, 2, 9)):
        assert call(Hq=Hq, Hkv=Hkv, T=T) == _lib.ERR_UNSUPPORTED and b"columns" in lib.srgpt_last_error(), (Hq, Hkv, T)


def test_lookup_kernels_refuse_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()

    def draft(prompt=256, n_prompt=5, out_ids=256, step=256, max_new=8, K=3, max_ngram=2, vocab=100, d=256, nd=256):
        return lib.srgpt_lookup_draft(prompt, n_prompt, out_ids, step, max_new, K, max_ngram, vocab, d, nd, None)

    for bad in (dict(prompt=None), dict(out_ids=None), dict(step=None), dict(d=None), dict(nd=None)):
        assert draft(**bad) == _lib.ERR_ARG and b"null pointer" in lib.srgpt_last_error(), bad
    for bad in (dict(n_prompt=-1), dict(max_new=0), dict(vocab=0)):
        assert draft(**bad) == _lib.ERR_ARG and b"bad sizes" in lib.srgpt_last_error(), bad
    for K in (0, -1, 16):
        assert draft(K=K) == _lib.ERR_ARG and b"drafts outside" in lib.srgpt_last_error(), K
    for n in (0, 9):
        assert draft(max_ngram=n) == _lib.ERR_ARG and b"max_ngram" in lib.srgpt_last_error(), n

    def accept(picks=256, d=256, nd=256, T=4, tok=256, out_ids=256, pos=256, step=256, max_new=8, max_pos=64):
        return lib.srgpt_lookup_accept(picks, d, nd, T, tok, out_ids, pos, step, max_new, max_pos, None, None, None)

    for bad in (dict(picks=None), dict(d=None), dict(nd=None), dict(tok=None), dict(out_ids=None), dict(pos=None), dict(step=None)):
        assert accept(**bad) == _lib.ERR_ARG and b"null pointer" in lib.srgpt_last_error(), bad
    for bad in (dict(T=1), dict(T=17), dict(max_new=0), dict(max_pos=0)):
        assert accept(**bad) == _lib.ERR_ARG and b"bad sizes" in lib.srgpt_last_error(), bad


def test_lookup_step_refuses_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    P = ctypes.POINTER
    w = _lib.LlmWeights()
    w.dtype, w.hidden, w.inter, w.layers, w.heads, w.kv_heads, w.head_dim, w.vocab = _lib.BF16, 512, 1024, 2, 8, 2, 128, 4000
    st = _lib.LlmState()
    st.batch, st.max_pos, st.max_new, st.ws_tokens = 1, 512, 16, 32
    for f in ("kcache", "vcache", "pos", "tok", "out_ids", "step", "ws", "logits"):
        setattr(st, f, 256)  # never dereferenced: every check below fails before a launch
    lk = _lib.Lookup()
    lk.T, lk.max_ngram, lk.prompt_ids, lk.n_prompt, lk.ws, lk.logits, lk.stats = 4, 2, 256, 7, 256, 256, 256

    def variant(obj, **kw):
        c = type(obj)()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(obj), ctypes.sizeof(obj))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    graph = ctypes.c_void_p()
    entries = {"step": lambda w_, s_, l_: lib.srgpt_llm_lookup_step(w_, s_, l_, None),
               "graph": lambda w_, s_, l_: lib.srgpt_llm_lookup_graph_create(w_, s_, l_, None, ctypes.byref(graph))}
    for name, call in entries.items():
        assert call(ctypes.byref(w), ctypes.byref(st), ctypes.cast(None, P(_lib.Lookup))) == _lib.ERR_ARG, name
        assert call(ctypes.cast(None, P(_lib.LlmWeights)), ctypes.byref(st), ctypes.byref(lk)) == _lib.ERR_ARG, name
        assert call(ctypes.byref(w), ctypes.byref(variant(st, batch=2)), ctypes.byref(lk)) == _lib.ERR_ARG and b"batch 2" in lib.srgpt_last_error()
        assert call(ctypes.byref(w), ctypes.byref(variant(st, pos=None)), ctypes.byref(lk)) == _lib.ERR_ARG and b"null buffers" in lib.srgpt_last_error()
        for T in (1, 0, -3):
            assert call(ctypes.byref(w), ctypes.byref(st), ctypes.byref(variant(lk, T=T))) == _lib.ERR_ARG and b"rows" in lib.srgpt_last_error()
        for bad in (dict(ws=None), dict(logits=None), dict(stats=None), dict(prompt_ids=None), dict(n_prompt=-1)):
            assert call(ctypes.byref(w), ctypes.byref(st), ctypes.byref(variant(lk, **bad))) == _lib.ERR_ARG, (name, bad)
            assert b"null buffers" in lib.srgpt_last_error(), (name, bad)
        assert call(ctypes.byref(w), ctypes.byref(st), ctypes.byref(variant(lk, prompt_ids=None, n_prompt=0, T=5))) == _lib.ERR_UNSUPPORTED
        for n in (0, 9):
            assert call(ctypes.byref(w), ctypes.byref(st), ctypes.byref(variant(lk, max_ngram=n))) == _lib.ERR_ARG and b"max_ngram" in lib.srgpt_last_error()
        # greedy only
        assert call(ctypes.byref(w), ctypes.byref(variant(st, sampling=256)), ctypes.byref(lk)) == _lib.ERR_UNSUPPORTED
        assert b"greedy only" in lib.srgpt_last_error(), name
        # G = 4: five rows do not fit the attention's 16 columns; 17 rows fit no route
        assert call(ctypes.byref(w), ctypes.byref(st), ctypes.byref(variant(lk, T=5))) == _lib.ERR_UNSUPPORTED and b"columns" in lib.srgpt_last_error()
        assert call(ctypes.byref(variant(w, dtype=_lib.F32)), ctypes.byref(st), ctypes.byref(variant(lk, T=17))) == _lib.ERR_UNSUPPORTED
    assert graph.value is None
    assert lib.srgpt_llm_lookup_graph_create(ctypes.byref(w), ctypes.byref(st), ctypes.byref(lk), None, None) == _lib.ERR_ARG
    assert lib.srgpt_llm_lookup_sync_state(ctypes.byref(w), ctypes.byref(st), ctypes.cast(None, P(_lib.Lookup)), None) == _lib.ERR_ARG
    assert lib.srgpt_llm_lookup_sync_state(ctypes.byref(w), ctypes.byref(st), ctypes.byref(variant(lk, ws=None)), None) == _lib.ERR_ARG
