"""CPU: the C surface of the batched lookup step (srgpt_lookup_draft_batch / _accept_batch, srgpt_llm_lookup_*_batch and the
srgpt_lookup_batch block) -- declared, bound and exported as additions under ABI 9 -- and its refusals on the host before any launch
(fake non-null pointers that are never dereferenced, in the manner of tests/test_lookup_abi.py).  The batch-1 entry points keep
refusing a state of two sequences."""
import ctypes
import os
import re
import subprocess

from tests.util import ROOT

NEW_SYMBOLS = ("srgpt_lookup_draft_batch", "srgpt_lookup_accept_batch", "srgpt_llm_lookup_batch_ws_bytes", "srgpt_llm_lookup_step_batch",
               "srgpt_llm_lookup_graph_create_batch", "srgpt_llm_lookup_sync_state_batch")
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
    # the parameter block's fields, in the header's order; the batch-1 block is as it was
    for struct, mirror in (("srgpt_lookup_batch", _lib.LookupBatch), ("srgpt_lookup", _lib.Lookup)):
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} " + struct + ";", text).group(1), flags=re.S)
        fields = [re.findall(r"([A-Za-z_0-9]+)\s*$", d.strip())[0] for d in body.split(";") if d.strip()]
        assert fields == [f[0] for f in mirror._fields_], struct
    assert [f[0] for f in _lib.LookupBatch._fields_] == ["T", "max_ngram", "prompt_ids", "ld_prompt", "n_prompt", "steps", "ws", "logits", "stats"]
    assert [f[0] for f in _lib.Lookup._fields_] == ["T", "max_ngram", "prompt_ids", "n_prompt", "ws", "logits", "stats"]


def _weights(**kw):
    from spatialrgpt_amd import _lib

    w = _lib.LlmWeights()
    w.dtype, w.hidden, w.inter, w.layers, w.heads, w.kv_heads, w.head_dim, w.vocab = _lib.BF16, 512, 1024, 2, 4, 1, 128, 4000
    for k, v in kw.items():
        setattr(w, k, v)
    return w


def test_workspace_sizes():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    w = _weights()
    a256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
    sizes = {}
    for B, T in ((1, 2), (1, 4), (2, 2), (2, 4), (4, 2), (4, 4), (8, 2), (3, 5), (1, 16)):
        R = B * T
        want = (a256(R * 512 * 2) + a256(R * 6 * 128 * 2) + a256(R * 512 * 2) + a256(R * 1024 * 2) + a256(2 * R * 512 * 4) +
                a256(lib.srgpt_decode_attn_multi_ws_floats(B, T, 4, 128) * 4) + 2 * a256(R * 128 * 4) + 2 * a256(R * 8) + a256(R * 4))
        sizes[B, T] = lib.srgpt_llm_lookup_batch_ws_bytes(ctypes.byref(w), B, T)
        assert sizes[B, T] == want, (B, T)
    assert sizes[1, 4] < sizes[2, 4] < sizes[4, 4] and sizes[1, 2] < sizes[2, 2] < sizes[4, 2] < sizes[8, 2]  # grows with B
    for B, T in ((0, 4), (-1, 4), (2, 1), (2, 0), (1, 17), (2, 9), (4, 5), (8, 3), (9, 2), (17, 1)):
        assert lib.srgpt_llm_lookup_batch_ws_bytes(ctypes.byref(w), B, T) == -1, (B, T)
    assert lib.srgpt_llm_lookup_batch_ws_bytes(ctypes.cast(None, P(_lib.LlmWeights)), 2, 4) == -1


def test_batched_kernels_refuse_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()

    def draft(prompt=256, ld=5, n_prompt=256, out_ids=256, steps=256, B=2, max_new=8, K=3, max_ngram=2, vocab=100, d=256, nd=256):
        return lib.srgpt_lookup_draft_batch(prompt, ld, n_prompt, out_ids, steps, B, max_new, K, max_ngram, vocab, d, nd, None)

    for bad in (dict(prompt=None), dict(n_prompt=None), dict(out_ids=None), dict(steps=None), dict(d=None), dict(nd=None)):
        assert draft(**bad) == _lib.ERR_ARG and b"null pointer" in lib.srgpt_last_error(), bad
    for bad in (dict(B=0), dict(B=17), dict(ld=-1), dict(max_new=0), dict(vocab=0)):
        assert draft(**bad) == _lib.ERR_ARG and b"bad sizes" in lib.srgpt_last_error(), bad
    for K in (0, -1, 16):
        assert draft(K=K) == _lib.ERR_ARG and b"drafts outside" in lib.srgpt_last_error(), K
    for n in (0, 9):
        assert draft(max_ngram=n) == _lib.ERR_ARG and b"max_ngram" in lib.srgpt_last_error(), n

    def accept(picks=256, d=256, nd=256, B=2, T=4, tok=256, out_ids=256, pos=256, steps=256, step=256, max_new=8, max_pos=64):
        return lib.srgpt_lookup_accept_batch(picks, d, nd, B, T, tok, out_ids, pos, steps, step, max_new, max_pos, None, None, None)

    for bad in (dict(picks=None), dict(d=None), dict(nd=None), dict(tok=None), dict(out_ids=None), dict(pos=None), dict(steps=None),
                dict(step=None)):
        assert accept(**bad) == _lib.ERR_ARG and b"null pointer" in lib.srgpt_last_error(), bad
    for bad in (dict(B=0), dict(T=1), dict(T=0), dict(max_new=0), dict(max_pos=0)):
        assert accept(**bad) == _lib.ERR_ARG and b"bad sizes" in lib.srgpt_last_error(), bad
    for B, T in ((1, 17), (2, 9), (4, 5), (17, 2)):
        assert accept(B=B, T=T) == _lib.ERR_UNSUPPORTED and b"rows exceed 16" in lib.srgpt_last_error(), (B, T)


def _state_and_block(batch=2):
    from spatialrgpt_amd import _lib

    st = _lib.LlmState()
    st.batch, st.max_pos, st.max_new, st.ws_tokens = batch, 512, 16, 32
    for f in ("kcache", "vcache", "pos", "tok", "out_ids", "step", "ws", "logits"):
        setattr(st, f, 256)  # never dereferenced: every check below fails before a launch
    lk = _lib.LookupBatch()
    lk.T, lk.max_ngram, lk.prompt_ids, lk.ld_prompt, lk.n_prompt, lk.steps, lk.ws, lk.logits, lk.stats = 4, 2, 256, 7, 256, 256, 256, 256, 256
    return st, lk


def _variant(obj, **kw):
    c = type(obj)()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(obj), ctypes.sizeof(obj))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_batched_step_refuses_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    w = _weights()
    st, lk = _state_and_block()
    by = ctypes.byref
    graph = ctypes.c_void_p()
    entries = {"step": lambda w_, s_, l_: lib.srgpt_llm_lookup_step_batch(w_, s_, l_, None),
               "graph": lambda w_, s_, l_: lib.srgpt_llm_lookup_graph_create_batch(w_, s_, l_, None, by(graph))}
    for name, call in entries.items():
        assert call(by(w), by(st), ctypes.cast(None, P(_lib.LookupBatch))) == _lib.ERR_ARG, name
        assert call(ctypes.cast(None, P(_lib.LlmWeights)), by(st), by(lk)) == _lib.ERR_ARG, name
        assert call(by(w), by(_variant(st, pos=None)), by(lk)) == _lib.ERR_ARG and b"null buffers" in lib.srgpt_last_error()
        for T in (1, 0, -3):
            assert call(by(w), by(st), by(_variant(lk, T=T))) == _lib.ERR_ARG and b"rows" in lib.srgpt_last_error(), (name, T)
        for bad in (dict(ws=None), dict(logits=None), dict(stats=None), dict(steps=None), dict(n_prompt=None), dict(prompt_ids=None)):
            assert call(by(w), by(st), by(_variant(lk, **bad))) == _lib.ERR_ARG, (name, bad)
            assert b"null buffers" in lib.srgpt_last_error(), (name, bad)
        assert call(by(w), by(st), by(_variant(lk, ld_prompt=-1))) == _lib.ERR_ARG and b"ld_prompt" in lib.srgpt_last_error()
        for n in (0, 9):
            assert call(by(w), by(st), by(_variant(lk, max_ngram=n))) == _lib.ERR_ARG and b"max_ngram" in lib.srgpt_last_error()
        # greedy only
        assert call(by(w), by(_variant(st, sampling=256)), by(lk)) == _lib.ERR_UNSUPPORTED and b"greedy only" in lib.srgpt_last_error(), name
        # B * T = 17 rows (and 18, 20): one weight pass carries 16; the message names both numbers
        w1 = _weights(heads=4, kv_heads=4)  # G = 1: 16 attention columns per sequence, so only the row bound refuses
        for batch, T in ((1, 17), (17, 2), (2, 9), (5, 4)):
            assert call(by(w1), by(_variant(st, batch=batch)), by(_variant(lk, T=T))) == _lib.ERR_UNSUPPORTED, (name, batch, T)
            msg = lib.srgpt_last_error()
            assert f"batch {batch} x T={T}".encode() in msg and f"{batch * T} rows exceed the 16 rows".encode() in msg, msg
        # G = 4: five rows per sequence do not fit the attention's 16 columns, whatever the batch
        assert call(by(w), by(st), by(_variant(lk, T=5))) == _lib.ERR_UNSUPPORTED and b"columns" in lib.srgpt_last_error()
        assert call(by(w), by(_variant(st, batch=1)), by(_variant(lk, T=5))) == _lib.ERR_UNSUPPORTED and b"columns" in lib.srgpt_last_error()
    assert graph.value is None
    assert lib.srgpt_llm_lookup_graph_create_batch(by(w), by(st), by(lk), None, None) == _lib.ERR_ARG
    assert lib.srgpt_llm_lookup_sync_state_batch(by(w), by(st), ctypes.cast(None, P(_lib.LookupBatch)), None) == _lib.ERR_ARG
    assert lib.srgpt_llm_lookup_sync_state_batch(by(w), by(st), by(_variant(lk, ws=None)), None) == _lib.ERR_ARG
    assert lib.srgpt_llm_lookup_sync_state_batch(by(w), by(_variant(st, batch=5)), by(lk), None) == _lib.ERR_ARG


def test_the_batch_one_entry_points_still_refuse_two_sequences():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    w = _weights()
    st, _ = _state_and_block(batch=2)
    lk1 = _lib.Lookup()
    lk1.T, lk1.max_ngram, lk1.prompt_ids, lk1.n_prompt, lk1.ws, lk1.logits, lk1.stats = 4, 2, 256, 7, 256, 256, 256
    by = ctypes.byref
    graph = ctypes.c_void_p()
    calls = [lambda: lib.srgpt_llm_lookup_step(by(w), by(st), by(lk1), None),
             lambda: lib.srgpt_llm_lookup_step_ex(by(w), by(st), by(lk1), _lib.SAMPLER_TOPK64, None, None),
             lambda: lib.srgpt_llm_lookup_graph_create(by(w), by(st), by(lk1), None, by(graph)),
             lambda: lib.srgpt_llm_lookup_graph_create_ex(by(w), by(st), by(lk1), _lib.SAMPLER_TOPK64, None, None, by(graph))]
    for call in calls:
        assert call() == _lib.ERR_ARG and b"batch 2" in lib.srgpt_last_error()
    assert graph.value is None
