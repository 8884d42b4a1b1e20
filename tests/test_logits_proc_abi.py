"""CPU: the logits processors' C surface (srgpt_logits_proc, srgpt_logits_process, the _proc forms of the decode entry points) --
layout, exports, refusals on the host before any launch --, the generation-config resolution that feeds it, and the pin of the CPU
restatement the GPU tests compare the kernel with (tests/logits_proc_ref.py) to the installed transformers' processor classes."""
import ctypes
import os
import re

import pytest
import torch

from tests.logits_proc_ref import hf_process, hf_processors, process_ref
from tests.util import ROOT

NEW_SYMBOLS = ("srgpt_logits_process", "srgpt_llm_sample_first_proc", "srgpt_llm_decode_step_proc", "srgpt_llm_decode_graph_create_proc")


def test_block_layout_matches_the_header():
    from spatialrgpt_amd import _lib

    src = open(os.path.join(ROOT, "include", "srgpt.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} srgpt_logits_proc;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.split() for d in body.split(";") if d.strip()]
    assert [(t, n) for t, n in decls] == [("float", "repetition_penalty"), ("int", "no_repeat_ngram"), ("int", "min_new_tokens"),
                                          ("int", "n_eos"), ("int64_t", "eos[8]")]
    assert [f[0] for f in _lib.LogitsProc._fields_] == [n.split("[")[0] for _, n in decls]
    assert ctypes.sizeof(_lib.LogitsProc) == 80 and _lib.LogitsProc.eos.offset == 16 and _lib.LogitsProc.eos.size == 64
    assert _lib.LOGITS_PROC_EOS_MAX == 8


def test_symbols_are_declared_bound_and_exported():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srgpt.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.srgpt_abi_version() == _lib.ABI_VERSION == 9  # additions under ABI 9


def test_logits_process_refuses_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    ok = dict(scores=16, lp=16, ids=16, ld=48, n=3, n_dev=None, B=2, V=1000)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.srgpt_logits_process(a["scores"], a["lp"], a["ids"], a["ld"], a["n"], a["n_dev"], a["B"], a["V"], None)

    for bad in (dict(scores=None), dict(lp=None), dict(ids=None)):
        assert call(**bad) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error(), bad
    for bad in (dict(B=0), dict(B=-1), dict(V=0), dict(ld=0), dict(ld=-4)):
        assert call(**bad) == _lib.ERR_ARG and b"empty shape" in lib.srgpt_last_error(), bad
    for bad in (dict(n=-1), dict(n=49)):
        assert call(**bad) == _lib.ERR_ARG and b"history length" in lib.srgpt_last_error(), bad
    assert call(ld=_lib.LOGITS_PROC_HISTORY_MAX + 1) == _lib.ERR_UNSUPPORTED and b"exceeds" in lib.srgpt_last_error()


def test_proc_entry_points_refuse_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    P = ctypes.POINTER
    null_w, null_st = ctypes.cast(None, P(_lib.LlmWeights)), ctypes.cast(None, P(_lib.LlmState))
    g = _lib.vp()
    assert lib.srgpt_llm_sample_first_proc(null_w, null_st, 0, 16, None) == _lib.ERR_ARG
    assert lib.srgpt_llm_decode_step_proc(null_w, null_st, 0, 16, None) == _lib.ERR_ARG
    assert lib.srgpt_llm_decode_graph_create_proc(null_w, null_st, 0, 16, None, ctypes.byref(g)) == _lib.ERR_ARG
    w = _lib.LlmWeights()
    w.dtype, w.hidden, w.inter, w.layers, w.heads, w.kv_heads, w.head_dim, w.vocab = _lib.BF16, 64, 128, 1, 4, 2, 16, 32000
    st = _lib.LlmState()
    st.batch, st.max_pos, st.max_new, st.ws_tokens = 1, 8, _lib.LOGITS_PROC_HISTORY_MAX + 1, 8
    for f in ("kcache", "vcache", "pos", "tok", "out_ids", "step", "ws", "logits"):
        setattr(st, f, 256)  # never dereferenced: every check below fails before a launch
    assert lib.srgpt_llm_decode_graph_create_proc(ctypes.byref(w), ctypes.byref(st), 0, 16, None, None) == _lib.ERR_ARG  # null out
    for call in (lambda: lib.srgpt_llm_sample_first_proc(ctypes.byref(w), ctypes.byref(st), 7, 16, None),
                 lambda: lib.srgpt_llm_decode_step_proc(ctypes.byref(w), ctypes.byref(st), 7, 16, None),
                 lambda: lib.srgpt_llm_decode_graph_create_proc(ctypes.byref(w), ctypes.byref(st), 7, 16, None, ctypes.byref(g))):
        assert call() == _lib.ERR_ARG and b"sampler kind" in lib.srgpt_last_error()
    # a history (max_new ids per row) the kernel cannot hold
    for call in (lambda: lib.srgpt_llm_sample_first_proc(ctypes.byref(w), ctypes.byref(st), 0, 16, None),
                 lambda: lib.srgpt_llm_decode_step_proc(ctypes.byref(w), ctypes.byref(st), 0, 16, None),
                 lambda: lib.srgpt_llm_decode_graph_create_proc(ctypes.byref(w), ctypes.byref(st), 0, 16, None, ctypes.byref(g))):
        assert call() == _lib.ERR_UNSUPPORTED and b"logits processors" in lib.srgpt_last_error()


def test_resolve_generation_carries_the_processor_keys():
    from spatialrgpt_amd.generation import HF_DEFAULTS, NOT_GIVEN, generation_config_from_files, resolve_generation

    assert (HF_DEFAULTS["repetition_penalty"], HF_DEFAULTS["no_repeat_ngram_size"], HF_DEFAULTS["min_length"]) == (1.0, 0, 0)
    g = resolve_generation({})
    assert (g.repetition_penalty, g.no_repeat_ngram_size, g.min_length, g.min_tokens) == (1.0, 0, 0, 0) and g.logits_processors() is None
    # from a stored generation config (the keys survive the load filter) ...
    stored = generation_config_from_files({}, dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=4, eos_token_id=2,
                                                   unknown_key=1))
    assert stored == dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=4, eos_token_id=2)
    g = resolve_generation(stored, repetition_penalty=NOT_GIVEN, no_repeat_ngram_size=NOT_GIVEN, min_length=NOT_GIVEN)
    assert (g.repetition_penalty, g.no_repeat_ngram_size, g.min_length, g.min_tokens) == (1.2, 3, 4, 4)
    assert g.logits_processors() == dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=4, eos_token_ids=[2])
    # ... from keywords, which win over it; min_length and min_new_tokens count the same (generated) tokens
    g = resolve_generation(stored, repetition_penalty=1.5, no_repeat_ngram_size=2, min_new_tokens=9)
    assert (g.repetition_penalty, g.no_repeat_ngram_size, g.min_tokens) == (1.5, 2, 9)
    # an explicit None or the off value switches a stored one off
    for off in (dict(repetition_penalty=None, no_repeat_ngram_size=None, min_length=None),
                dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0)):
        g = resolve_generation(stored, **off)
        assert (g.repetition_penalty, g.no_repeat_ngram_size, g.min_length) == (1.0, 0, 0) and g.logits_processors() is None
    # a minimum length without an EOS id bans nothing: no processor
    assert resolve_generation({}, min_new_tokens=5, eos_token_id=None).logits_processors() is None
    assert resolve_generation({}, min_new_tokens=5, eos_token_id=[7, 9]).logits_processors() == dict(
        repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=5, eos_token_ids=[7, 9])
    # more EOS ids than the device block holds, together with a minimum length
    with pytest.raises(NotImplementedError):
        resolve_generation({}, min_length=2, eos_token_id=list(range(9))).logits_processors()
    assert resolve_generation({}, eos_token_id=list(range(9)), repetition_penalty=1.1).logits_processors()["eos_token_ids"] is None


@pytest.mark.parametrize("kw", [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.5), dict(repetition_penalty=2),
                                dict(repetition_penalty="1.2"), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.0),
                                dict(no_repeat_ngram_size="3")])
def test_hf_validation_errors(kw):
    from spatialrgpt_amd.generation import resolve_generation

    with pytest.raises(ValueError):
        resolve_generation({}, **kw)


def test_hf_raises_for_the_same_values():
    """the two ValueErrors are HF's own: the processor classes refuse these values when generate() builds them"""
    from transformers import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor

    for p in (0.0, -1.5, 2):
        with pytest.raises(ValueError):
            RepetitionPenaltyLogitsProcessor(penalty=p)
    for g in (-1, 2.0):
        with pytest.raises(ValueError):
            NoRepeatNGramLogitsProcessor(g)


@pytest.mark.parametrize("V", [97, 1000])
def test_restatement_equals_the_transformers_processors(V):
    """process_ref == RepetitionPenaltyLogitsProcessor -> NoRepeatNGramLogitsProcessor -> MinLength / MinNewTokensLength on random
    2-D inputs, bit for bit (fp32 on the CPU): histories with repeats, scores of both signs with zeros and -inf."""
    from transformers import MinLengthLogitsProcessor

    gen = torch.Generator().manual_seed(V)
    B = 3
    for n in (0, 1, 2, 3, 7, 20):
        ids = torch.randint(0, min(V, 12), (B, 24), generator=gen)  # a small alphabet: repeated ids and repeated n-grams
        ids[0, :n] = ids[0, 0]
        scores = torch.randn((B, V), generator=gen) * 3
        scores[:, 1] = 0.0
        scores[:, 2] = -0.0
        scores[:, 3] = float("-inf")
        for p in (1.0, 1.3, 0.8):
            for g in (0, 1, 2, 3):
                for mn, eos in ((0, ()), (n + 1, (5,)), (n, (5,)), (n + 3, (4, 0))):
                    want = hf_process(hf_processors(p, g, mn, eos), ids[:, :n], scores)
                    got = process_ref(scores, ids, n, p, g, mn, eos)
                    assert torch.equal(got, want), (n, p, g, mn, eos)
                    assert torch.equal(torch.signbit(got), torch.signbit(want))
        # MinLengthLogitsProcessor counts input_ids, which hold generated tokens only: the same rule
        want = MinLengthLogitsProcessor(n + 1, [5])(ids[:, :n], scores.clone())
        assert torch.equal(process_ref(scores, ids, n, min_new_tokens=n + 1, eos=(5,)), want)
        want = MinLengthLogitsProcessor(max(n, 1), [5])(ids[:, :max(n, 1)], scores.clone())
        assert torch.equal(process_ref(scores, ids, max(n, 1), min_new_tokens=max(n, 1), eos=(5,)), want)
