"""GPU: HF's logits processors on the device (csrc/logits_proc.hip) -- the kernel against its CPU restatement bit for bit, its
output through both samplers, and generate(repetition_penalty / no_repeat_ngram_size / min_new_tokens) against a host loop that
applies the installed transformers' processors to the logits of the existing decode path."""
import functools

import pytest
import torch

from tests.logits_proc_ref import hf_process, hf_processors, process_ref
from tests.util import load_tiny

pytestmark = pytest.mark.gpu
DEV = "cuda"
LD = 48
NEG = float("-inf")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------------------
# the kernel against the CPU restatement
# ------------------------------------------------------------------------------------------------------------------------------
def _history(B, V, seed):
    """ids int64 [B, LD] over a six-id alphabet (repeated ids, repeated n-grams) that holds ids 0 and V - 1, a different walk per
    row, and one id outside [0, V) per row"""
    g = torch.Generator().manual_seed(seed)
    alphabet = torch.tensor([0, V - 1, 17, 64, 255, 256])
    ids = alphabet[torch.randint(0, 6, (B, LD), generator=g)]
    ids[:, 2] = ids[:, 0]          # a duplicate inside every history of 3+ ids
    ids[0, 5] = V + 5
    if B > 1:
        ids[1, 9] = -3
        ids[2, 30] = 2 ** 33 + 17  # beyond 32 bits: must not alias id 17
    return ids


def _scores(B, V, seed):
    g = torch.Generator().manual_seed(seed + 1)
    s = torch.randn((B, V), generator=g) * 3
    s[:, 0], s[:, V - 1] = -2.5, 3.25     # negative and positive entries the histories meet
    s[:, 17], s[:, 64], s[:, 255] = 0.0, -0.0, NEG
    return s


@pytest.mark.parametrize("B,V", [(1, 1000), (3, 1000), (1, 32003), (3, 32003)])
def test_kernel_equals_the_cpu_restatement_bit_for_bit(B, V):
    """Every setting of the block x every history length at which the code can change its mind (0, 1, g - 2, g - 1, g for
    g = 1 .. 3, 37, and 48 = ld), the count given on the host and on the device in turn.  The whole [B, V] result is compared as
    bits (so -0.0 / +0.0 count), which covers what must NOT change too: entries no history id or EOS id names keep the bits of the
    input -- rows do not leak into each other."""
    from spatialrgpt_amd import ops

    ids, scores = _history(B, V, seed=V + B), _scores(B, V, seed=V + B)
    assert not bool(torch.isnan(scores).any())
    ids_d, scores_d = ids.to(DEV), scores.to(DEV)
    params = ops.LogitsProcParams(DEV)
    n_dev = torch.zeros((1,), dtype=torch.int32, device=DEV)
    e1, e2 = 3, V - 2  # EOS ids outside the alphabet: a ban there is the minimum length's alone
    case = 0
    for n in (0, 1, 2, 3, 37, LD):
        for g in (0, 1, 2, 3):
            for p in (1.3, 0.8):
                for mn, eos in ((0, ()), (n + 1, (e1,)), (n, (e1,)), (n + 1, (e1, e2))):
                    params.set(p, g, mn, list(eos))
                    got = scores_d.clone()
                    if case % 2:
                        n_dev.fill_(n)
                        ops.logits_process(got, params, ids_d, n_dev)
                    else:
                        ops.logits_process(got, params, ids_d, n)
                    case += 1
                    want = process_ref(scores, ids, n, p, g, mn, eos)
                    assert torch.equal(_bits(got), _bits(want)), (n, g, p, mn, eos, case % 2)
                    touched = torch.zeros((B, V), dtype=torch.bool)
                    for b in range(B):
                        for t in ids[b, :n].tolist() + list(eos):
                            if 0 <= t < V:
                                touched[b, t] = True
                    assert torch.equal(_bits(got)[~touched], _bits(scores)[~touched])
                    assert not bool(torch.isnan(got).any())
    # a device count beyond ld is clamped to ld
    params.set(1.3, 2, 0, None)
    n_dev.fill_(LD + 1000)
    got = ops.logits_process(scores_d.clone(), params, ids_d, n_dev)
    assert torch.equal(_bits(got), _bits(process_ref(scores, ids, LD, 1.3, 2)))
    # the ban of the minimum length on an id the history also penalises: the ban wins
    params.set(1.3, 0, 38, [0, V - 1])
    got = ops.logits_process(scores_d.clone(), params, ids_d, 37)
    assert torch.equal(_bits(got), _bits(process_ref(scores, ids, 37, 1.3, 0, 38, (0, V - 1)))) and bool((got[:, 0] == NEG).all())
    # an all-off block leaves every bit alone, whatever the history
    params.set(1.0, 0, 0, None)
    for n in (0, 37, LD):
        assert torch.equal(_bits(ops.logits_process(scores_d.clone(), params, ids_d, n)), _bits(scores))


# ------------------------------------------------------------------------------------------------------------------------------
# into the samplers
# ------------------------------------------------------------------------------------------------------------------------------
def test_a_banned_eos_is_never_drawn_by_either_sampler():
    """One EOS id 50 above the rest: unprocessed it is drawn with probability 1 - 999 e^-50 > 1 - 1e-18.  (The rest is flat up to a
    1e-3 ramp: an exactly flat rest is a 999-way tie at the top-k threshold, which the top-k-64 sampler reports as an error by
    design.)  With the minimum length on, 64 draws of each sampler never return it, the kept-set hooks do not list it, nothing is
    NaN and no error bit is raised."""
    from spatialrgpt_amd import ops

    B, V, EOS = 2, 1000, 437
    raw = (-1e-3 * torch.arange(V, dtype=torch.float32) / V).repeat(B, 1)
    raw[:, EOS] = 50.0
    raw = raw.to(DEV)
    ids = torch.zeros((B, LD), dtype=torch.int64, device=DEV)
    # unprocessed: the EOS id is what both samplers draw
    sp = ops.SamplingParams(DEV, B, keep_kept_sets=True).set(1.0, 50, None, seed=3)
    assert ops.sample(raw, sp, check=True).tolist() == [EOS] * B
    assert ops.sample_full(raw, ops.SamplingParams(DEV, B).set(1.0, 0, 0.9, seed=3)).tolist() == [EOS] * B
    params = ops.LogitsProcParams(DEV).set(1.0, 0, 3, [EOS])
    scores = ops.logits_process(raw.clone(), params, ids, 2)
    assert bool((scores[:, EOS] == NEG).all()) and not bool(torch.isnan(scores).any())
    spf = ops.SamplingParams(DEV, B).set(1.0, 0, 0.9, seed=5)
    for _ in range(64):
        tok = ops.sample(scores, sp, check=True)
        kept = sp.kept.cpu()
        for b in range(B):
            n = int(kept[b, 0])
            assert 1 <= n <= 50 and EOS not in kept[b, 1:1 + n].tolist() and int(tok[b]) in kept[b, 1:1 + n].tolist()
        tok_f, mask = ops.sample_full(scores, spf, kept_mask=True)
        assert not bool(mask[:, EOS].any()) and bool(mask.gather(1, tok_f[:, None]).all())
        assert EOS not in tok.tolist() + tok_f.tolist()
    # at the minimum length the ban is gone
    assert torch.equal(ops.logits_process(raw.clone(), params, ids, 3), raw)


# ------------------------------------------------------------------------------------------------------------------------------
# the decode step: generate() against a host loop over the existing path with the transformers processors on the CPU
# ------------------------------------------------------------------------------------------------------------------------------
G = 24
SETTINGS = (dict(repetition_penalty=1.5), dict(no_repeat_ngram_size=2), dict(repetition_penalty=1.5, no_repeat_ngram_size=2))


@functools.lru_cache(maxsize=None)
def _tiny(name):
    """the tiny golden model the pipeline tests load, and the embeddings of its golden prompt (T = 210 rows) as a batch of one and as
    a ragged batch of three (the prompt cut by 0 / 7 / 20 rows, right-padded)"""
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.model import LlavaLlamaModel

    cfgd, dtype, w, inp, _ = load_tiny(name)
    model = LlavaLlamaModel(SrgptConfig.from_dict(cfgd), dict(w), device=DEV, dtype=dtype, rope_positions=1024)
    emb = model.engine.prepare_inputs(inp["input_ids"].to(DEV), inp["images"].to(DEV), inp["depths"].to(DEV),
                                      [m.to(DEV) for m in inp["masks"]])[0]
    T = emb.shape[1]
    emb3 = emb.repeat(3, 1, 1)
    am3 = torch.ones((3, T), dtype=torch.int64, device=DEV)
    for b, cut in enumerate((0, 7, 20)):
        am3[b, T - cut:] = 0
        emb3[b, T - cut:] = 0
    return model, {1: (emb, torch.ones((1, T), dtype=torch.int64, device=DEV)), 3: (emb3, am3)}


def _generate(model, batch, **kw):
    emb, am = batch
    kw.setdefault("eos_token_id", None)
    if kw["eos_token_id"]:
        kw.setdefault("pad_token_id", kw["eos_token_id"][0])  # what the reference loop pads finished rows with
    return model.llm.generate(inputs_embeds=emb, attention_mask=am, do_sample=False, max_new_tokens=G, **kw).cpu()


@functools.lru_cache(maxsize=None)
def _reference(name, B, key):
    """The reference: forward(use_cache=True) + engine.step -- the existing path, unchanged by the processors -- for the logits, the
    transformers processors on the CPU, argmax; with EOS ids HF's loop (a finished row is padded, the loop ends when every row is).
    key: the processor settings as a sorted tuple of items (+ "eos").  -> int64 [B, <= G] on the CPU."""
    model, batches = _tiny(name)
    emb, am = batches[B]
    kw = dict(key)
    eos = kw.pop("eos", None)
    procs = hf_processors(kw.get("repetition_penalty", 1.0), kw.get("no_repeat_ngram_size", 0), kw.get("min_new_tokens", 0), eos or ())
    st = model(inputs_embeds=emb, attention_mask=am, use_cache=True).past_key_values
    logits = st.logits.clone()
    ids = torch.zeros((B, 0), dtype=torch.int64)
    done = torch.zeros((B,), dtype=torch.bool)
    for t in range(G):
        tok = hf_process(procs, ids, logits).argmax(-1)
        nxt = torch.where(done, torch.full_like(tok, eos[0]), tok) if eos else tok
        ids = torch.cat((ids, nxt[:, None]), 1)
        if eos:
            done |= (nxt[:, None] == torch.tensor(eos)[None, :]).any(-1)
            if bool(done.all()):
                break
        if t + 1 < G:
            logits = model.engine.step(st, tok[:, None].to(DEV))  # (rows are independent: a finished row's token does not matter)
    return ids


def _key(**kw):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items()))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", ["tiny_fp32.npz", "tiny_bf16.npz"])
def test_generate_equals_the_host_loop_with_the_transformers_processors(name, B):
    """The prompt is the golden prompt of the tiny models (and its first 203 / 190 rows in the ragged batch): on the CPU oracle its
    plain greedy continuation falls into the cycle 124, 110, 45 after one or two tokens in both dtypes, so a repetition penalty of
    1.5 changes the ids from the fifth or sixth token on and no_repeat_ngram_size = 2 from the sixth or seventh -- asserted below on
    the reference loop, so the test fails without the feature.  The reference loop runs the same decode kernels: ids must be EQUAL,
    with the captured step and the eager one, and in any order of requests on the pooled state (a stale parameter block or a stale
    graph would show)."""
    model, batches = _tiny(name)
    plain = _generate(model, batches[B])
    refs = [_reference(name, B, _key(**kw)) for kw in SETTINGS]
    for kw, ref in zip(SETTINGS, refs):
        assert ref.shape == (B, G) and not torch.equal(ref, plain), kw
        assert all(not torch.equal(ref[b], plain[b]) for b in range(B)), kw  # every row shows it
    assert not torch.equal(refs[0], refs[1])
    try:
        for use_graph in (True, False):
            model.engine.use_graph = use_graph
            for i in (0, 1, 2, 0, 0):  # every setting, then the first one twice more on the same pooled state
                got = _generate(model, batches[B], **SETTINGS[i])
                assert torch.equal(got, refs[i]), (use_graph, SETTINGS[i], got, refs[i])
            assert torch.equal(_generate(model, batches[B]), plain)  # and a plain request in between is a plain request
    finally:
        model.engine.use_graph = True


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", ["tiny_fp32.npz", "tiny_bf16.npz"])
def test_min_new_tokens_keeps_the_eos_ids_out(name, B):
    """The first id of every row's plain greedy run as EOS: without the feature the request stops after one token.  With
    min_new_tokens = 5 no EOS id appears among the first 5 tokens of any row and the whole output equals the reference loop's
    (HF's padding of finished rows included); min_length means the same, and a minimum at max_new_tokens lets nothing stop."""
    model, batches = _tiny(name)
    plain = _generate(model, batches[B])
    eos = sorted(set(plain[:, 0].tolist()))
    stop = _generate(model, batches[B], eos_token_id=eos)
    assert stop.shape == (B, 1)  # the existing behaviour without a minimum
    ref = _reference(name, B, _key(min_new_tokens=5, eos=eos))
    for kw in (dict(min_new_tokens=5), dict(min_length=5), dict(min_new_tokens=5, min_length=2)):
        got = _generate(model, batches[B], eos_token_id=eos, **kw)
        assert got.shape[1] >= 5 and not any(t in eos for t in got[:, :5].flatten().tolist())
        assert torch.equal(got, ref), (kw, got, ref)
    model.engine.use_graph = False
    try:
        assert torch.equal(_generate(model, batches[B], eos_token_id=eos, min_new_tokens=5), ref)
    finally:
        model.engine.use_graph = True
    full = _generate(model, batches[B], eos_token_id=eos, min_new_tokens=G)
    assert torch.equal(full, _reference(name, B, _key(min_new_tokens=G, eos=eos))) and full.shape == (B, G)
    assert not any(t in eos for t in full.flatten().tolist())


def test_off_values_take_the_existing_path():
    """All three keywords at their off values (or None): the bits of a request without them, and no "+proc" graph is captured."""
    model, batches = _tiny("tiny_fp32.npz")
    model.engine._state = None  # a fresh pooled state: whatever ran before on this model left no graph behind
    plain = _generate(model, batches[3])
    off = _generate(model, batches[3], repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, min_new_tokens=0)
    none = _generate(model, batches[3], repetition_penalty=None, no_repeat_ngram_size=None, min_length=None)
    no_eos = _generate(model, batches[3], min_new_tokens=5)  # a minimum length without an EOS id bans nothing
    assert torch.equal(off, plain) and torch.equal(none, plain) and torch.equal(no_eos, plain)
    graphs = model.engine._state.graphs
    assert "greedy" in graphs and not any(k.endswith("+proc") for k in graphs), list(graphs)
    _generate(model, batches[3], repetition_penalty=1.5)
    assert "greedy+proc" in model.engine._state.graphs


def test_beam_search_applies_the_processors_to_the_log_softmax_scores():
    """generate(num_beams=3, repetition_penalty=1.5) == generation.beam_generate driven by the transformers processor on the CPU
    over the same per-step logits (the processors see log_softmax scores and each beam's generated ids, HF 4.37.2's order)."""
    from spatialrgpt_amd import ops
    from spatialrgpt_amd.generation import beam_generate

    model, batches = _tiny("tiny_fp32.npz")
    emb, am = batches[1]
    NB, N = 3, 10
    eng = model.engine
    kw = dict(inputs_embeds=emb, attention_mask=am, do_sample=False, num_beams=NB, max_new_tokens=N, eos_token_id=None, pad_token_id=0)
    plain = model.llm.generate(**kw).cpu()
    st, _, _ = eng.prefill(emb.repeat_interleave(NB, dim=0), max_new=N, fresh_state=True)
    ident = torch.arange(NB, device=DEV)

    def step(tokens, beam_idx):
        if not torch.equal(beam_idx, ident):
            assert ops.kv_beam_reorder(st.kcache, st.vcache, beam_idx, NB, max(st.host_len))
        return eng.step(st, tokens[:, None])

    procs = hf_processors(repetition_penalty=1.5)

    def on_cpu(seqs, scores):
        ids = torch.tensor(seqs, dtype=torch.int64).reshape(len(seqs), len(seqs[0]))
        return hf_process(procs, ids, scores).to(scores.device)

    want = beam_generate(st.logits.clone(), step, 1, NB, N, None, 0, logits_processor=on_cpu).cpu()
    got = model.llm.generate(repetition_penalty=1.5, **kw).cpu()
    assert torch.equal(got, want), (got, want)
    assert not torch.equal(want, plain)  # the penalty changes the beam result on this prompt
    assert torch.equal(model.llm.generate(**kw).cpu(), plain)
