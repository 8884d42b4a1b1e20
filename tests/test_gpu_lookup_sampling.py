"""Prompt-lookup decoding under SAMPLING on the GPU (srgpt_llm_lookup_step_ex with st->sampling set, engine.greedy_decode(lookup=,
sampling=), generate(do_sample=True, prompt_lookup_num_tokens=K) with model.lookup_sampling on).

The contract is the per-row draw: a sampled lookup step equals, bit for bit, its composition from the per-op entries on the step's
own logits -- the drafts (ops.lookup_draft), the T draws at counter c0 + step (ops.sample_rows / ops.sample_full_rows) and the accept
rule restated in Python.  Lookup ids equal to the plain sampled loop's at a high temperature is deliberately NOT asserted: one-row
and T-row products take different kernels, their logits differ in the last bits.  End to end the request is therefore checked at
near-deterministic settings (the demo's temperature 0.2, top-k 50, on PEAKED weights: the mass outside the top-1 token is asserted
below 1e-6 on the CPU oracle's logits), where every draw is its row's argmax whatever the seed, against the oracle's greedy ids.

Geometry, weights, prompts and the oracle's ids are tests/test_gpu_lookup.py's (hidden 512, 2 layers, head_dim 128, G = 4: T = 4 rows
per step, its 3002-id vocabulary), shared through that module's caches."""
import ctypes as C
import functools

import pytest
import torch

from tests import test_gpu_lookup as tl

pytestmark = pytest.mark.gpu
DEV = tl.DEV
K, V, SENT = tl.K, tl.V, tl.SENT
T = K + 1
COUNTER_AT = 24  # byte offset of srgpt_sampling::counter
DEMO = dict(do_sample=True, temperature=0.2, top_k=50)  # the demo's settings (top_k: the transformers default)
# The composition test needs draws that really leave the argmax.  On the peaked bundle the top-1 logit stands about 19 above the
# 2nd .. 20th (the lm_head row of perm[last] is the unit vector of its embedding), so at a temperature about 1 the mass outside the
# top-1 token is ~1e-7: no draw would ever differ and the test's premise could not hold.  At 5.0 the top-1 token keeps ~0.7 of the
# top-20 mass: most draws follow the walk (drafts are accepted), some do not (drafts are rejected, ids off the argmax are emitted).
COMPOSE_TEMPERATURE, COMPOSE_TOP_K = 5.0, 20
COMPOSE_SEED = 7  # chosen among 0 .. 9: all four runs (two weight formats x two samplers) meet the premise and draft in 2+ steps


def _counter(st):
    return st.sampling.buf[COUNTER_AT:COUNTER_AT + 8].clone().view(torch.int64)


def _sampled_state(eng, prompt, max_new, sampling, guard=False):
    """a fresh batch-1 state: the prompt prefilled, the sampling block set, the first token DRAWN (srgpt_llm_sample_first_ex)"""
    from spatialrgpt_amd import _lib as L, ops

    st = eng.new_state(1, 256, max_new, ws_tokens=len(prompt))
    big = None
    if guard:  # out_ids between two sentinel rows
        big = torch.full((3, max_new), SENT, dtype=torch.int64, device=DEV)
        st.out_ids = big[1:2]
        st.c.out_ids = st.out_ids.data_ptr()
    eng.prefill(eng.embed_tokens(torch.tensor([list(prompt)], device=DEV)), max_new=max_new, state=st)
    st.set_sampling(sampling)
    L.check(L.load().srgpt_llm_sample_first_ex(C.byref(eng.w.llm), C.byref(st.c), st.sampler, ops._stream()))
    torch.cuda.synchronize()
    return st, big


def _step(eng, st, lk, graph=None):
    from spatialrgpt_amd import _lib as L, ops

    with torch.cuda.stream(eng.stream):
        eng.stream.wait_stream(torch.cuda.default_stream())
        if graph is None:
            L.check(L.load().srgpt_llm_lookup_step_ex(C.byref(eng.w.llm), C.byref(st.c), C.byref(lk["c"]), st.sampler, st.lookup_sample_ws(),
                                                      ops._stream()))
        else:
            L.check(L.load().srgpt_graph_launch(graph, 1, ops._stream()))
    eng.stream.synchronize()


def run_composition(fmt, kind, seed, steps=6, max_new=32):
    """six eager sampled lookup steps, each compared with its composition on the step's own logits; -> (drafted, accepted, emitted ids
    that are not their row's argmax)"""
    from spatialrgpt_amd import _lib as L, ops

    eng = tl._model(fmt).engine
    prompt = list(tl._prompt_full())
    sampling = dict(temperature=COMPOSE_TEMPERATURE, top_k=COMPOSE_TOP_K, top_p=1.0, seed=seed, sampler=kind)
    st, _ = _sampled_state(eng, prompt, max_new, sampling)
    lk = st.ensure_lookup(K, 2, torch.tensor(prompt, dtype=torch.int64))
    assert int(_counter(st)) == 1 and int(st.step) == 1  # c0 = 0: the first token was drawn at counter 0
    off_argmax = 0
    for rnd in range(steps):
        tok, out_ids, pos, step, stats, ctr = st.tok.clone(), st.out_ids.clone(), st.pos.clone(), st.step.clone(), lk["stats"].clone(), _counter(st)
        assert int(ctr) == int(step)  # generated id i is drawn at counter c0 + i
        _step(eng, st, lk)
        what = f"{fmt} sampler {kind} seed {seed} step {rnd}"
        # ---- the composition, on the bits the step left in lk->logits
        logits = lk["logits"].clone()
        draft, nd = ops.lookup_draft(lk["prompt"], out_ids[0], step, K, 2, V)
        ref = ops.SamplingParams(DEV, T).set(COMPOSE_TEMPERATURE, COMPOSE_TOP_K, 1.0, seed=seed, counter=int(ctr))
        draws = (ops.sample_full_rows(logits, ref) if kind == L.SAMPLER_FULL else ops.sample_rows(logits, ref, check=True)).tolist()
        d, s, P = draft.tolist(), int(step), int(pos)
        n = min(int(nd), T - 1, max(st.max_pos - 1 - P, 0))
        acc = 0
        while acc < n and d[acc] == draws[acc]:
            acc += 1
        emitted = min(acc + 1, max_new - s)
        out_ids[0, s:s + emitted] = torch.tensor(draws[:emitted], device=DEV)
        stats += torch.tensor([1, n, acc], dtype=torch.int32, device=DEV)
        assert st.tok.tolist() == [draws[emitted - 1]], what
        assert torch.equal(st.out_ids, out_ids), (what, st.out_ids.tolist(), out_ids.tolist())
        assert int(st.pos) == P + emitted and int(st.step) == s + emitted, what
        assert torch.equal(lk["stats"], stats), (what, lk["stats"].tolist(), stats.tolist())
        assert int(_counter(st)) == int(ctr) + emitted, what
        top = logits.argmax(dim=-1).tolist()
        off_argmax += sum(draws[i] != top[i] for i in range(emitted))
    assert L.load().srgpt_llm_lookup_sync_state(C.byref(eng.w.llm), C.byref(st.c), C.byref(lk["c"]), ops._stream()) == 0, L.last_error()
    _, drafted, accepted = lk["stats"].tolist()
    return drafted, accepted, off_argmax


@pytest.mark.parametrize("kind", [0, 1], ids=["topk64", "full"])
@pytest.mark.parametrize("fmt", ["native", "fp8"])
def test_sampled_step_equals_composition_bit_for_bit(fmt, kind):
    """tok, out_ids, pos, step, the stats and the device counter after each of six steps == drafts + T draws at counter c0 + step +
    the accept rule, recomputed on the step's own logits.  Premise: the run accepts some drafts and rejects some, and emits at least
    one id that is not its row's argmax -- the draws are real draws"""
    drafted, accepted, off_argmax = run_composition(fmt, kind, COMPOSE_SEED)
    assert 0 < accepted < drafted, (drafted, accepted)
    assert off_argmax >= 1


def test_captured_step_equals_eager_step():
    """the same request stepped six times eagerly and as six replays of its captured graph: every buffer the step writes is equal"""
    from spatialrgpt_amd import _lib as L

    eng = tl._model("native").engine
    prompt = list(tl._prompt_full())
    sampling = dict(temperature=COMPOSE_TEMPERATURE, top_k=COMPOSE_TOP_K, top_p=1.0, seed=COMPOSE_SEED, sampler=L.SAMPLER_TOPK64)
    res = []
    for captured in (False, True):
        st, _ = _sampled_state(eng, prompt, 32, sampling)
        lk = st.ensure_lookup(K, 2, torch.tensor(prompt, dtype=torch.int64))
        graph = None
        if captured:
            with torch.cuda.stream(eng.stream):  # a capture needs a stream of its own
                eng.stream.wait_stream(torch.cuda.default_stream())
                graph = st.ensure_lookup_graph()
        for _ in range(6):
            _step(eng, st, lk, graph)
        res.append((st.tok.clone(), st.out_ids.clone(), st.pos.clone(), st.step.clone(), lk["stats"].clone(), _counter(st),
                    lk["logits"].clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b), (a, b)
    assert int(res[0][3]) > 6  # some step emitted more than one id


def test_rejected_drafts_do_not_perturb_row_zero_under_sampling():
    """the same state and seed stepped with no history match and with planted wrong drafts: row 0's logits, the emitted token and the
    counter are equal -- one id is emitted, so the counter is c0 + 1 (c0: the counter the step found)"""
    from spatialrgpt_amd import _lib as L

    eng = tl._model().engine
    prompt = tl._chain(tl.A0, 4)[:4]
    sampling = dict(temperature=1.0, top_k=20, top_p=1.0, seed=1234, sampler=L.SAMPLER_TOPK64)
    res = []
    for planted in (False, True):
        st, _ = _sampled_state(eng, prompt, 8, sampling)
        first, c0 = int(st.tok), int(_counter(st))
        hist = torch.tensor([first, 1500, 1501, 1502] if planted else [], dtype=torch.int64)
        assert 1500 != int(tl._bundle()["perm"][first])
        lk = st.ensure_lookup(K, 2, hist if planted else None)
        _step(eng, st, lk)
        res.append(dict(logits=lk["logits"][0].clone(), tok=int(st.tok), step=int(st.step), pos=int(st.pos), stats=lk["stats"].tolist(),
                        out=st.out_ids[0, :2].tolist(), first=first, c0=c0, counter=int(_counter(st))))
    assert res[0]["stats"] == [1, 0, 0] and res[1]["stats"] == [1, 3, 0]
    assert torch.equal(res[0]["logits"], res[1]["logits"])
    for key in ("first", "c0", "tok", "step", "pos", "out", "counter"):
        assert res[0][key] == res[1][key], key
    assert res[0]["step"] == 2 and res[0]["counter"] == res[0]["c0"] + 1


# ------------------------------------------------------------------------------------------------ end to end, near-deterministic
@functools.lru_cache(maxsize=None)
def _oracle_outside_top1(prompt, n, temperature, top_k):
    """the CPU oracle's plain loop over the prompt (bf16 values, as tl._oracle_ids): at every step the mass of softmax(top-k(logits /
    temperature)) outside its top-1 token -> the largest of the n steps"""
    b = tl._bundle()
    so, ocfg, w = b["so"], b["ocfg"], b["w_cpu"]
    emb = torch.nn.functional.embedding(torch.tensor([list(prompt)]), w["llm.model.embed_tokens.weight"]).to(tl.BF16)
    kv = so.KVCache(ocfg.layers)
    lg = so.llama_forward(w, ocfg, emb, torch.arange(len(prompt))[None], kv, last_only=True)[:, -1]
    worst = 0.0
    for t in range(n):
        p = (lg[0].double() / temperature).topk(top_k).values.softmax(dim=-1)
        worst = max(worst, float(1.0 - p[0]))
        e = torch.nn.functional.embedding(torch.tensor([[int(lg[0].argmax())]]), w["llm.model.embed_tokens.weight"]).to(tl.BF16)
        lg = so.llama_forward(w, ocfg, e, torch.tensor([[len(prompt) + t]]), kv, last_only=True)[:, -1]
    return worst


@pytest.fixture
def model_on():
    """the shared peaked model with the lookup_sampling switch on for one test"""
    m = tl._model()
    m.lookup_sampling = True
    try:
        yield m
    finally:
        m.lookup_sampling = False


@pytest.mark.parametrize("which,stats", [("full", (3, 9, 9)), ("zero", (11, 33, 0))])
def test_near_deterministic_request_walks_the_oracles_ids(model_on, which, stats):
    """the demo's temperature 0.2 and top-k 50 on the peaked prompts: the oracle's greedy ids, in lookup steps, with the greedy tests'
    step counts; the same ids with the switch off"""
    prompt, n = (tl._prompt_full() if which == "full" else tl._prompt_zero()), 12
    want = tl._oracle_ids(prompt, tl.N_ORACLE)
    # on the CPU, before the engine runs: 0.2 is low enough on this bundle (no lower temperature is needed)
    assert _oracle_outside_top1(prompt, tl.N_ORACLE, DEMO["temperature"], DEMO["top_k"]) < 1e-6
    assert tl.simulate(prompt, want, K, n) == stats
    torch.manual_seed(3)
    out = tl._gen(model_on, prompt, max_new_tokens=n, prompt_lookup_num_tokens=K, **DEMO)
    ll = dict(model_on.last_lookup)
    assert out.cpu().tolist() == [want[:n]]
    assert ll["mode"] == "lookup" and ll["tokens"] == n and (ll["steps"], ll["drafted"], ll["accepted"]) == stats, ll
    assert sorted(ll) == ["accepted", "drafted", "mode", "reason", "steps", "tokens"]
    model_on.lookup_sampling = False
    torch.manual_seed(3)
    off = tl._gen(model_on, prompt, max_new_tokens=n, prompt_lookup_num_tokens=K, **DEMO)
    assert model_on.last_lookup["mode"] == "plain" and torch.equal(out, off)


def test_eos_and_stopping_criteria_cut_where_the_plain_sampled_loop_cuts(model_on):
    """ids 1 | 2 3 4 5 | 6 7 8 9 | ...: id 7 is the first accepted draft of its step, id 8 the second"""
    prompt, n = tl._prompt_full(), 12
    want = tl._oracle_ids(prompt, tl.N_ORACLE)
    assert _oracle_outside_top1(prompt, tl.N_ORACLE, DEMO["temperature"], DEMO["top_k"]) < 1e-6
    crit = [lambda ids, scores: int(ids[0, -1]) == want[7]]
    cases = [(dict(eos_token_id=want[6]), want[:7]), (dict(eos_token_id=[want[9], want[4]], pad_token_id=3), want[:5]),
             (dict(eos_token_id=[want[0]]), want[:1]), (dict(stopping_criteria=crit), want[:8])]
    for kw, kept in cases:
        plain = tl._gen(model_on, prompt, max_new_tokens=n, **DEMO, **kw)
        assert model_on.last_lookup["mode"] == "plain"
        out = tl._gen(model_on, prompt, max_new_tokens=n, prompt_lookup_num_tokens=K, **DEMO, **kw)
        assert model_on.last_lookup["mode"] == "lookup" and model_on.last_lookup["tokens"] == len(kept), (kw, model_on.last_lookup)
        assert torch.equal(out, plain) and out.cpu().tolist() == [kept], (kw, out, plain)


def test_max_new_tokens_inside_an_emission_under_sampling():
    """10 ids = 1 + 4 + 4 + the first of a step that would emit 4: exactly 10 come back, as from the plain sampled loop, and out_ids --
    10 long, between two sentinel rows -- is not overrun however many steps run ahead"""
    from spatialrgpt_amd import _lib as L

    prompt, n = tl._prompt_full(), 10
    want = tl._oracle_ids(prompt, tl.N_ORACLE)
    assert _oracle_outside_top1(prompt, tl.N_ORACLE, DEMO["temperature"], DEMO["top_k"]) < 1e-6
    eng = tl._model().engine
    sampling = dict(temperature=DEMO["temperature"], top_k=DEMO["top_k"], top_p=1.0, seed=77, sampler=L.SAMPLER_TOPK64)
    st, _ = tl._state_after_first_token(eng, prompt, n)
    plain = eng.greedy_decode(st, n, sampling=dict(sampling))
    st, big = tl._state_after_first_token(eng, prompt, n, guard=True)
    out = eng.greedy_decode(st, n, sampling=dict(sampling), lookup=dict(K=K, max_ngram=2, prompt_ids=torch.tensor(prompt, dtype=torch.int64)))
    torch.cuda.synchronize()
    assert out.shape == (1, n) and torch.equal(out, plain) and out.cpu().tolist() == [want[:n]]
    assert eng.last_lookup_stats["tokens"] == n and eng.last_lookup_stats["steps"] == 3
    assert bool((big[0] == SENT).all()) and bool((big[2] == SENT).all()) and big[1].tolist() == want[:n]
    assert st.c.sampling is None  # the loop leaves the state greedy, as the plain loop does
    # the counter did not move for the step that ran ahead of a full request: n ids were drawn at counters 0 .. n - 1
    assert int(_counter(st)) == n


@pytest.mark.parametrize("second", ["plain", "lookup"])
def test_returned_state_continues_under_sampling(model_on, second):
    """return_dict_in_generate=True after a sampled lookup request: the state continues with a plain sampled request and with another
    sampled lookup request to the oracle's ids over the whole conversation"""
    prompt, n1, n2 = tl._prompt_full(), 6, 7
    first = tl._oracle_ids(prompt, tl.N_ORACLE)[:n1]
    seg = (tl._chain(tl.A0, 30)[20], )
    whole = tuple(prompt) + tuple(first) + seg
    want2 = tl._oracle_ids(whole, n2)
    assert _oracle_outside_top1(prompt, tl.N_ORACLE, DEMO["temperature"], DEMO["top_k"]) < 1e-6
    assert _oracle_outside_top1(whole, n2, DEMO["temperature"], DEMO["top_k"]) < 1e-6
    r = tl._gen(model_on, prompt, max_new_tokens=n1, prompt_lookup_num_tokens=K, return_dict_in_generate=True, **DEMO)
    assert r.sequences.cpu().tolist() == [first] and model_on.last_lookup["mode"] == "lookup"
    st = r.past_key_values
    assert st.host_len == [len(prompt) + n1 - 1] and st.pending is not None
    kw = dict(prompt_lookup_num_tokens=K) if second == "lookup" else {}
    out = tl._gen(model_on, seg, max_new_tokens=n2, past_key_values=st, **DEMO, **kw)
    assert out.cpu().tolist() == [want2] and model_on.last_lookup["mode"] == second
    assert st.host_len == [len(whole) + n2 - 1]


# ------------------------------------------------------------------------------------------------ the seed
@functools.lru_cache(maxsize=None)
def _flat_model():
    """the same geometry with the synthetic weights as they come (no peaked head): logits a few tenths apart, so that at temperature
    1.0 a draw really depends on its random number"""
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.model import LlavaLlamaModel
    from spatialrgpt_amd.weights import synth_state_dict

    cfg = SrgptConfig(**tl.KW)
    return LlavaLlamaModel(cfg, synth_state_dict(cfg, seed=0, dtype=tl.BF16, device=DEV), device=DEV, dtype=tl.BF16, rope_positions=512,
                           lookup_sampling=True)


def test_requests_are_reproducible_under_the_seed():
    """temperature 1.0 (this test only: the draws must depend on the seed): under torch.manual_seed(s) two identical requests return
    identical ids, and two different seeds differ somewhere"""
    model = _flat_model()
    prompt = (5, 6, 7, 8, 9, 5, 6, 7, 8, 9, 5, 6)

    def run(seed):
        torch.manual_seed(seed)
        out = tl._gen(model, prompt, max_new_tokens=16, prompt_lookup_num_tokens=K, do_sample=True, temperature=1.0)
        assert model.last_lookup["mode"] == "lookup" and model.last_lookup["tokens"] == 16, model.last_lookup
        return out

    a, b, c = run(11), run(11), run(12)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)


def test_switch_off_names_the_switch():
    """off (the default): a sampled request with the keyword runs the plain loop and the reason says which switch would change that"""
    model = tl._model()
    assert model.lookup_sampling is False
    tl._gen(model, tl._prompt_full(), max_new_tokens=4, prompt_lookup_num_tokens=K, **DEMO)
    ll = model.last_lookup
    assert ll["mode"] == "plain" and "do_sample" in ll["reason"] and "lookup_sampling" in ll["reason"], ll
    assert (ll["steps"], ll["tokens"], ll["drafted"], ll["accepted"]) == (0, 0, 0, 0)
