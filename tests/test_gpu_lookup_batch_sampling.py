"""Prompt-lookup decoding for SAMPLED BATCHES on the GPU (srgpt_llm_lookup_step_batch_ex with st->sampling set,
engine.greedy_decode(lookup=, sampling=) on 2+ rows, generate(input_ids [B, P], do_sample=True, prompt_lookup_num_tokens=K) with
model.lookup_batch and model.lookup_batch_sampling on).

The contract is the per-row draw at the plain loop's address: a sampled batched lookup step equals, bit for bit, its composition on
the step's own logits -- the drafts (ops.lookup_draft_batch), every row's draw from the B-MODE sampler (ops.sample / ops.sample_full)
at (counter + steps[b] - m + t, sequence b), m = min steps, and the accept and counter rules restated in Python.  What these tests
cannot show: ids equal to the plain sampled batched loop's at a high temperature.  Products over B * T rows and over B rows take
different kernels and their logits differ in the last bits (tests/test_gpu_lookup_sampling.py says the same of batch 1), so that
equality is NOT asserted; the address identity (tests/test_host_draw_addr.py, tests/test_gpu_sample_seq_rows.py) and the composition
stand in for it.  End to end the request runs at near-deterministic settings (the demo's temperature 0.2 and top-k 50 on PEAKED
weights, the mass outside the top-1 token asserted below 1e-6 on the CPU oracle's logits) against the oracle's greedy ids.

Geometry, weights, prompts and the oracle's ids are tests/test_gpu_lookup.py's (2 layers, hidden 512, heads 4 / kv_heads 1, head_dim
128, vocab 3002: T = 4 is the attention's limit, (4, 4) fills the 16-row pass), the batch's prompts tests/test_gpu_lookup_batch.py's."""
import ctypes as C

import pytest
import torch

from tests import test_gpu_lookup as tl
from tests import test_gpu_lookup_batch as tb
from tests import test_gpu_lookup_sampling as tls

pytestmark = pytest.mark.gpu
DEV = tl.DEV
K, V, SENT = tl.K, tl.V, tl.SENT
T = K + 1
DEMO = tls.DEMO
COMPOSE_TEMPERATURE, COMPOSE_TOP_K = tls.COMPOSE_TEMPERATURE, tls.COMPOSE_TOP_K  # 5.0 / 20: draws that really leave the argmax
COMPOSE_SEED = 7  # chosen on the GPU among 0 .. 9 (3, 5, 6, 7 and 9 qualify): all eight runs (two weight formats x two samplers x B = 2, 4) meet the premise


def _sampled_state(eng, prompts, max_new, sampling, guard=False):
    """tests/test_gpu_lookup_batch.py's _state with the sampling block set and the first token of every row DRAWN
    (srgpt_llm_sample_first_ex: at counter 0, so the counter is 1 behind it); sampling None: the greedy state"""
    from spatialrgpt_amd import _lib as L, ops

    B, P = len(prompts), max(len(p) for p in prompts)
    st = eng.new_state(B, 256, max_new, ws_tokens=P)
    st.kcache.zero_()
    st.vcache.zero_()
    big = None
    if guard:
        big = torch.full((B + 2, max_new), SENT, dtype=torch.int64, device=DEV)
        st.out_ids = big[1:B + 1]
        st.c.out_ids = st.out_ids.data_ptr()
    ids = torch.tensor([list(p) + [0] * (P - len(p)) for p in prompts], device=DEV)
    lens = torch.tensor([len(p) for p in prompts], dtype=torch.int32, device=DEV)
    eng.prefill(eng.embed_tokens(ids), max_new=max_new, lens=None if min(len(p) for p in prompts) == P else lens, state=st)
    st.set_sampling(sampling)
    L.check(L.load().srgpt_llm_sample_first_ex(C.byref(eng.w.llm), C.byref(st.c), st.sampler, ops._stream()))
    torch.cuda.synchronize()
    mask = torch.tensor([[1] * len(p) + [0] * (P - len(p)) for p in prompts], device=DEV)
    lk = st.ensure_lookup_batch(K, 2, ids, mask)
    lk["steps"].fill_(1)
    return st, lk, big


def _step(eng, st, lk, graph=None, entry="srgpt_llm_lookup_step_batch_ex"):
    from spatialrgpt_amd import _lib as L, ops

    with torch.cuda.stream(eng.stream):
        eng.stream.wait_stream(torch.cuda.default_stream())
        if graph is not None:
            L.check(L.load().srgpt_graph_launch(graph, 1, ops._stream()))
        elif entry == "srgpt_llm_lookup_step_batch":
            L.check(L.load().srgpt_llm_lookup_step_batch(C.byref(eng.w.llm), C.byref(st.c), C.byref(lk["c"]), ops._stream()))
        else:
            L.check(L.load().srgpt_llm_lookup_step_batch_ex(C.byref(eng.w.llm), C.byref(st.c), C.byref(lk["c"]), st.sampler,
                                                           st.lookup_sample_ws(batched=True), ops._stream()))
    eng.stream.synchronize()


def _written(st, lk):
    """every buffer a step writes, and the counter"""
    return dict(tok=st.tok.clone(), out_ids=st.out_ids.clone(), pos=st.pos.clone(), step=st.step.clone(), steps=lk["steps"].clone(),
                stats=lk["stats"].clone(), logits=lk["logits"].clone(), kcache=tl._bits(st.kcache).clone(), vcache=tl._bits(st.vcache).clone(),
                **({"counter": tls._counter(st)} if st.c.sampling else {}))


def _b_mode_draws(logits, B, kind, seed, ctr, steps, m):
    """every row's draw from the B-mode sampler: row (b, t) is row b of a B-row call at counter ctr + steps[b] - m + t"""
    from spatialrgpt_amd import _lib as L, ops

    at = {}
    for b in range(B):
        for t in range(T):
            at.setdefault(ctr + steps[b] - m + t, []).append((b, t))
    draws = [None] * (B * T)
    for c, rows in sorted(at.items()):
        x = logits[:1].repeat(B, 1)  # the other rows: any row without a tie group the sampler would report
        for b, t in rows:
            x[b] = logits[b * T + t]
        ref = ops.SamplingParams(DEV, B).set(COMPOSE_TEMPERATURE, COMPOSE_TOP_K, 1.0, seed=seed, counter=c)
        ids = (ops.sample_full(x, ref) if kind == L.SAMPLER_FULL else ops.sample(x, ref, check=True)).tolist()
        for b, t in rows:
            draws[b * T + t] = ids[b]
    return draws


def run_composition(fmt, kind, B, seed, rounds=6, max_new=32):
    """six eager sampled batched lookup steps, each compared with its composition on the step's own logits; -> (drafted, accepted,
    emitted ids that are not their row's argmax, steps after which the rows' counts differed)"""
    from spatialrgpt_amd import _lib as L, ops

    eng = tl._model(fmt).engine
    prompts = tb.STEP_CASES[B]()
    sampling = dict(temperature=COMPOSE_TEMPERATURE, top_k=COMPOSE_TOP_K, top_p=1.0, seed=seed, sampler=kind)
    st, lk, big = _sampled_state(eng, prompts, max_new, sampling, guard=True)
    assert int(tls._counter(st)) == 1 and int(st.step) == 1  # c0 = 0: every row's first token was drawn at (0, b)
    off_argmax = apart = 0
    for rnd in range(rounds):
        tok, out_ids, pos, stats = st.tok.clone(), st.out_ids.clone(), st.pos.tolist(), lk["stats"].clone()
        steps, ctr = lk["steps"].tolist(), int(tls._counter(st))
        m = min(max(s, 0) for s in steps)
        assert ctr == m and int(st.step) == m  # the counter names the draw of the column every row has filled (c0 = 0)
        _step(eng, st, lk)
        what = f"{fmt} sampler {kind} B={B} seed {seed} step {rnd}"
        # ---- the composition, on the bits the step left in lk->logits
        logits = lk["logits"].clone()
        draft, nd = ops.lookup_draft_batch(lk["prompt"], lk["n_prompt"], out_ids, torch.tensor(steps, dtype=torch.int32, device=DEV), K, 2, V)
        draws = _b_mode_draws(logits, B, kind, seed, ctr, steps, m)
        top = logits.argmax(dim=-1).tolist()
        after, live, n_sum, acc_sum = list(steps), 0, 0, 0
        for b in range(B):
            s, P, d, mine = steps[b], pos[b], draft[b].tolist(), draws[b * T:(b + 1) * T]
            if s < 0 or s >= max_new:
                continue  # frozen: nothing of it is written or counted
            n = min(int(nd[b]), T - 1, max(st.max_pos - 1 - P, 0))
            acc = 0
            while acc < n and d[acc] == mine[acc]:
                acc += 1
            emitted = min(acc + 1, max_new - s)
            out_ids[b, s:s + emitted] = torch.tensor(mine[:emitted], device=DEV)
            tok[b], pos[b], after[b] = mine[emitted - 1], P + emitted, s + emitted
            live, n_sum, acc_sum = 1, n_sum + n, acc_sum + acc
            off_argmax += sum(mine[i] != top[b * T + i] for i in range(emitted))
        stats += torch.tensor([live, n_sum, acc_sum], dtype=torch.int32, device=DEV)
        m_after = min(max(s, 0) for s in after)
        assert torch.equal(st.tok, tok), (what, st.tok.tolist(), tok.tolist())
        assert torch.equal(st.out_ids, out_ids), (what, st.out_ids.tolist(), out_ids.tolist())
        assert st.pos.tolist() == pos and lk["steps"].tolist() == after and int(st.step) == min(after), what
        assert torch.equal(lk["stats"], stats), (what, lk["stats"].tolist(), stats.tolist())
        assert int(tls._counter(st)) == ctr + (m_after - m), what
        apart += len(set(after)) > 1
    assert bool((big[0] == SENT).all()) and bool((big[B + 1] == SENT).all())
    assert L.load().srgpt_llm_lookup_sync_state_batch(C.byref(eng.w.llm), C.byref(st.c), C.byref(lk["c"]), ops._stream()) == 0, L.last_error()
    _, drafted, accepted = lk["stats"].tolist()
    return drafted, accepted, off_argmax, apart


@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize("kind", [0, 1], ids=["topk64", "full"])
@pytest.mark.parametrize("fmt", ["native", "fp8"])
def test_sampled_batched_step_equals_composition_bit_for_bit(fmt, kind, B):
    """tok, out_ids (between sentinel rows), pos, steps, *step, the stats and the device counter after each of six steps == the batched
    drafts + every row's B-mode draw at (counter + steps[b] - m + t, b) + the accept and counter rules, recomputed on the step's own
    logits.  Premise: some drafts accepted and some rejected, the rows' counts differ after at least one step, and at least one
    emitted id is not its row's argmax"""
    drafted, accepted, off_argmax, apart = run_composition(fmt, kind, B, COMPOSE_SEED)
    print(f"{fmt} sampler {kind} B={B}: drafted {drafted} accepted {accepted} off the argmax {off_argmax} steps with rows apart {apart}")
    assert 0 < accepted < drafted, (drafted, accepted)
    assert apart >= 1
    assert off_argmax >= 1


def test_captured_step_equals_eager_step():
    """the same sampled batch stepped six times eagerly and as six replays of its captured graph: every buffer the step writes, and
    the counter, are equal"""
    from spatialrgpt_amd import _lib as L

    eng = tl._model("native").engine
    sampling = dict(temperature=COMPOSE_TEMPERATURE, top_k=COMPOSE_TOP_K, top_p=1.0, seed=COMPOSE_SEED, sampler=L.SAMPLER_TOPK64)
    res = []
    for captured in (False, True):
        st, lk, _ = _sampled_state(eng, tb.STEP_CASES[2](), 32, sampling)
        graph = None
        if captured:
            with torch.cuda.stream(eng.stream):  # a capture needs a stream of its own
                eng.stream.wait_stream(torch.cuda.default_stream())
                graph = st.ensure_lookup_batch_graph()
            assert "lookup_batch+sample" in st.graphs and "lookup_batch" not in st.graphs  # a graph key of its own
        for _ in range(6):
            _step(eng, st, lk, graph)
        res.append(_written(st, lk))
    for key in res[0]:
        assert torch.equal(res[0][key], res[1][key]), key
    assert int(res[0]["steps"].max()) > 7  # some step emitted more than one id


def test_one_sequence_is_the_batch_one_sampled_step():
    """from identical states srgpt_llm_lookup_step_batch_ex on one sequence and srgpt_llm_lookup_step_ex leave the same bits, the
    counter included, under both samplers"""
    from spatialrgpt_amd import _lib as L

    eng = tl._model().engine
    prompt = list(tl._prompt_full())
    for kind in (L.SAMPLER_TOPK64, L.SAMPLER_FULL):
        sampling = dict(temperature=COMPOSE_TEMPERATURE, top_k=COMPOSE_TOP_K, top_p=1.0, seed=tls.COMPOSE_SEED, sampler=kind)
        sa, _ = tls._sampled_state(eng, prompt, 32, sampling)
        la = sa.ensure_lookup(K, 2, torch.tensor(prompt, dtype=torch.int64))
        sb, lb, _ = _sampled_state(eng, [tuple(prompt)], 32, sampling)
        assert torch.equal(sa.tok, sb.tok) and int(tls._counter(sa)) == int(tls._counter(sb)) == 1
        for rnd in range(6):
            tls._step(eng, sa, la)
            _step(eng, sb, lb)
            assert torch.equal(la["logits"], lb["logits"]), (kind, rnd)
            assert torch.equal(sa.out_ids, sb.out_ids) and torch.equal(sa.pos, sb.pos) and torch.equal(sa.step, sb.step) and torch.equal(sa.tok, sb.tok)
            assert torch.equal(la["stats"], lb["stats"]) and torch.equal(lb["steps"], sb.step), (kind, rnd)
            assert int(tls._counter(sa)) == int(tls._counter(sb)) == int(sb.step), (kind, rnd)
        drafted, accepted = la["stats"].tolist()[1:]
        assert 0 < accepted < drafted  # tests/test_gpu_lookup_sampling.py's premise at its seed


@pytest.mark.parametrize("frozen", [0, 1])
def test_a_row_at_max_new_is_frozen_and_the_counter_follows_the_live_row(frozen):
    """tests/test_gpu_lookup_batch.py's frozen-row request under near-deterministic sampling: row `frozen` accepts everything and
    holds max_new = 8 ids after two steps, the other row emits one id per step.  Nothing of the frozen row is written, and the
    counter names the live row's column (c0 = 0: counter == min steps) until both are frozen, where it stays"""
    from spatialrgpt_amd import _lib as L, ops

    max_new = 8
    prompts = [tb._full(tl.A0), tb._zero(tb.A1)] if frozen == 0 else [tb._zero(tb.A1), tb._full(tl.A0)]
    live = 1 - frozen
    wants = [tl._oracle_ids(p, tl.N_ORACLE) for p in prompts]
    log, n_after = tb._replay(prompts, wants, K, max_new, 9)
    assert [row[frozen] for row in log] == [(3, 3), (3, 3)] + [None] * 7
    assert [row[live] for row in log] == [(3, 0)] * 7 + [None] * 2 and n_after == [8, 8]
    for p in prompts:  # every draw is its row's argmax whatever the seed
        assert tls._oracle_outside_top1(p, tl.N_ORACLE, DEMO["temperature"], DEMO["top_k"]) < 1e-6

    eng = tl._model().engine
    sampling = dict(temperature=DEMO["temperature"], top_k=DEMO["top_k"], top_p=1.0, seed=41, sampler=L.SAMPLER_TOPK64)
    st, lk, big = _sampled_state(eng, prompts, max_new, sampling, guard=True)
    for _ in range(2):
        _step(eng, st, lk)
    assert lk["steps"].tolist()[frozen] == max_new and lk["steps"].tolist()[live] == 3 and int(st.step) == 3
    assert int(tls._counter(st)) == 3 and lk["stats"].tolist() == [2, 12, 6]
    snap = dict(pos=int(st.pos[frozen]), tok=int(st.tok[frozen]), out=st.out_ids[frozen].tolist())
    assert snap["out"] == wants[frozen][:max_new]
    for n in range(3, 8):  # the live row goes on alone
        _step(eng, st, lk)
        assert lk["steps"].tolist()[frozen] == max_new and int(st.pos[frozen]) == snap["pos"] and int(st.tok[frozen]) == snap["tok"]
        assert st.out_ids[frozen].tolist() == snap["out"]
        assert lk["steps"].tolist()[live] == n + 1 and int(st.step) == n + 1 and int(tls._counter(st)) == n + 1
        assert lk["stats"].tolist() == [n, 6 + 3 * n, 6], n
        assert st.out_ids[live, :n + 1].tolist() == wants[live][:n + 1] and st.out_ids[live, n + 1:].tolist() == [SENT] * (max_new - n - 1)
    assert lk["steps"].tolist() == [8, 8] and int(st.step) == 8 and int(tls._counter(st)) == 8
    state = (st.pos.tolist(), st.tok.tolist(), st.out_ids.tolist(), lk["stats"].tolist(), int(tls._counter(st)))
    for _ in range(2):  # every row frozen: a step that ran ahead changes and counts nothing, the counter does not move
        _step(eng, st, lk)
    assert (st.pos.tolist(), st.tok.tolist(), st.out_ids.tolist(), lk["stats"].tolist(), int(tls._counter(st))) == state and int(st.step) == 8
    assert bool((big[0] == SENT).all()) and bool((big[3] == SENT).all())
    assert L.load().srgpt_llm_lookup_sync_state_batch(C.byref(eng.w.llm), C.byref(st.c), C.byref(lk["c"]), ops._stream()) == 0, L.last_error()


def test_without_sampling_the_ex_step_is_the_greedy_batched_step():
    """st->sampling == NULL: from identical states srgpt_llm_lookup_step_batch_ex (no sampler workspace) and
    srgpt_llm_lookup_step_batch leave the same bits"""
    eng = tl._model().engine
    prompts = tb.STEP_CASES[4]()
    sa, la, _ = _sampled_state(eng, prompts, 32, None)
    sb, lb, _ = _sampled_state(eng, prompts, 32, None)
    assert sa.c.sampling is None and sa.lookup_sample_ws() is None
    for rnd in range(4):
        _step(eng, sa, la, entry="srgpt_llm_lookup_step_batch")
        _step(eng, sb, lb)
        wa, wb = _written(sa, la), _written(sb, lb)
        for key in wa:
            assert torch.equal(wa[key], wb[key]), (rnd, key)
    assert la["stats"].tolist()[2] > 0 and len(set(la["steps"].tolist())) > 1


# ------------------------------------------------------------------------------------------------ end to end, near-deterministic
@pytest.fixture
def model_bs():
    """the shared peaked model with both batch switches on for one test (the pooled state dropped, as tests/test_gpu_lookup_batch.py's
    fixture does)"""
    model = tl._model()
    model.lookup_batch = model.lookup_batch_sampling = True
    model.engine._state = None
    try:
        yield model
    finally:
        model.lookup_batch = model.lookup_batch_sampling = False


@pytest.mark.parametrize("side", ["right", "left"])
def test_generate_with_ragged_acceptance_under_sampling(model_bs, side):
    """the demo's temperature 0.2 and top-k 50 on the peaked prompts, rows that accept fully, never and partly: every row returns the
    CPU oracle's greedy ids through batched sampled lookup steps, with the greedy batch's counts"""
    rows, n = [tl._prompt_full(), tl._prompt_zero(), tb._partial(tb.A2)], 12
    wants = [tl._oracle_ids(r, tl.N_ORACLE) for r in rows]
    sims = [tl.simulate(r, w_, K, n) for r, w_ in zip(rows, wants)]
    assert sims[0] == (3, 9, 9) and sims[1] == (n - 1, 3 * (n - 1), 0)
    assert 0 < sims[2][2] < sims[2][1] and sims[0][0] < sims[2][0] < sims[1][0], sims
    for r in rows:  # on the CPU, before the engine runs: every draw is its row's argmax whatever the seed
        assert tls._oracle_outside_top1(r, tl.N_ORACLE, DEMO["temperature"], DEMO["top_k"]) < 1e-6
    ids, mask = tb._pad(rows, side)
    kw = dict(attention_mask=mask, eos_token_id=None, max_new_tokens=n, prompt_lookup_num_tokens=K, **DEMO)
    torch.manual_seed(3)
    out = model_bs.generate(ids, **kw)
    ll = dict(model_bs.last_lookup)
    assert out.cpu().tolist() == [w_[:n] for w_ in wants]
    assert ll == dict(mode="lookup", reason="K = 3 drafts per step, batch 3, sampled", steps=max(s[0] for s in sims), tokens=3 * n,
                      drafted=sum(s[1] for s in sims), accepted=sum(s[2] for s in sims), batch=3), ll
    torch.manual_seed(3)
    again = model_bs.generate(ids, **kw)
    assert torch.equal(out, again) and model_bs.last_lookup == ll


def test_with_the_switch_off_the_request_runs_the_plain_loop(model_bs):
    rows, n = [tl._prompt_full(), tl._prompt_zero(), tb._partial(tb.A2)], 12
    ids, mask = tb._pad(rows, "right")
    kw = dict(attention_mask=mask, eos_token_id=None, max_new_tokens=n, prompt_lookup_num_tokens=K, **DEMO)
    torch.manual_seed(3)
    on = model_bs.generate(ids, **kw)
    assert model_bs.last_lookup["mode"] == "lookup"
    model_bs.lookup_batch_sampling = False
    torch.manual_seed(3)
    off = model_bs.generate(ids, **kw)
    ll = model_bs.last_lookup
    assert ll["mode"] == "plain" and ll["reason"] == ("do_sample: batch 3 draws from one Philox counter, rows that emit different "
                                                      "numbers of ids would need one each"), ll
    assert (ll["steps"], ll["tokens"], ll["drafted"], ll["accepted"]) == (0, 0, 0, 0)
    assert torch.equal(on, off)  # near-deterministic settings: both are the oracle's greedy ids
