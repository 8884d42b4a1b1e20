"""Prompt-lookup decoding for BATCHES on the GPU (srgpt_llm_lookup_step_batch, LlavaLlamaModel.lookup_batch): the per-row draft rule
against the Python restatement; the batched step, eager and as a replayed graph, bf16 and fp8 W8A16, against its composition from the
per-op entries bit for bit; one sequence through the batched step against the batch-1 step; a row frozen at max_new while the other
goes on; and generate(input_ids [B, P], prompt_lookup_num_tokens=K) end to end on the peaked weights of tests/test_gpu_lookup.py
(same geometry: 2 layers, hidden 512, heads 4 / kv_heads 1, head_dim 128, vocab 3002).

Expected ids always come from the CPU oracle's plain loop run PER ROW (_oracle_ids), never from the engine; every prompt construction
is replayed on the CPU (simulate / _replay) before the GPU is touched, and the replay asserts the premise the test rests on: which
rows accept how much in which step."""
import ctypes as C

import pytest
import torch

from tests.test_gpu_lookup import (_bundle, _chain, _model, _oracle_ids, _prompt_full, _prompt_zero, draft_ref, simulate, A0, DEV, K,
                                   N_ORACLE, SENT, V, _bits)

pytestmark = pytest.mark.gpu
A1, A2 = 29, 43  # two more starts of the walk (asserted below: their walks share no id with A0's over the ids a test generates)
T = K + 1


# ------------------------------------------------------------------------------------------------ prompts
def _full(a):
    """a, perm[a], ..., perm^12[a], a: every draft agrees with the model"""
    return tuple(_chain(a, 12) + [a])


def _zero(a):
    """every hop of the walk followed by an id the model does not pick"""
    chain = _chain(a, 12)
    perm = _bundle()["perm"]
    z = next(t for t in range(100, V) if t not in chain and all(int(perm[c]) != t for c in chain))
    out = []
    for c in chain:
        out += [c, z]
    return tuple(out + [a])


def _partial(a):
    """the walk, then a stretch whose continuation the model does not follow (tests/test_gpu_lookup.py's step test): 3 of 3, 1 of 3,
    1 of 3, then steps without a match"""
    c = _chain(a, 12)
    assert 999 not in c and 998 not in c
    return tuple(c[:6] + [c[6], 999, c[7], c[8], 998] + [a])


def _replay(prompts, wants, k, cap, n_steps, max_ngram=2):
    """the batched lookup loop replayed over the ids the model WILL pick per row: -> per step, per row (drafted, accepted) or None for
    a row frozen at `cap` ids; and the rows' counts afterwards"""
    n = [1] * len(prompts)
    log = []
    for _ in range(n_steps):
        row = []
        for b, (p, ids) in enumerate(zip(prompts, wants)):
            if n[b] >= cap:
                row.append(None)
                continue
            d = draft_ref(list(p) + list(ids[:n[b]]), k, max_ngram, V)
            acc = 0
            while acc < len(d) and d[acc] == ids[n[b] + acc]:
                acc += 1
            n[b] = min(n[b] + acc + 1, cap)
            row.append((len(d), acc))
        log.append(row)
    return log, n


def _kinds(step_row):
    """all / some / none of the drafts accepted, per live row that drafted"""
    return {("all" if a == d else "none" if a == 0 else "some") for d, a in (r for r in step_row if r is not None) if d > 0}


def _state(eng, prompts, max_new, guard=False):
    """a fresh state of len(prompts) sequences, caches zeroed (two such states hold the same bits): the ragged prompts prefilled, the
    first token of every row picked (srgpt_llm_sample_first).  guard: out_ids between two sentinel rows, itself filled with the sentinel"""
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
    L.check(L.load().srgpt_llm_sample_first(C.byref(eng.w.llm), C.byref(st.c), ops._stream()))
    mask = torch.tensor([[1] * len(p) + [0] * (P - len(p)) for p in prompts], device=DEV)
    return st, big, ids, mask


def _step(eng, st, lk, graph=None):
    from spatialrgpt_amd import _lib as L, ops

    with torch.cuda.stream(eng.stream):
        eng.stream.wait_stream(torch.cuda.default_stream())
        if graph is None:
            L.check(L.load().srgpt_llm_lookup_step_batch(C.byref(eng.w.llm), C.byref(st.c), C.byref(lk["c"]), ops._stream()))
        else:
            L.check(L.load().srgpt_graph_launch(graph, 1, ops._stream()))
    eng.stream.synchronize()


@pytest.fixture
def model_b():
    """the shared peaked model with the lookup_batch switch on for one test; the pooled state is dropped so that the request's state
    holds exactly max_new_tokens ids per row (a row is frozen at the STATE's max_new: the replayed counts assume the request's)"""
    model = _model()
    model.lookup_batch = True
    model.engine._state = None
    try:
        yield model
    finally:
        model.lookup_batch = False


def _pad(rows, side):
    P = max(len(r) for r in rows)
    ids = [list(r) + [0] * (P - len(r)) if side == "right" else [0] * (P - len(r)) + list(r) for r in rows]
    mask = [[1] * len(r) + [0] * (P - len(r)) if side == "right" else [0] * (P - len(r)) + [1] * len(r) for r in rows]
    return torch.tensor(ids, dtype=torch.int64, device=DEV), torch.tensor(mask, dtype=torch.int64, device=DEV)


def test_the_walks_are_disjoint():
    c0, c1, c2 = (set(_chain(a, N_ORACLE + 1)) for a in (A0, A1, A2))
    assert not (c0 & c1) and not (c0 & c2) and not (c1 & c2)


# ------------------------------------------------------------------------------------------------ 1. the draft rule per row
def test_draft_rule_per_row():
    from spatialrgpt_amd import ops

    max_new, ld, k, ng = 8, 24, 3, 2
    # (prompt, generated ids in out_ids, steps[b]): different lengths, sentinels inside, a count beyond max_new and a negative one
    rows = [([1, 2, 3, 4, 9, 1, 2, 5, 6, 7], [1, 2, 77, 77, 77, 77, 77, 77], 2),        # two matches of (1, 2): the earliest -> 3, 4, 9
            ([1, 2, 5, -200, 6, 1, 2], [77] * 8, 0),                                    # cut in front of the sentinel -> 5
            ([4, 4, 4], [1, 2, 3, 1, 2, 8, 1, 2], max_new + 5)]                         # clamped to 8 ids: (1, 2) at 3 -> 3, 1, 2
    want = [draft_ref(p + g[:min(max(s, 0), max_new)], k, ng, V) for p, g, s in rows]
    assert want == [[3, 4, 9], [5], [3, 1, 2]]
    B = len(rows)
    prompt = torch.empty((B, ld), dtype=torch.int64)
    for b, (p, _, _) in enumerate(rows):
        # behind n_prompt[b]: ids that WOULD match earlier / longer if they were read
        prompt[b] = torch.tensor((p + [1, 2, 11, 12, 13] * 5)[:ld])
    out_ids = torch.tensor([g for _, g, _ in rows], dtype=torch.int64)
    n_prompt = torch.tensor([len(p) for p, _, _ in rows], dtype=torch.int32)
    steps = torch.tensor([s for _, _, s in rows], dtype=torch.int32)
    big = torch.full((B + 2, k), SENT, dtype=torch.int64, device=DEV)
    big_n = torch.full((B + 2,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    draft, nd = ops.lookup_draft_batch(prompt.to(DEV), n_prompt.to(DEV), out_ids.to(DEV), steps.to(DEV), k, ng, V, draft=big[1:B + 1],
                                       n_draft=big_n[1:B + 1])
    torch.cuda.synchronize()
    for b in range(B):
        n = int(nd[b])
        assert draft[b, :n].tolist() == want[b] and draft[b, n:].tolist() == [-1] * (k - n), (b, draft[b].tolist(), want[b])
    assert bool((big[0] == SENT).all()) and bool((big[B + 1] == SENT).all())
    assert int(big_n[0]) == 0x5A5A5A5A and int(big_n[B + 1]) == 0x5A5A5A5A
    # no prompt ids at all, a negative count (no generated ids either: an empty history) and a count of one
    draft, nd = ops.lookup_draft_batch(None, torch.zeros((2,), dtype=torch.int32, device=DEV), torch.tensor([[6, 6, 6, 6], [6, 6, 6, 6]], device=DEV),
                                       torch.tensor([-3, 3], dtype=torch.int32, device=DEV), k, ng, V)
    assert nd.tolist() == [0, 1] and draft.tolist() == [[-1, -1, -1], [6, -1, -1]]
    assert draft_ref([6, 6, 6], k, ng, V) == [6]


# ------------------------------------------------------------------------------------------------ 2. step == composition
STEP_CASES = {2: lambda: [_partial(A0), _zero(A1)], 4: lambda: [_full(A0), _partial(A1), _zero(A2), tuple(_chain(A1, 3))]}


@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize("fmt", ["native", "fp8"])
def test_batched_step_equals_per_op_composition_bit_for_bit(fmt, B):
    """srgpt_llm_lookup_step_batch, three eager steps and three replays of its graph, against srgpt_lookup_draft_batch +
    srgpt_embed_rows + srgpt_gemv_rowss(batch = B * T) + srgpt_decode_attention_multi(B, T) + srgpt_argmax + srgpt_lookup_accept_batch
    on copies of the state; (4, 4) is the full 16-row pass"""
    from spatialrgpt_amd import _lib as L, ops

    prompts = STEP_CASES[B]()
    max_new, rounds = 32, 6
    wants = [_oracle_ids(p, max_new) for p in prompts]
    log, n_after = _replay(prompts, wants, K, max_new, rounds)
    assert all(r is not None for row in log for r in row) and max(n_after) < max_new  # nobody is frozen in these steps
    if B == 2:  # all vs none, then some vs none: different counts within a step, the three kinds over the steps
        assert log[0] == [(3, 3), (3, 0)] and log[1] == [(3, 1), (3, 0)], log
    else:       # all, some and none within ONE step (and a row with nothing to draft)
        assert log[1] == [(3, 3), (3, 1), (3, 0), (0, 0)] and _kinds(log[1]) == {"all", "some", "none"}, log
    assert len(set(len(p) for p in prompts)) > 1  # ragged

    eng = _model(fmt).engine
    cfg, w, lib = eng.cfg, eng.w, L.load()
    fp8 = fmt == "fp8"
    R = B * T
    Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
    assert ops.gemv_rowss_supported(R, fp8)
    st, _, ids, mask = _state(eng, prompts, max_new)
    lk = st.ensure_lookup_batch(K, 2, ids, mask)
    lk["steps"].fill_(1)
    assert lk["n_prompt"].tolist() == [len(p) for p in prompts] and lk["c"].ld_prompt > max(len(p) for p in prompts)
    graph = None

    def mat(name, i):
        if fp8 and name in w.llm_pk:
            return dict(w8=w.llm_pk[name][i], wscale=w.llm_q[name][1][i], packed_rows=w.pk_rows[name], n_rows=w.llm_q[name][0][i].shape[0])
        if fp8:
            return dict(w8=w.llm_q[name][0][i], wscale=w.llm_q[name][1][i])
        return dict(w=w.llm_t[name][i])

    tot = [0, 0, 0]
    for rnd in range(rounds):
        # ---- the composition, on copies
        kc, vc = st.kcache.clone(), st.vcache.clone()
        tok, out_ids, pos, step, steps = st.tok.clone(), st.out_ids.clone(), st.pos.clone(), st.step.clone(), lk["steps"].clone()
        stats = lk["stats"].clone()
        draft, nd = ops.lookup_draft_batch(lk["prompt"], lk["n_prompt"], out_ids, steps, K, 2, V)
        rows = []
        for b in range(B):
            r = [int(tok[b])] + draft[b, :int(nd[b])].tolist()
            rows += r + [r[-1]] * (T - len(r))
        h = ops.embed_rows(w.embed, torch.tensor(rows, device=DEV))
        ss = None
        for i in range(cfg.layers):
            qkv = ops.gemv_rowss(h, norm_w=w.llm_t["attn_norm"][i], eps=cfg.rms_eps, rowss_in=ss, **mat("wqkv", i))
            a = ops.decode_attention_multi(qkv.view(B, T, -1), kc[i], vc[i], pos, w.rope_cos, w.rope_sin, Hq, Hkv, D).view(R, -1)
            h, ss = ops.gemv_rowss(a, residual=h, publish=True, **mat("wo", i))
            act = ops.gemv_rowss(h, norm_w=w.llm_t["mlp_norm"][i], eps=cfg.rms_eps, swiglu=True, rowss_in=ss, **mat("wgu", i))
            h, ss = ops.gemv_rowss(act, residual=h, publish=True, **mat("wdown", i))
        head = dict(w8=w.lm_head8, wscale=w.lm_head_scale) if fp8 else dict(w=w.lm_head)
        ref = ops.gemv_rowss(h, norm_w=w.final_norm, eps=cfg.rms_eps, out_f32=True, rowss_in=ss, **head)
        ops.lookup_accept_batch(ops.argmax(ref), draft, nd, tok, out_ids, pos, steps, step, st.max_pos, stats=stats)
        # ---- the step: three eager, then three replays of its graph
        if rnd >= 3 and graph is None:
            with torch.cuda.stream(eng.stream):
                eng.stream.wait_stream(torch.cuda.default_stream())
                graph = st.ensure_lookup_batch_graph()
        _step(eng, st, lk, graph if rnd >= 3 else None)
        what = f"{fmt} B={B} round {rnd}"
        assert torch.equal(lk["logits"], ref), f"{what}: logits differ, max {float((lk['logits'] - ref).abs().max())}"
        assert torch.equal(st.out_ids, out_ids) and torch.equal(st.pos, pos) and torch.equal(st.tok, tok), what
        assert torch.equal(lk["steps"], steps) and torch.equal(st.step, step) and int(step) == int(steps.min()), what
        assert torch.equal(lk["stats"], stats), what
        assert torch.equal(_bits(st.kcache), _bits(kc)) and torch.equal(_bits(st.vcache), _bits(vc)), what
        # ... and what the CPU replay said this step would do
        tot = [tot[0] + 1, tot[1] + sum(d for d, _ in log[rnd]), tot[2] + sum(a for _, a in log[rnd])]
        assert lk["stats"].tolist() == tot, (what, lk["stats"].tolist(), tot)
    assert lk["steps"].tolist() == n_after
    for b in range(B):
        assert st.out_ids[b, :n_after[b]].tolist() == wants[b][:n_after[b]], b
    assert lib.srgpt_llm_lookup_sync_state_batch(C.byref(w.llm), C.byref(st.c), C.byref(lk["c"]), ops._stream()) == 0, L.last_error()


# ------------------------------------------------------------------------------------------------ 3. one sequence
def test_one_sequence_is_the_batch_one_step():
    """from identical states srgpt_llm_lookup_step_batch and srgpt_llm_lookup_step leave the same bits"""
    from spatialrgpt_amd import _lib as L, ops

    eng = _model().engine
    lib, w = L.load(), eng.w
    prompt = _partial(A0)
    max_new = 16
    assert simulate(prompt, _oracle_ids(prompt, max_new + T), K, 8) == (3, 9, 5)  # 3 of 3, 1 of 3, 1 of 3 in the steps below
    sa, _, ids, mask = _state(eng, [prompt], max_new)
    sb, _, _, _ = _state(eng, [prompt], max_new)
    la = sa.ensure_lookup(K, 2, ids[0])
    lb = sb.ensure_lookup_batch(K, 2, ids, mask)
    lb["steps"].fill_(1)
    assert torch.equal(_bits(sa.kcache), _bits(sb.kcache)) and torch.equal(sa.tok, sb.tok)
    for rnd in range(4):
        with torch.cuda.stream(eng.stream):
            eng.stream.wait_stream(torch.cuda.default_stream())
            L.check(lib.srgpt_llm_lookup_step(C.byref(w.llm), C.byref(sa.c), C.byref(la["c"]), ops._stream()))
        _step(eng, sb, lb)
        assert torch.equal(la["logits"], lb["logits"]), rnd
        assert torch.equal(sa.out_ids, sb.out_ids) and torch.equal(sa.pos, sb.pos) and torch.equal(sa.step, sb.step) and torch.equal(sa.tok, sb.tok)
        assert torch.equal(la["stats"], lb["stats"]) and torch.equal(lb["steps"], sb.step), rnd
        assert torch.equal(_bits(sa.kcache), _bits(sb.kcache)) and torch.equal(_bits(sa.vcache), _bits(sb.vcache)), rnd
    assert la["stats"].tolist() == [4, 9, 5]


# ------------------------------------------------------------------------------------------------ 4. a frozen row
@pytest.mark.parametrize("frozen", [0, 1])
def test_a_row_at_max_new_is_frozen_while_the_other_goes_on(frozen):
    """row `frozen` accepts everything and holds max_new = 8 ids after two steps; the other row emits one id per step.  out_ids lies
    between two sentinel rows and starts out filled with the sentinel (its rows are contiguous: the frozen row's other neighbour is
    the live row, whose ids and untouched tail are checked)"""
    from spatialrgpt_amd import _lib as L, ops

    max_new = 8
    prompts = [_full(A0), _zero(A1)] if frozen == 0 else [_zero(A1), _full(A0)]
    live = 1 - frozen
    wants = [_oracle_ids(p, N_ORACLE) for p in prompts]
    log, n_after = _replay(prompts, wants, K, max_new, 9)
    assert [row[frozen] for row in log] == [(3, 3), (3, 3)] + [None] * 7                  # 1 + 4 + 3 (cut at 8), then frozen
    assert [row[live] for row in log] == [(3, 0)] * 7 + [None] * 2 and n_after == [8, 8]   # one id per step, frozen after seven

    eng = _model().engine
    st, big, ids, mask = _state(eng, prompts, max_new, guard=True)
    lk = st.ensure_lookup_batch(K, 2, ids, mask)
    lk["steps"].fill_(1)
    for _ in range(2):
        _step(eng, st, lk)
    assert lk["steps"].tolist()[frozen] == max_new and lk["steps"].tolist()[live] == 3 and int(st.step) == 3
    assert lk["stats"].tolist() == [2, 12, 6]
    snap = dict(pos=int(st.pos[frozen]), tok=int(st.tok[frozen]), out=st.out_ids[frozen].tolist())
    assert snap["out"] == wants[frozen][:max_new]
    for n in range(3, 8):  # the live row goes on alone
        _step(eng, st, lk)
        assert lk["steps"].tolist()[frozen] == max_new and int(st.pos[frozen]) == snap["pos"] and int(st.tok[frozen]) == snap["tok"]
        assert st.out_ids[frozen].tolist() == snap["out"]
        assert lk["steps"].tolist()[live] == n + 1 and int(st.step) == n + 1
        assert lk["stats"].tolist() == [n, 6 + 3 * n, 6], n   # + {1, 3, 0}: the live row's alone
        assert st.out_ids[live, :n + 1].tolist() == wants[live][:n + 1] and st.out_ids[live, n + 1:].tolist() == [SENT] * (max_new - n - 1)
    assert lk["steps"].tolist() == [8, 8] and int(st.step) == 8
    state = (st.pos.tolist(), st.tok.tolist(), st.out_ids.tolist(), lk["stats"].tolist())
    for _ in range(2):  # every row frozen: a step that ran ahead changes and counts nothing
        _step(eng, st, lk)
    assert (st.pos.tolist(), st.tok.tolist(), st.out_ids.tolist(), lk["stats"].tolist()) == state and int(st.step) == 8
    assert state[2] == [wants[0][:max_new], wants[1][:max_new]] and state[3] == [7, 27, 6]
    assert bool((big[0] == SENT).all()) and bool((big[3] == SENT).all())
    assert L.load().srgpt_llm_lookup_sync_state_batch(C.byref(eng.w.llm), C.byref(st.c), C.byref(lk["c"]), ops._stream()) == 0, L.last_error()


# ------------------------------------------------------------------------------------------------ 5. end to end
@pytest.mark.parametrize("side", ["right", "left"])
def test_generate_with_ragged_acceptance(model_b, side):
    rows, n = [_prompt_full(), _prompt_zero(), _partial(A2)], 12
    wants = [_oracle_ids(r, N_ORACLE) for r in rows]
    sims = [simulate(r, w_, K, n) for r, w_ in zip(rows, wants)]
    assert sims[0] == (3, 9, 9) and sims[1] == (n - 1, 3 * (n - 1), 0)
    assert 0 < sims[2][2] < sims[2][1] and sims[0][0] < sims[2][0] < sims[1][0], sims  # partial: between the two, in drafts kept and in steps
    ids, mask = _pad(rows, side)
    out = model_b.generate(ids, attention_mask=mask, do_sample=False, eos_token_id=None, max_new_tokens=n, prompt_lookup_num_tokens=K)
    ll = dict(model_b.last_lookup)
    plain = model_b.generate(ids, attention_mask=mask, do_sample=False, eos_token_id=None, max_new_tokens=n)
    assert model_b.last_lookup["mode"] == "plain" and "not set" in model_b.last_lookup["reason"]
    assert out.cpu().tolist() == [w_[:n] for w_ in wants]
    assert torch.equal(out, plain)
    # the slowest row's steps, the rows' sums (a faster row is frozen at n ids while the others catch up)
    assert ll == dict(mode="lookup", reason="K = 3 drafts per step, batch 3", steps=max(s[0] for s in sims), tokens=3 * n,
                      drafted=sum(s[1] for s in sims), accepted=sum(s[2] for s in sims), batch=3), ll


# ------------------------------------------------------------------------------------------------ 6. EOS and criteria across rows
def test_eos_in_one_rows_accepted_run_and_a_criterion_on_a_column_reached_steps_apart(model_b):
    rows, n = [_full(A0), _zero(A1)], 12
    w0, w1 = (_oracle_ids(r, N_ORACLE) for r in rows)
    log, _ = _replay(rows, [w0, w1], K, n, 8)
    assert [r[0] for r in log[:2]] == [(3, 3), (3, 3)] and all(r[1] == (3, 0) for r in log)  # row 0: ids 1 | 2 .. 5 | 6 .. 9; row 1: one per step
    ids, mask = _pad(rows, "right")
    kw = dict(attention_mask=mask, do_sample=False, max_new_tokens=n)

    def both(**extra):
        plain = model_b.generate(ids, **kw, **extra)
        assert model_b.last_lookup["mode"] == "plain"
        out = model_b.generate(ids, prompt_lookup_num_tokens=K, **kw, **extra)
        assert model_b.last_lookup["mode"] == "lookup", model_b.last_lookup
        assert out.shape == plain.shape and torch.equal(out, plain), (extra, out, plain)
        return out.cpu().tolist()

    # id 7 of row 0 is the first accepted draft of its second step; row 1 never emits it and runs to the end
    eos = w0[6]
    assert eos not in w1[:n]
    got = both(eos_token_id=eos)
    assert got == [w0[:7] + [eos] * (n - 7), w1[:n]]
    assert model_b.last_lookup["tokens"] == 7 + n
    # every row ends, at different columns: the request is as long as the later one; a pad id of its own
    got = both(eos_token_id=[w0[6], w1[3]], pad_token_id=3)
    assert got == [w0[:7], w1[:4] + [3] * 3]
    # a criterion on column 8 of row 0: row 0 holds it after two steps, row 1 after seven
    crit = [lambda ids_, scores: int(ids_[0, -1]) == w0[7]]
    got = both(eos_token_id=None, stopping_criteria=crit)
    assert got == [w0[:8], w1[:8]]
    # ... one that needs both rows' ids of a column, and EOS ids with it (the column's EOS is judged first)
    crit = [lambda ids_, scores: ids_.shape[1] >= 5 and int(ids_[1, -1]) == w1[4] and int(ids_[0, -1]) == w0[4]]
    assert both(eos_token_id=None, stopping_criteria=crit) == [w0[:5], w1[:5]]
    assert both(eos_token_id=[w0[1], w1[4]], stopping_criteria=crit, pad_token_id=5) == [w0[:2] + [5] * 3, w1[:5]]


# ------------------------------------------------------------------------------------------------ 7. the pooled state afterwards
def test_a_plain_batched_request_follows_a_batched_lookup_request(model_b):
    rows, n = [_full(A0), _zero(A1)], 10
    w0, w1 = (_oracle_ids(r, N_ORACLE)[:n] for r in rows)
    ids, mask = _pad(rows, "left")
    kw = dict(attention_mask=mask, do_sample=False, max_new_tokens=n)
    # row 0 ends at its 7th id, inside an accepted run, while the device goes on with it: its position runs ahead of the kept ids
    out = model_b.generate(ids, eos_token_id=w0[6], prompt_lookup_num_tokens=K, **kw)
    assert out.cpu().tolist() == [w0[:7] + [w0[6]] * 3, w1]
    st = model_b.engine._state
    assert model_b.last_lookup["mode"] == "lookup" and st.batch == 2 and st._pos_stale
    assert st.host_len == [len(rows[0]) + 6, len(rows[1]) + n - 1] and int(st.pos[0]) > st.host_len[0]
    # the same pooled state: positions set by the prefill, the lookup workspace's tickets left at zero
    assert model_b.generate(ids, eos_token_id=None, **kw).cpu().tolist() == [w0, w1] and model_b.engine._state is st
    assert model_b.last_lookup["mode"] == "plain"
    # ... and a second lookup request on it, the rows swapped
    ids2, mask2 = _pad(rows[::-1], "right")
    out = model_b.generate(ids2, attention_mask=mask2, do_sample=False, eos_token_id=None, max_new_tokens=n, prompt_lookup_num_tokens=K)
    assert out.cpu().tolist() == [w1, w0] and model_b.engine._state is st and model_b.last_lookup["mode"] == "lookup"


# ------------------------------------------------------------------------------------------------ 8. fallbacks
def test_requests_the_batched_step_does_not_serve_run_the_plain_loop(model_b):
    rows = [_full(A0), _full(A1)]  # one length: no padding in these calls
    ids2, mask2 = _pad(rows, "right")
    ids9, mask9 = _pad([rows[i % 2] for i in range(9)], "right")
    assert bool(mask2.all()) and bool(mask9.all())
    ids1 = torch.tensor([list(rows[0])], dtype=torch.int64, device=DEV)
    cases = [("off", False, ids2, mask2, dict(do_sample=False), "batch 2: the lookup step takes one sequence"),
             ("do_sample", True, ids2, mask2, dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.9), "one Philox counter"),
             ("processors", True, ids2, mask2, dict(do_sample=False, repetition_penalty=1.2), "logits processors are on"),
             ("beams", True, ids2, mask2, dict(do_sample=False, num_beams=2), "num_beams > 1"),
             ("batch 9", True, ids9, mask9, dict(do_sample=False), "batch 9: two rows per sequence exceed the 16-row weight pass")]
    for name, on, ids, mask, kw, reason in cases:
        model_b.lookup_batch = on
        outs = []
        for extra in ({}, dict(prompt_lookup_num_tokens=K)):
            torch.manual_seed(11)
            outs.append(model_b.generate(ids, attention_mask=mask, max_new_tokens=6, eos_token_id=None, **kw, **extra))
            if extra:
                assert model_b.last_lookup["mode"] == "plain" and reason in model_b.last_lookup["reason"], (name, model_b.last_lookup)
                assert model_b.last_lookup["steps"] == 0
        assert torch.equal(outs[0], outs[1]), name
    # batch 1 with the switch on: the batch-1 step, as without it
    model_b.lookup_batch = True
    out = model_b.generate(ids1, max_new_tokens=12, eos_token_id=None, do_sample=False, prompt_lookup_num_tokens=K)
    assert out.cpu().tolist() == [_oracle_ids(rows[0], N_ORACLE)[:12]]
    assert model_b.last_lookup == dict(mode="lookup", reason="K = 3 drafts per step", steps=3, tokens=12, drafted=9, accepted=9)
    # llm.generate(inputs_embeds=...) has no prompt ids: every row drafts from its generated ids alone
    emb = model_b.engine.embed_tokens(ids2).to(model_b.dtype)
    out = model_b.llm.generate(inputs_embeds=emb, max_new_tokens=8, eos_token_id=None, do_sample=False, prompt_lookup_num_tokens=K)
    assert out.cpu().tolist() == [_oracle_ids(r, N_ORACLE)[:8] for r in rows]
    assert model_b.last_lookup == dict(mode="lookup", reason="K = 3 drafts per step, batch 2", steps=7, tokens=16, drafted=0, accepted=0, batch=2)
