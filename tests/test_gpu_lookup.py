"""Prompt-lookup decoding on the GPU: the draft rule (srgpt_lookup_draft) against a Python restatement of HF's
PromptLookupCandidateGenerator; the lookup step (srgpt_llm_lookup_step, eager and as a replayed graph, bf16 and fp8 W8A16) against its
composition from the per-op entries, bit for bit; rejected drafts leaving row 0 untouched; and generate(prompt_lookup_num_tokens=K)
end to end on PEAKED weights (tests.util.make_peaked: the greedy continuation walks a permutation with a margin asserted >= 10 x the
fp32-measured noise floor, as tests/test_gpu_freerun_parity.py does), where the expected ids come from the CPU oracle's plain greedy
loop -- never from the engine -- and the prompt constructions are checked on the CPU by replaying the draft rule over those ids.

Geometry: a true-width LLM-only config -- head_dim 128, 2 layers, hidden 512, heads 4 / kv_heads 1 (G = 4: four rows per step, K = 3),
3000 text ids in front of the mask and depth ids."""
import ctypes as C
import functools

import pytest
import torch

from tests.util import load_tiny, make_peaked

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
KW = dict(vit_hidden=64, vit_inter=128, vit_layers=2, vit_heads=4, image_size=56, patch_size=14, hidden=512, inter=1408, layers=2,
          heads=4, kv_heads=1, vocab=3002, mask_token_id=3000, depth_token_id=3001, rope_theta=10000.0)
V = KW["vocab"]
K = 3
MARGIN_OVER_FLOOR = 10.0
SENT = 0x5A5A5A5A5A5A


# ------------------------------------------------------------------------------------------------ the draft rule, restated
def draft_ref(hist, k, max_ngram, vocab):
    """HF PromptLookupCandidateGenerator.get_candidates on a list of ids; ids outside [0, vocab) never match and are never drafted"""
    real = lambda t: 0 <= t < vocab  # noqa: E731
    for n in range(min(max_ngram, len(hist) - 1), 0, -1):
        tail = hist[-n:]
        if not all(real(t) for t in tail):
            continue
        for i in range(len(hist) - n):
            if hist[i:i + n] == tail and real(hist[i + n]):
                out = []
                for t in hist[i + n:i + n + k]:
                    if not real(t):
                        break
                    out.append(t)
                return out
    return []


def simulate(prompt, ids, k, max_new, max_ngram=2):
    """the lookup loop replayed over the ids the model WILL pick (`ids`, at least max_new + k + 1 of them): the first id comes from
    the prefill, every step drafts from prompt + emitted ids, accepts the agreeing prefix and emits it + 1 -> (steps, drafted, accepted)"""
    n, steps, drafted, accepted = 1, 0, 0, 0
    while n < max_new:
        d = draft_ref(list(prompt) + list(ids[:n]), k, max_ngram, V)
        acc = 0
        while acc < len(d) and d[acc] == ids[n + acc]:
            acc += 1
        steps, drafted, accepted, n = steps + 1, drafted + len(d), accepted + acc, n + acc + 1
    return steps, drafted, accepted


DRAFT_CASES = [
    # (prompt, generated, K, max_ngram)
    ([5, 6, 7, 8], [9], 3, 2),                          # no match
    ([5, 6, 7, 8, 9, 6], [], 3, 2),                     # a match only at n = 1 (the pair (9, 6) occurs nowhere else)
    ([1, 2, 3, 4, 9, 1, 2, 5, 6, 7], [1, 2], 3, 2),     # two matches of (1, 2): the earliest wins -> 3, 4, 9
    ([1, 2, 3, 7, 7, 7], [1, 2], 2, 2),                 # K = 2 of the 4 ids that follow
    ([4, 4, 4, 1, 2, 3], [1, 2], 3, 2),                 # the continuation (3, 1, 2) runs into the generated ids
    ([8, 1, 2], [1], 3, 1),                             # a continuation shorter than K: (2, 1)
    ([1, 2, -200, 3, 1, 2], [], 3, 2),                  # a sentinel right behind the match: nothing to draft there, and nowhere else
    ([1, 2, 5, -200, 6, 1, 2], [], 3, 2),               # the draft is cut in front of the sentinel -> 5
    ([7, -200, 9, 7, -200], [], 3, 2),                  # sentinels inside the window: no match at n = 2 (and none at n = 1)
    ([3, -200, 5, 6, 9], [-200 + 203, 5], 3, 2),        # (3, 5) does not occur -- the sentinel between them is no wildcard --, n = 1 finds 5 -> 6, 9, 3
    ([1, 2, 3], [], 3, 2),                              # the trailing n-gram matches only itself
    ([6, 6], [], 3, 2),                                 # n = 1: the earlier 6 is followed by the last id -> 6
    ([], [4], 3, 2),                                    # a history of one id
    ([1, 2, 3, 4, 1, 2, 3, 9, 2, 3], [], 3, 3),         # max_ngram 3: (9, 2, 3) nowhere, then (2, 3) at 1 -> 4, 1, 2
    ([V, 1, V + 5, 1], [], 3, 2),                       # ids beyond the table are sentinels too
]


def test_draft_rule_equals_the_python_restatement():
    from spatialrgpt_amd import ops

    # the restatement itself, on the cases whose answer is evident
    assert draft_ref([5, 6, 7, 8, 9], 3, 2, V) == [] and draft_ref([1, 2, 3, 4, 9, 1, 2, 5, 6, 7, 1, 2], 3, 2, V) == [3, 4, 9]
    assert draft_ref([1, 2, 3], 3, 2, V) == [] and draft_ref([1, 2, 5, -200, 6, 1, 2], 3, 2, V) == [5] and draft_ref([6, 6], 3, 2, V) == [6]
    for prompt, gen, k, ng in DRAFT_CASES:
        want = draft_ref(prompt + gen, k, ng, V)
        max_new = 8
        out_ids = torch.full((max_new,), 77, dtype=torch.int64)  # ids behind *step are not history
        out_ids[:len(gen)] = torch.tensor(gen, dtype=torch.int64)
        p = torch.tensor(prompt, dtype=torch.int64, device=DEV) if prompt else None
        draft, nd = ops.lookup_draft(p, out_ids.to(DEV), torch.tensor([len(gen)], dtype=torch.int32, device=DEV), k, ng, V)
        nd = int(nd)
        assert draft[:nd].tolist() == want and draft[nd:].tolist() == [-1] * (k - nd), (prompt, gen, k, ng, draft.tolist(), want)
    # a long history: the earliest of many matches, found by whichever thread
    g = torch.Generator().manual_seed(5)
    long = torch.randint(0, 50, (5000,), generator=g).tolist()
    draft, nd = ops.lookup_draft(torch.tensor(long, dtype=torch.int64, device=DEV), torch.zeros((4,), dtype=torch.int64, device=DEV),
                                 torch.zeros((1,), dtype=torch.int32, device=DEV), 5, 3, V)
    assert draft[:int(nd)].tolist() == draft_ref(long, 5, 3, V) and int(nd) == 5


def test_batched_draft_of_one_sequence_is_the_single_draft():
    """srgpt_lookup_draft_batch with B = 1 against srgpt_lookup_draft, element for element: the two kernels find their history and
    call ONE draft body.  Every history above, at its own count, at max_new and beyond it (both clamp to the max_new ids of out_ids)"""
    from spatialrgpt_amd import ops

    max_new = 8
    for prompt, gen, k, ng in DRAFT_CASES:
        out_ids = torch.full((max_new,), 77, dtype=torch.int64)
        out_ids[:len(gen)] = torch.tensor(gen, dtype=torch.int64)
        out_ids = out_ids.to(DEV)
        p = torch.tensor(prompt, dtype=torch.int64, device=DEV) if prompt else None
        for count in (len(gen), max_new, max_new + 3):
            step = torch.tensor([count], dtype=torch.int32, device=DEV)
            one, n_one = ops.lookup_draft(p, out_ids, step, k, ng, V)
            many, n_many = ops.lookup_draft_batch(None if p is None else p[None], torch.tensor([len(prompt)], dtype=torch.int32, device=DEV),
                                                  out_ids[None], step, k, ng, V)
            assert torch.equal(many[0], one) and torch.equal(n_many, n_one), (prompt, gen, count, one.tolist(), many.tolist())


def test_accept_leaves_a_negative_count_alone():
    """srgpt_lookup_accept with *step = -1 (no state of a request): the sequence is frozen, as a row of the batched accept is -- no
    id is written in front of out_ids (a sentinel row on either side), nothing advances, nothing is counted"""
    from spatialrgpt_amd import ops

    T, max_new = 4, 8
    big = torch.full((3, max_new), SENT, dtype=torch.int64, device=DEV)
    big[1] = torch.arange(100, 100 + max_new, device=DEV)
    bufs = dict(big=big, tok=torch.tensor([41], dtype=torch.int64, device=DEV), pos=torch.tensor([9], dtype=torch.int32, device=DEV),
                step=torch.tensor([-1], dtype=torch.int32, device=DEV), tok_emb=torch.tensor([41], dtype=torch.int64, device=DEV),
                stats=torch.tensor([3, 7, 5], dtype=torch.int32, device=DEV))
    before = {k: v.clone() for k, v in bufs.items()}
    picks = torch.tensor([11, 12, 13, 14], dtype=torch.int64, device=DEV)
    draft = torch.tensor([11, 12, 99], dtype=torch.int64, device=DEV)  # two would be accepted, three ids emitted
    ops.lookup_accept(picks, draft, torch.tensor([T - 1], dtype=torch.int32, device=DEV), bufs["tok"], big[1], bufs["pos"], bufs["step"],
                      64, tok_emb=bufs["tok_emb"], stats=bufs["stats"])
    torch.cuda.synchronize()
    for k in bufs:
        assert torch.equal(bufs[k], before[k]), (k, bufs[k].tolist(), before[k].tolist())


# ------------------------------------------------------------------------------------------------ the peaked bundle
@functools.lru_cache(maxsize=None)
def _bundle():
    """peaked weights on the GPU, their host copies (bf16 values, and fp32 for the noise floor), the permutation"""
    from oracle import srgpt_oracle as so
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.weights import synth_state_dict

    cfg = SrgptConfig(**KW)
    assert cfg.head_dim == 128
    sd = synth_state_dict(cfg, seed=0, dtype=BF16, device=DEV)
    perm = make_peaked(sd, cfg)
    w_cpu = {k: v.cpu() for k, v in sd.items() if k.startswith("llm.")}
    return dict(so=so, cfg=cfg, ocfg=so.SrgptConfig(**KW), sd=sd, perm=perm, w_cpu=w_cpu, w32={k: v.float() for k, v in w_cpu.items()})


@functools.lru_cache(maxsize=None)
def _model(fmt="native"):
    from spatialrgpt_amd.model import LlavaLlamaModel

    b = _bundle()
    return LlavaLlamaModel(b["cfg"], dict(b["sd"]), device=DEV, dtype=BF16, rope_positions=512, llm_weight_format=fmt)


@functools.lru_cache(maxsize=None)
def _oracle_ids(prompt, n):
    """the CPU oracle's plain greedy loop over the text-only prompt (a tuple of ids) -> n new ids; asserts the premise: the top-1 /
    top-2 margin of every step is >= 10 x the noise floor measured against the same loop in fp32"""
    b = _bundle()
    so, ocfg = b["so"], b["ocfg"]

    def run(w, dtype):
        emb = torch.nn.functional.embedding(torch.tensor([list(prompt)]), w["llm.model.embed_tokens.weight"]).to(dtype)
        kv = so.KVCache(ocfg.layers)
        lg = so.llama_forward(w, ocfg, emb, torch.arange(len(prompt))[None], kv, last_only=True)[:, -1]
        ids, steps = [], []
        for t in range(n):
            steps.append(lg[0].float())
            ids.append(int(lg[0].argmax()))
            e = torch.nn.functional.embedding(torch.tensor([[ids[-1]]]), w["llm.model.embed_tokens.weight"]).to(dtype)
            lg = so.llama_forward(w, ocfg, e, torch.tensor([[len(prompt) + t]]), kv, last_only=True)[:, -1]
        return ids, torch.stack(steps)

    ids, lg16 = run(b["w_cpu"], BF16)
    ids32, lg32 = run(b["w32"], torch.float32)
    assert ids == ids32
    top2 = lg16.topk(2, dim=-1).values
    floor = float((lg16 - lg32).abs().max())
    margin = float((top2[:, 0] - top2[:, 1]).min())
    assert margin >= MARGIN_OVER_FLOOR * floor, (margin, floor)
    return ids


def _chain(a, n):
    perm = _bundle()["perm"]
    out = [a]
    for _ in range(n):
        out.append(int(perm[out[-1]]))
    return out


A0 = 17         # the walk's start
N_ORACLE = 16   # ids the oracle generates per prompt: the longest request (12) and what a step may pick beyond it (K + 1)


def _prompt_full():
    """a, perm[a], ..., perm^12[a], a: every draft agrees with the model"""
    return tuple(_chain(A0, 12) + [A0])


def _prompt_zero():
    """a, z, perm[a], z, perm^2[a], z, ..., a: every hop of the walk is in the prompt, followed by an id the model does not pick"""
    chain = _chain(A0, 12)
    z = next(t for t in range(100, V) if t not in chain and all(int(_bundle()["perm"][c]) != t for c in chain))
    out = []
    for c in chain:
        out += [c, z]
    return tuple(out + [A0])


def _gen(model, prompt, **kw):
    ids = torch.tensor([list(prompt)], dtype=torch.int64, device=DEV)
    kw.setdefault("do_sample", False)
    kw.setdefault("eos_token_id", None)
    return model.generate(ids, **kw)


# ------------------------------------------------------------------------------------------------ 4. step == composition
def _state_after_first_token(eng, prompt, max_new, guard=False):
    """a fresh batch-1 state: the prompt prefilled, the first token picked (srgpt_llm_sample_first)"""
    from spatialrgpt_amd import _lib as L, ops

    st = eng.new_state(1, 256, max_new, ws_tokens=len(prompt))
    big = None
    if guard:  # out_ids between two sentinel rows
        big = torch.full((3, max_new), SENT, dtype=torch.int64, device=DEV)
        st.out_ids = big[1:2]
        st.c.out_ids = st.out_ids.data_ptr()
    eng.prefill(eng.embed_tokens(torch.tensor([list(prompt)], device=DEV)), max_new=max_new, state=st)
    L.check(L.load().srgpt_llm_sample_first(C.byref(eng.w.llm), C.byref(st.c), ops._stream()))
    return st, big


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


@pytest.mark.parametrize("fmt", ["native", "fp8"])
def test_lookup_step_equals_per_op_composition_bit_for_bit(fmt):
    """srgpt_llm_lookup_step, eager and as a replayed graph, against srgpt_lookup_draft + srgpt_embed_rows + srgpt_gemv_rowss(batch = T)
    + srgpt_decode_attention_multi + srgpt_argmax + srgpt_lookup_accept on a copy of the state: logits [T, V], out_ids, pos, step, tok
    and the caches, over steps that accept all, some and none of their drafts"""
    from spatialrgpt_amd import _lib as L, ops

    eng = _model(fmt).engine
    cfg, w, lib = eng.cfg, eng.w, L.load()
    fp8 = fmt == "fp8"
    T = K + 1
    Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
    assert ops.gemv_rowss_supported(T, fp8)
    chain = _chain(A0, 12)
    # the walk, then a stretch whose continuation the model does not follow (partial and zero acceptance), ending in a
    prompt = chain[:6] + [chain[6], 999, chain[7], chain[8], 998] + [A0]
    max_new = 16
    st, _ = _state_after_first_token(eng, prompt, max_new)
    lk = st.ensure_lookup(K, 2, torch.tensor(prompt, dtype=torch.int64))
    graph = None

    def mat(name, i):
        if fp8 and name in w.llm_pk:
            return dict(w8=w.llm_pk[name][i], wscale=w.llm_q[name][1][i], packed_rows=w.pk_rows[name], n_rows=w.llm_q[name][0][i].shape[0])
        if fp8:
            return dict(w8=w.llm_q[name][0][i], wscale=w.llm_q[name][1][i])
        return dict(w=w.llm_t[name][i])

    assert 999 not in chain and 998 not in chain
    for rnd in range(6):
        # ---- the composition, on copies
        kc, vc = st.kcache.clone(), st.vcache.clone()
        tok, out_ids, pos, step = st.tok.clone(), st.out_ids.clone(), st.pos.clone(), st.step.clone()
        stats = lk["stats"].clone()
        draft, nd = ops.lookup_draft(lk["prompt"], out_ids[0], step, K, 2, V)
        n = int(nd)
        rows = [int(tok)] + draft[:n].tolist()
        rows += [rows[-1]] * (T - len(rows))
        h = ops.embed_rows(w.embed, torch.tensor(rows, device=DEV))
        ss = None
        for i in range(cfg.layers):
            qkv = ops.gemv_rowss(h, norm_w=w.llm_t["attn_norm"][i], eps=cfg.rms_eps, rowss_in=ss, **mat("wqkv", i))
            a = ops.decode_attention_multi(qkv[None], kc[i], vc[i], pos, w.rope_cos, w.rope_sin, Hq, Hkv, D)[0]
            h, ss = ops.gemv_rowss(a, residual=h, publish=True, **mat("wo", i))
            act = ops.gemv_rowss(h, norm_w=w.llm_t["mlp_norm"][i], eps=cfg.rms_eps, swiglu=True, rowss_in=ss, **mat("wgu", i))
            h, ss = ops.gemv_rowss(act, residual=h, publish=True, **mat("wdown", i))
        head = dict(w8=w.lm_head8, wscale=w.lm_head_scale) if fp8 else dict(w=w.lm_head)
        ref = ops.gemv_rowss(h, norm_w=w.final_norm, eps=cfg.rms_eps, out_f32=True, rowss_in=ss, **head)
        ops.lookup_accept(ops.argmax(ref), draft, nd, tok, out_ids[0], pos, step, st.max_pos, stats=stats)
        # ---- the step: three eager, then three replays of its graph
        with torch.cuda.stream(eng.stream):
            eng.stream.wait_stream(torch.cuda.default_stream())
            if rnd < 3:
                L.check(lib.srgpt_llm_lookup_step(C.byref(w.llm), C.byref(st.c), C.byref(lk["c"]), ops._stream()))
            else:
                graph = graph or st.ensure_lookup_graph()
                L.check(lib.srgpt_graph_launch(graph, 1, ops._stream()))
        eng.stream.synchronize()
        what = f"{fmt} round {rnd}"
        assert torch.equal(lk["logits"], ref), f"{what}: logits differ, max {float((lk['logits'] - ref).abs().max())}"
        assert torch.equal(st.out_ids, out_ids) and torch.equal(st.pos, pos) and torch.equal(st.step, step) and torch.equal(st.tok, tok), what
        assert torch.equal(lk["stats"], stats), what
        assert torch.equal(_bits(st.kcache), _bits(kc)) and torch.equal(_bits(st.vcache), _bits(vc)), what
        assert int(lk["stats"][0]) == rnd + 1 and int(step) < max_new, what
    # the ids are the oracle's walk, and the steps met full, partial and zero acceptance
    got = st.out_ids[0, :int(st.step)].tolist()
    assert got == _oracle_ids(tuple(prompt), max_new)[:len(got)]
    assert lk["stats"].tolist() == [6, 9, 5], lk["stats"].tolist()  # 3 of 3, 1 of 3, 1 of 3, then three steps without a match
    assert lib.srgpt_llm_lookup_sync_state(C.byref(w.llm), C.byref(st.c), C.byref(lk["c"]), ops._stream()) == 0, L.last_error()


# ------------------------------------------------------------------------------------------------ 5. rejected drafts do not perturb
def test_rejected_drafts_do_not_perturb_row_zero():
    """the same state stepped with no history match and with deliberately wrong drafts: row 0's logits and the emitted token are
    bit-identical (its column sees no key behind its own position, the products treat their rows independently)"""
    from spatialrgpt_amd import _lib as L, ops

    eng = _model().engine
    lib, w = L.load(), eng.w
    prompt = _chain(A0, 4)[:4]
    res = []
    for planted in (False, True):
        st, _ = _state_after_first_token(eng, prompt, 8)
        first = int(st.tok)
        # no match: the lookup history is empty; planted: the first token followed by three ids the model does not pick
        hist = torch.tensor([first, 1500, 1501, 1502] if planted else [], dtype=torch.int64)
        assert 1500 != int(_bundle()["perm"][first])
        lk = st.ensure_lookup(K, 2, hist if planted else None)
        with torch.cuda.stream(eng.stream):
            eng.stream.wait_stream(torch.cuda.default_stream())
            L.check(lib.srgpt_llm_lookup_step(C.byref(w.llm), C.byref(st.c), C.byref(lk["c"]), ops._stream()))
        eng.stream.synchronize()
        res.append(dict(logits=lk["logits"][0].clone(), tok=int(st.tok), step=int(st.step), pos=int(st.pos), stats=lk["stats"].tolist(),
                        out=st.out_ids[0, :2].tolist()))
    assert res[0]["stats"] == [1, 0, 0] and res[1]["stats"] == [1, 3, 0]
    assert torch.equal(res[0]["logits"], res[1]["logits"])
    for key in ("tok", "step", "pos", "out"):
        assert res[0][key] == res[1][key], key
    assert res[0]["step"] == 2 and res[0]["pos"] == len(prompt) + 1


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_full_acceptance():
    prompt, n = _prompt_full(), 12
    want = _oracle_ids(prompt, N_ORACLE)
    assert want[:n] == _chain(A0, 12)[1:]  # the walk
    assert simulate(prompt, want, K, n) == (3, 9, 9)  # on the CPU, before the GPU is touched: 1 + 4 + 4 + 4 ids
    model = _model()
    out = _gen(model, prompt, max_new_tokens=n, prompt_lookup_num_tokens=K)
    assert out.cpu().tolist() == [want[:n]]
    ll = model.last_lookup
    assert ll["mode"] == "lookup" and ll["tokens"] == n and ll["steps"] <= 4 and ll["accepted"] == ll["drafted"], ll
    assert (ll["steps"], ll["drafted"], ll["accepted"]) == (3, 9, 9), ll


def test_zero_acceptance():
    prompt, n = _prompt_zero(), 12
    want = _oracle_ids(prompt, N_ORACLE)
    assert simulate(prompt, want, K, n) == (n - 1, 3 * (n - 1), 0)
    model = _model()
    out = _gen(model, prompt, max_new_tokens=n, prompt_lookup_num_tokens=K)
    assert out.cpu().tolist() == [want[:n]]
    ll = model.last_lookup
    assert ll["mode"] == "lookup" and ll["accepted"] == 0 and ll["steps"] == ll["tokens"] - 1 == n - 1 and ll["drafted"] == 3 * (n - 1), ll


def test_eos_and_stopping_criteria_inside_an_accepted_run():
    """ids 1 | 2 3 4 5 | 6 7 8 9 | ...: id 7 is the first accepted draft of its step, id 8 the second"""
    prompt, n = _prompt_full(), 12
    want = _oracle_ids(prompt, N_ORACLE)
    model = _model()
    eos = want[6]
    plain = _gen(model, prompt, max_new_tokens=n, eos_token_id=eos)
    assert model.last_lookup["mode"] == "plain"
    out = _gen(model, prompt, max_new_tokens=n, eos_token_id=eos, prompt_lookup_num_tokens=K)
    assert model.last_lookup["mode"] == "lookup" and model.last_lookup["tokens"] == 7
    assert torch.equal(out, plain) and out.cpu().tolist() == [want[:7]]
    # an EOS list and a pad id: cut and padded exactly as the plain loop's
    for kw in (dict(eos_token_id=[want[9], want[4]], pad_token_id=3), dict(eos_token_id=[want[0]])):
        a, b = _gen(model, prompt, max_new_tokens=n, **kw), _gen(model, prompt, max_new_tokens=n, prompt_lookup_num_tokens=K, **kw)
        assert torch.equal(a, b), (kw, a, b)
    crit = [lambda ids, scores: int(ids[0, -1]) == want[7]]
    plain = _gen(model, prompt, max_new_tokens=n, stopping_criteria=crit)
    out = _gen(model, prompt, max_new_tokens=n, stopping_criteria=crit, prompt_lookup_num_tokens=K)
    assert torch.equal(out, plain) and out.cpu().tolist() == [want[:8]]


def test_max_new_tokens_inside_an_emission_and_out_ids_not_overrun():
    """10 ids = 1 + 4 + 4 + the first of a step that would emit 4: exactly 10 come back, and out_ids -- 10 long, between two sentinel
    rows -- is not overrun however many steps run ahead"""
    prompt, n = _prompt_full(), 10
    want = _oracle_ids(prompt, N_ORACLE)
    eng = _model().engine
    st, big = _state_after_first_token(eng, prompt, n, guard=True)
    out = eng.greedy_decode(st, n, lookup=dict(K=K, max_ngram=2, prompt_ids=torch.tensor(prompt, dtype=torch.int64)))
    torch.cuda.synchronize()
    assert out.shape == (1, n) and out.cpu().tolist() == [want[:n]]
    assert eng.last_lookup_stats["tokens"] == n and eng.last_lookup_stats["steps"] == 3
    assert bool((big[0] == SENT).all()) and bool((big[2] == SENT).all()) and big[1].tolist() == want[:n]
    # through generate(): 5 and 2 ids (a cut inside the first step, and a request of one step)
    model = _model()
    for m in (5, 2, 1):
        assert _gen(model, prompt, max_new_tokens=m, prompt_lookup_num_tokens=K).cpu().tolist() == [want[:m]], m


@pytest.mark.parametrize("second", ["plain", "lookup"])
def test_returned_state_continues(second):
    """return_dict_in_generate=True after a lookup request: the state continues with a plain generate(past_key_values=...) and with
    another lookup request to the oracle's ids over the whole conversation (host_len / pending / tok_emb are right)"""
    prompt, n1, n2 = _prompt_full(), 6, 7
    first = _oracle_ids(prompt, N_ORACLE)[:n1]
    seg = (_chain(A0, 30)[20], )
    whole = tuple(prompt) + tuple(first) + seg
    want2 = _oracle_ids(whole, n2)
    model = _model()
    r = _gen(model, prompt, max_new_tokens=n1, prompt_lookup_num_tokens=K, return_dict_in_generate=True)
    assert r.sequences.cpu().tolist() == [first] and model.last_lookup["mode"] == "lookup"
    st = r.past_key_values
    assert st.host_len == [len(prompt) + n1 - 1] and st.pending is not None
    kw = dict(prompt_lookup_num_tokens=K) if second == "lookup" else {}
    out = _gen(model, seg, max_new_tokens=n2, past_key_values=st, **kw)
    assert out.cpu().tolist() == [want2] and model.last_lookup["mode"] == second
    assert st.host_len == [len(whole) + n2 - 1]


def test_requests_the_lookup_step_does_not_serve_fall_back_unchanged():
    """do_sample, num_beams = 2, batch 2, repetition_penalty: with the keyword the ids equal the same call without it"""
    model = _model()
    prompt = _prompt_full()
    ids1 = torch.tensor([list(prompt)], dtype=torch.int64, device=DEV)
    ids2 = torch.tensor([list(prompt), list(_prompt_zero())[:len(prompt)]], dtype=torch.int64, device=DEV)
    cases = [("do_sample", ids1, dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.9)), ("num_beams", ids1, dict(do_sample=False, num_beams=2)),
             ("batch", ids2, dict(do_sample=False)), ("logits processors", ids1, dict(do_sample=False, repetition_penalty=1.2))]
    for name, ids, kw in cases:
        outs = []
        for extra in ({}, dict(prompt_lookup_num_tokens=K)):
            torch.manual_seed(11)
            outs.append(model.generate(ids, max_new_tokens=8, eos_token_id=None, **kw, **extra))
            if extra:
                assert model.last_lookup["mode"] == "plain" and name.split("_")[0] in model.last_lookup["reason"], (name, model.last_lookup)
        assert torch.equal(outs[0], outs[1]), name
    # the keyword off, K = 0 and None: the plain loop, and it says so
    for extra in ({}, dict(prompt_lookup_num_tokens=0), dict(prompt_lookup_num_tokens=None)):
        model.generate(ids1, max_new_tokens=4, eos_token_id=None, do_sample=False, **extra)
        assert model.last_lookup["mode"] == "plain" and "not set" in model.last_lookup["reason"]
    # a K beyond the attention's columns is clamped (G = 4: 4 rows per step), max_matching_ngram_size is honoured
    out = model.generate(ids1, max_new_tokens=12, eos_token_id=None, do_sample=False, prompt_lookup_num_tokens=10, max_matching_ngram_size=1)
    assert out.cpu().tolist() == [_oracle_ids(prompt, N_ORACLE)[:12]] and model.last_lookup["mode"] == "lookup"
    assert "K = 3" in model.last_lookup["reason"] and model.last_lookup["drafted"] <= 3 * model.last_lookup["steps"]
    # llm.generate(inputs_embeds=...) has no prompt ids: the history is the generated ids alone
    emb = model.engine.embed_tokens(ids1).to(model.dtype)
    out = model.llm.generate(inputs_embeds=emb, max_new_tokens=12, eos_token_id=None, do_sample=False, prompt_lookup_num_tokens=K)
    assert out.cpu().tolist() == [_oracle_ids(prompt, N_ORACLE)[:12]] and model.last_lookup == dict(
        mode="lookup", reason="K = 3 drafts per step", steps=11, tokens=12, drafted=0, accepted=0)


# ------------------------------------------------------------------------------------------------ 7. the tiny fp32 golden
def test_tiny_fp32_golden_ids_with_the_keyword():
    """generate(prompt_lookup_num_tokens=2) on tests/golden/tiny_fp32.npz (fp32, head_dim 16: the composed attention route) returns
    the reference's ids"""
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.model import LlavaLlamaModel

    cfgd, dtype, w, inp, ref = load_tiny("tiny_fp32.npz")
    model = LlavaLlamaModel(SrgptConfig.from_dict(cfgd), dict(w), device=DEV, dtype=dtype, rope_positions=1024)
    n = ref["new_ids"].shape[1]
    kw = dict(images=inp["images"].to(DEV), depths=inp["depths"].to(DEV), masks=[m.to(DEV) for m in inp["masks"]], do_sample=False,
              max_new_tokens=n, eos_token_id=None)
    out = model.generate(inp["input_ids"].to(DEV), prompt_lookup_num_tokens=2, **kw)
    assert model.last_lookup["mode"] == "lookup" and model.last_lookup["tokens"] == n, model.last_lookup
    assert torch.equal(out.cpu(), ref["new_ids"]), (out.cpu(), ref["new_ids"])
