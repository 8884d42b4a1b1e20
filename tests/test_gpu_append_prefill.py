"""srgpt_llm_prefill_append -- a multi-token segment appended to a LIVE KV cache -- on the geometry, oracle call and tolerance of
tests/test_gpu_pipeline.py::test_decode_equals_teacher_forced_prefill: hidden 512, inter 1408, 3 layers, heads 8 / 2, head_dim 64,
rope_positions 512; the oracle is `so.llama_forward` with an `so.KVCache` over the WHOLE sequence; the bar is
(3e-2 bf16 | 2e-4 fp32) x max |logits|.  What is checked: (1) on rows at position 0 the call writes srgpt_llm_prefill's bytes;
(2) prefill + append == the oracle over the concatenation, and so are decode steps over the appended cache; (3) chains of appends and a
ragged batch at per-row live lengths; (4) the cache outside [pos0, pos0 + T) keeps its bits; (5) a device position beyond the host's
bound raises the sticky error word and writes inside the cache; (6) both fp8 formats; (7) captured and eager steps after an append
agree bit for bit."""
import ctypes as C
import functools

import pytest
import torch

from tests.util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
KW = dict(vit_hidden=64, vit_inter=128, vit_layers=2, vit_heads=4, image_size=56, patch_size=14, hidden=512, inter=1408,
          layers=3, heads=8, kv_heads=2, vocab=1000, mask_token_id=998, depth_token_id=999, rope_theta=10000.0)
H = KW["hidden"]


def _rel(dtype):
    """the bar of test_decode_equals_teacher_forced_prefill, as a fraction of max |logits|"""
    return 3e-2 if dtype == BF16 else 2e-4


@functools.lru_cache(maxsize=None)
def _setup(dtype, fmt="native"):
    """(oracle config, oracle weights [dequantised for the fp8 formats], engine) -- built once per (dtype, weight format)"""
    from oracle import srgpt_oracle as so
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine

    ocfg = so.SrgptConfig(**KW)
    w = so.synth_weights(ocfg, seed=3, dtype=dtype)
    eng = SrgptEngine(SrgptConfig(**KW), dict(w), device=DEV, dtype=dtype, rope_positions=512, llm_weight_format=fmt)
    return ocfg, (w if fmt == "native" else so.fp8_dequantised_weights(w)), eng


def _x(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 0.5).to(dtype)


@functools.lru_cache(maxsize=None)
def _oracle(dtype, fmt, n, seed, steps=0, act_quant=False):
    """the oracle's logits over ONE sequence of n rows (_x((1, n, H), dtype, seed)), then over `steps` teacher-forced tokens
    (ids 3, 4, ...) fed one at a time through the same cache.  Computed once per case and shared; -> ([n, V], [steps, V])"""
    from oracle import srgpt_oracle as so

    ocfg, w, _ = _setup(dtype, fmt)
    kv = so.KVCache(ocfg.layers)
    kw = dict(act_quant=so.fp8_rowwise_fake_quant) if act_quant else {}
    ref = so.llama_forward(w, ocfg, _x((1, n, H), dtype, seed), torch.arange(n)[None], kv, **kw)[0]
    out = []
    for s in range(steps):  # decode is W8A16 under both fp8 formats: no activation quantisation
        emb = torch.nn.functional.embedding(torch.tensor([[3 + s]]), w["llm.model.embed_tokens.weight"])
        out.append(so.llama_forward(w, ocfg, emb, torch.tensor([[n + s]]), kv)[0, 0])
    return ref, (torch.stack(out) if out else None)


def _lib():
    from spatialrgpt_amd import _lib as L, ops
    return L.load(), L, ops


def _prefill_append(eng, st, x, T, lens, h_pos_max, all_logits=True, hidden=False):
    """srgpt_llm_prefill_append straight at the C ABI -> (rc, all_logits, hidden_out)"""
    lib, L, ops = _lib()
    B = x.shape[0]
    al = torch.full((B, T, eng.w.vocab), float("nan"), device=DEV, dtype=F32) if all_logits else None
    hs = torch.full((eng.cfg.layers + 1, B, T, H), float("nan"), device=DEV, dtype=eng.dtype) if hidden else None
    rc = lib.srgpt_llm_prefill_append(C.byref(eng.w.llm), C.byref(st.c), x.data_ptr(), T, None if lens is None else lens.data_ptr(),
                                      h_pos_max, None if al is None else al.data_ptr(), None if hs is None else hs.data_ptr(), ops._stream())
    return rc, al, hs


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


# ------------------------------------------------------------------------------------------------ 1. position 0 == srgpt_llm_prefill
@pytest.mark.parametrize("dtype,fmt,B,T", [(BF16, "native", 2, 37), (F32, "native", 2, 37), (BF16, "native", 1, 130), (BF16, "fp8", 2, 37),
                                           (BF16, "fp8_w8a8", 2, 37)])
def test_append_at_position_zero_writes_the_bytes_of_prefill(dtype, fmt, B, T):
    """all rows at position 0, lens NULL, h_pos_max 0: st->logits, all_logits, the hidden states, cache rows [0, T) of every layer and
    pos are srgpt_llm_prefill's, bit for bit (same products, same routes, same attention tiles)"""
    lib, L, ops = _lib()
    _, _, eng = _setup(dtype, fmt)
    x = _x((B, T, H), dtype, 11).to(DEV)
    got = []
    for append in (False, True):
        st = eng.new_state(B, 256, 4, ws_tokens=T)
        st.kcache.fill_(float("nan"))
        st.vcache.fill_(float("nan"))
        st.logits.fill_(float("nan"))
        if append:
            rc, al, hs = _prefill_append(eng, st, x, T, None, 0, hidden=True)
        else:
            al = torch.full((B, T, eng.w.vocab), float("nan"), device=DEV, dtype=F32)
            hs = torch.full((eng.cfg.layers + 1, B, T, H), float("nan"), device=DEV, dtype=dtype)
            rc = lib.srgpt_llm_prefill(C.byref(eng.w.llm), C.byref(st.c), x.data_ptr(), T, al.data_ptr(), hs.data_ptr(), ops._stream())
        L.check(rc)
        torch.cuda.synchronize()
        assert lib.srgpt_llm_decode_sync_state(C.byref(eng.w.llm), C.byref(st.c), ops._stream()) == 0
        got.append(dict(logits=st.logits.clone(), all_logits=al, hidden=_bits(hs), k=_bits(st.kcache[:, :, :, :T]).clone(),
                        v=_bits(st.vcache[:, :, :, :T]).clone(), k_rest=_bits(st.kcache[:, :, :, T:]).clone(), pos=st.pos.clone()))
    assert bool(torch.isfinite(got[0]["all_logits"]).all()) and got[0]["pos"].tolist() == [T] * B
    for key in got[0]:
        assert torch.equal(got[0][key], got[1][key]), f"{key} differs from srgpt_llm_prefill ({dtype}, {fmt})"


# ------------------------------------------------------------------------------------------------ 2. prefill | append == the oracle
def _split_case(dtype, fmt, P, N, rel, act_quant=False, steps=3):
    """prefill x[:, :P], append x[:, P:]: the appended rows' all_logits and st.logits against the oracle's rows over the whole
    sequence, then `steps` teacher-forced step()s (the decode kernels read the appended cache) against the oracle's"""
    _, _, eng = _setup(dtype, fmt)
    ref, ref_steps = _oracle(dtype, fmt, P + N, 5, steps, act_quant)
    tol = rel * float(ref.abs().max())
    x = _x((1, P + N, H), dtype, 5).to(DEV)
    st = eng.new_state(1, 256, 4)
    eng.prefill(x[:, :P], max_new=1, state=st)
    _, al, _ = eng.append(st, x[:, P:], all_logits=True)
    what = f"{dtype} {fmt} split ({P}, {N})"
    assert st.host_len == [P + N] and st.pos.tolist() == [P + N], what
    assert_close(al[0], ref[P:], tol, 0, "appended rows' logits vs the oracle, " + what)
    assert_close(st.logits[0], ref[-1], tol, 0, "st.logits vs the oracle's last row, " + what)
    for s in range(steps):
        lg = eng.step(st, torch.tensor([[3 + s]], device=DEV))
        assert_close(lg[0], ref_steps[s], tol, 0, f"decode step {s} over the appended cache vs the oracle, " + what)
    lib, L, ops = _lib()
    assert lib.srgpt_llm_decode_sync_state(C.byref(eng.w.llm), C.byref(st.c), ops._stream()) == 0


@pytest.mark.parametrize("P,N", [(36, 1), (20, 17), (1, 36), (64, 66), (63, 67)])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_prefill_then_append_equals_the_oracle_over_the_whole_sequence(dtype, P, N):
    _split_case(dtype, "native", P, N, _rel(dtype))


# ------------------------------------------------------------------------------------------------ 3. chains, ragged batches
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_three_chunk_chain(dtype):
    """prefill 20 | append 17 | append 30 (the second append starts at an odd position inside a key tile and ends in the next)"""
    _, _, eng = _setup(dtype)
    cuts = [0, 20, 37, 67]
    ref, _ = _oracle(dtype, "native", cuts[-1], 5)
    tol = _rel(dtype) * float(ref.abs().max())
    x = _x((1, cuts[-1], H), dtype, 5).to(DEV)
    st = eng.new_state(1, 128, 2, ws_tokens=32)
    eng.prefill(x[:, :20], max_new=1, state=st)
    for a, b in zip(cuts[1:-1], cuts[2:]):
        _, al, _ = eng.append(st, x[:, a:b], all_logits=True)
        assert_close(al[0], ref[a:b], tol, 0, f"chain rows [{a}, {b}) vs the oracle ({dtype})")
        assert_close(st.logits[0], ref[b - 1], tol, 0, f"chain st.logits after row {b - 1} ({dtype})")
    assert st.pos.tolist() == [67] and st.host_len == [67]


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_ragged_batch_appends_at_per_row_live_lengths(dtype):
    """B = 3 at live lengths [5, 37, 20] (a ragged prefill) appends lens = [17, 1, 9] rows of a right-padded segment: every row
    against the oracle of that row ALONE over its prompt rows + its segment rows; the padding holds garbage"""
    from oracle import srgpt_oracle as so

    ocfg, w, eng = _setup(dtype)
    live, lens = [5, 37, 20], [17, 1, 9]
    P, T = max(live), max(lens)
    xp, xs = _x((3, P, H), dtype, 21), _x((3, T, H), dtype, 22)
    for b in range(3):
        xp[b, live[b]:] = 77.0
        xs[b, lens[b]:] = 77.0
    st = eng.new_state(3, 128, 2)
    eng.prefill(xp.to(DEV), max_new=1, lens=torch.tensor(live), state=st)
    _, al, _ = eng.append(st, xs.to(DEV), lens=torch.tensor(lens), all_logits=True)
    assert st.pos.tolist() == [a + n for a, n in zip(live, lens)] == st.host_len
    for b in range(3):
        row = torch.cat([xp[b:b + 1, :live[b]], xs[b:b + 1, :lens[b]]], 1)
        ref = so.llama_forward(w, ocfg, row, torch.arange(row.shape[1])[None], so.KVCache(ocfg.layers))[0]
        tol = _rel(dtype) * float(ref.abs().max())
        assert_close(al[b, :lens[b]], ref[live[b]:], tol, 0, f"ragged append row {b}: appended rows vs the row alone ({dtype})")
        assert_close(st.logits[b], ref[-1], tol, 0, f"ragged append row {b}: st.logits ({dtype})")


# ------------------------------------------------------------------------------------------------ 4. the cache outside the segment
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_append_leaves_the_rest_of_the_cache_alone(dtype):
    """cache pre-filled with a sentinel bit pattern (NaN), B = 2 at live lengths [20, 7], T = 17: in every layer rows [0, pos0) keep
    the prefill's bits, rows >= pos0 + T the sentinel's, and (fp32) the appended K / V rows are srgpt_rope_kv_append's for the same
    q/k/v rows -- the layer's input rows (hidden_out) through srgpt_rmsnorm and srgpt_gemm"""
    lib, L, ops = _lib()
    _, _, eng = _setup(dtype)
    cfg = eng.cfg
    live, T = [20, 7], 17
    st = eng.new_state(2, 64, 2)
    st.kcache.fill_(float("nan"))
    st.vcache.fill_(float("nan"))
    sentinel = _bits(st.kcache[0, 0, 0, 0]).clone()
    xp = _x((2, max(live), H), dtype, 31).to(DEV)
    eng.prefill(xp, max_new=1, lens=torch.tensor(live), state=st)
    k0, v0 = st.kcache.clone(), st.vcache.clone()
    xs = _x((2, T, H), dtype, 32).to(DEV)
    _, al, hs = eng.append(st, xs, all_logits=True, hidden_states=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(al).all())
    for b, p in enumerate(live):
        for now, old, name in ((st.kcache, k0, "k"), (st.vcache, v0, "v")):
            assert torch.equal(_bits(now[:, b, :, :p]), _bits(old[:, b, :, :p])), f"{name} rows [0, {p}) of row {b} changed"
            assert bool((_bits(now[:, b, :, p + T:]) == sentinel).all()), f"{name} rows >= {p + T} of row {b} written"
            assert bool(torch.isfinite(now[:, b, :, p:p + T]).all()), f"{name} rows [{p}, {p + T}) of row {b} not all written"
    if dtype == F32:
        pos0 = torch.tensor(live, dtype=torch.int32, device=DEV)
        for i in range(cfg.layers):
            h = ops.rmsnorm(hs[i].reshape(2 * T, H).contiguous(), eng.w.llm_t["attn_norm"][i], cfg.rms_eps)
            qkv = ops.gemm(h, eng.w.llm_t["wqkv"][i])
            kc = torch.zeros((2, cfg.kv_heads, 64, cfg.head_dim), device=DEV, dtype=dtype)
            vc = torch.zeros_like(kc)
            ops.rope_kv_append(qkv, kc, vc, eng.w.rope_cos, eng.w.rope_sin, 2, T, cfg.heads, cfg.kv_heads, cfg.head_dim, pos0=pos0)
            for b, p in enumerate(live):
                assert torch.equal(st.kcache[i, b, :, p:p + T], kc[b, :, p:p + T]), f"layer {i} row {b}: appended k rows"
                assert torch.equal(st.vcache[i, b, :, p:p + T], vc[b, :, p:p + T]), f"layer {i} row {b}: appended v rows"


# ------------------------------------------------------------------------------------------------ 5. a stale host bound
def test_a_position_beyond_the_hosts_bound_raises_the_error_word_and_stays_inside_the_cache():
    """device pos[0] = h_pos_max + 1 (written by hand; h_pos_max + 1 + T <= max_pos, so nothing here can leave the allocation): the
    call returns OK, srgpt_llm_decode_sync_state reports SRGPT_ERR_STATE, row 0's live cache rows keep their bits -- and the word is
    sticky across a later, valid append"""
    lib, L, ops = _lib()
    _, _, eng = _setup(F32)
    P, T = 20, 5
    st = eng.new_state(2, 64, 2)
    st.kcache.fill_(float("nan"))
    st.vcache.fill_(float("nan"))
    eng.prefill(_x((2, P, H), F32, 41).to(DEV), max_new=1, state=st)
    assert lib.srgpt_llm_decode_sync_state(C.byref(eng.w.llm), C.byref(st.c), ops._stream()) == 0
    k0, v0 = st.kcache.clone(), st.vcache.clone()
    st.pos.copy_(torch.tensor([P + 1, P], dtype=torch.int32))
    assert P + 1 + T <= st.max_pos
    rc, al, _ = _prefill_append(eng, st, _x((2, T, H), F32, 42).to(DEV), T, None, P)
    assert rc == 0
    assert lib.srgpt_llm_decode_sync_state(C.byref(eng.w.llm), C.byref(st.c), ops._stream()) == L.ERR_STATE
    assert b"srgpt_llm_prefill_append" in lib.srgpt_last_error()
    for now, old in ((st.kcache, k0), (st.vcache, v0)):
        assert torch.equal(_bits(now[:, 0, :, :P + 1]), _bits(old[:, 0, :, :P + 1])), "row 0's live cache rows changed"
        assert torch.equal(_bits(now[:, :, :, P + 1 + T:]), _bits(old[:, :, :, P + 1 + T:])), "rows behind every segment changed"
    assert 0 <= int(st.pos[0]) <= st.max_pos and int(st.pos[1]) == P + T
    # a bad length raises it too (fresh word: a prefill clears it), and a valid append afterwards does not clear it
    eng.prefill(_x((2, P, H), F32, 41).to(DEV), max_new=1, state=st)
    assert lib.srgpt_llm_decode_sync_state(C.byref(eng.w.llm), C.byref(st.c), ops._stream()) == 0
    rc, _, _ = _prefill_append(eng, st, _x((2, T, H), F32, 42).to(DEV), T, torch.tensor([T + 1, 2], dtype=torch.int32, device=DEV), P)
    assert rc == 0 and lib.srgpt_llm_decode_sync_state(C.byref(eng.w.llm), C.byref(st.c), ops._stream()) == L.ERR_STATE
    assert st.pos.tolist() == [P + T, P + 2]
    rc, _, _ = _prefill_append(eng, st, _x((2, T, H), F32, 43).to(DEV), T, None, P + T)
    assert rc == 0 and lib.srgpt_llm_decode_sync_state(C.byref(eng.w.llm), C.byref(st.c), ops._stream()) == L.ERR_STATE


# ------------------------------------------------------------------------------------------------ 6. fp8 formats
def test_append_w8a16_vs_oracle_on_dequantised_weights():
    """W8A16: the reference and bar of tests/test_gpu_pipeline.py::test_fp8_weight_decode_vs_oracle_on_dequantised_weights -- the
    oracle on dequant(quant(W)), 3e-2 x max |logits|"""
    _split_case(BF16, "fp8", 20, 17, 3e-2)


def test_append_w8a8_vs_the_oracles_restatement():
    """W8A8: the reference and bar of tests/test_gpu_fp8_mfma.py::test_w8a8_prefill_vs_oracle_restatement -- so.llama_forward on the
    dequantised weights with act_quant = so.fp8_rowwise_fake_quant in front of the layer projections (per-token, so cutting the
    sequence changes no row), 3e-2 x max |reference logits|; the decode steps after it are W8A16, as there"""
    _split_case(BF16, "fp8_w8a8", 20, 17, 3e-2, act_quant=True)


# ------------------------------------------------------------------------------------------------ 7. steps after an append
def test_graph_replays_equal_eager_steps_after_an_append():
    """a state that has already decoded (its embedded-token record names a token) is appended to, then srgpt_llm_sample_first and 4
    graph replays against 4 eager srgpt_llm_decode_steps from an identical state: ids and st.logits bit for bit"""
    lib, L, ops = _lib()
    _, _, eng = _setup(F32)
    x = _x((1, 37, H), F32, 51).to(DEV)
    res = []
    eng.stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(eng.stream):
        for graph in (True, False):
            st = eng.new_state(1, 128, 8)
            eng.prefill(x[:, :20], max_new=8, state=st)
            L.check(lib.srgpt_llm_sample_first(C.byref(eng.w.llm), C.byref(st.c), ops._stream()))
            L.check(lib.srgpt_llm_decode_step(C.byref(eng.w.llm), C.byref(st.c), ops._stream()))
            st.host_len = [21]
            eng.append(st, x[:, 20:])
            L.check(lib.srgpt_llm_sample_first(C.byref(eng.w.llm), C.byref(st.c), ops._stream()))
            if graph:
                L.check(lib.srgpt_graph_launch(st.ensure_graph(), 4, ops._stream()))
            else:
                for _ in range(4):
                    L.check(lib.srgpt_llm_decode_step(C.byref(eng.w.llm), C.byref(st.c), ops._stream()))
            torch.cuda.synchronize()
            assert lib.srgpt_llm_decode_sync_state(C.byref(eng.w.llm), C.byref(st.c), ops._stream()) == 0
            assert int(st.pos[0]) == 21 + 17 + 4 and int(st.step[0]) == 5
            res.append((st.out_ids[:, :5].clone(), st.logits.clone()))
    torch.cuda.current_stream().wait_stream(eng.stream)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
