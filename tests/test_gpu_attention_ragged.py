"""The attention kernels under PER-ROW lengths: srgpt_decode_attention with a different pos[b] in every row of one launch (the rows
then differ in their live-split count, their merge, the block that appends), srgpt_attention with kv_len[b] (alone and together with
the causal mask, on the MFMA flash kernel and on the one-wave kernel), srgpt_rope_kv_append with per-row pos0 -- each straight at the
kernel through the C ABI, against a float64 reference computed on the CPU from the dtype-rounded inputs.  Everything a row must not
read (cache rows at or behind its position, keys behind its length, the partials of the workspace) is NaN, and whatever the kernel
returns must be finite before it is compared (`_close`); everything a launch must not write is compared bit for bit with what was
there before.  Tolerances: tests/test_gpu_kernels.py's `_tol` for the same operations."""
import math

import pytest
import torch

from tests.test_gpu_kernels import DEV, _ops, _rand, _tol
from tests.util import assert_close

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


def _close(got, ref, atol, what):
    """tests/util.assert_close, which a NaN passes (`err > tol` is False for it): the poison this file plants shows up as a NaN in
    what the kernel returns, so everything compared has to be finite first"""
    bad = ~torch.isfinite(got.detach().float())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} elements are not finite (poison read, or a row never written)"
    assert_close(got, ref, atol, 0, what)


def _bits(t):
    """the tensor's bits as integers (NaN poison compares equal to itself)"""
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _rope_tables(Hq, Hkv, D, max_pos, dtype):
    from spatialrgpt_amd.config import SrgptConfig as PC
    from spatialrgpt_amd.weights import rope_tables
    return rope_tables(PC(hidden=Hq * D, heads=Hq, kv_heads=Hkv, rope_theta=10000.0), max_pos, dtype, DEV)


def _oracle_rope(x, positions, Hq, Hkv, dtype):
    """x [B, T, H, D] at positions [B, T] through the oracle's rotary (in `dtype`, every intermediate rounded) -> [B, H, T, D]"""
    from oracle import srgpt_oracle as so
    cfg = so.SrgptConfig(hidden=Hq * x.shape[-1], heads=Hq, kv_heads=Hkv, rope_theta=10000.0)
    c, s = so.rope_cos_sin(cfg, positions, dtype)
    xt = x.transpose(1, 2)
    return so.apply_rope(xt, xt, c, s)[0]


# ------------------------------------------------------------------------------------------------ 1. decode attention, ragged pos
def _decode_ragged_case(dtype, Hq, Hkv, D, max_pos, pos_list, steps, seed=300):
    """`steps` decode launches of one batch whose row b has pos_list[b] tokens cached, ONE workspace for all of them (its tickets
    zeroed once), pos += 1 in between.  After every launch: the output against the float64 softmax over the row's own pos[b] + 1
    keys; cache row pos[b] = the oracle's rotated k / the v bits; every other cache element bit-unchanged; every ticket zero; row b
    bit-identical to row b of a launch of the same B, max_pos and workspace size whose rows are all copies of row b (same split
    count, so only per-row indexing can differ) and -- MFMA kernel, whose split count depends on max_pos only -- to the row launched
    alone."""
    ops, L = _ops()
    B, G = len(pos_list), Hq // Hkv
    pos0 = torch.tensor(pos_list, dtype=torch.int64)
    T = int(pos0.max()) + steps
    assert int(pos0.min()) >= 0 and T <= max_pos, (pos_list, steps, max_pos)  # the last launch appends row max(pos) + steps - 1
    # attn_decode_route (csrc/attn_route.h); the "ragged mfma" / "ragged valu" rows of tests/golden/attn_routes.json pin the family
    # of every parametrisation below (tests/test_host_attn_route.py)
    mfma = dtype == BF16 and D == 128 and G in (1, 2, 4, 8)
    cos_t, sin_t = _rope_tables(Hq, Hkv, D, max_pos, dtype)
    ar = torch.arange(B)

    q_raw = _rand((B, steps, Hq, D), dtype, seed)        # the new token of every launch
    k_raw = _rand((B, T, Hkv, D), dtype, seed + 1)       # token t of row b sits at position t: rows [0, pos) are the history,
    v_all = _rand((B, T, Hkv, D), dtype, seed + 2)       # rows pos + s the new tokens
    k_rot = _oracle_rope(k_raw, torch.arange(T)[None].expand(B, -1), Hq, Hkv, dtype)              # [B, Hkv, T, D]
    q_rot = _oracle_rope(q_raw, pos0[:, None] + torch.arange(steps)[None], Hq, Hkv, dtype)        # [B, Hq, steps, D]

    # the history goes into the caches on the host (not through srgpt_rope_kv_append); everything at or behind pos[b] is NaN
    kc_h = torch.full((B, Hkv, max_pos, D), float("nan"), dtype=dtype)
    vc_h = torch.full((B, Hkv, max_pos, D), float("nan"), dtype=dtype)
    for b, p in enumerate(pos_list):
        kc_h[b, :, :p] = k_rot[b, :, :p]
        vc_h[b, :, :p] = v_all[b, :p].transpose(0, 1)
    kc, vc = kc_h.to(DEV), vc_h.to(DEV)

    def workspace(nb):
        ws, tickets = ops.decode_attention_ws(nb, Hq, D, DEV)
        ws[:ws.numel() - tickets.numel()] = float("nan")  # the partials; the tickets stay zero
        return ws, tickets

    ws, tickets = workspace(B)      # the batch under test
    ws_u, tickets_u = workspace(B)  # the uniform batches (same size)
    ws_1, tickets_1 = workspace(1)

    for s in range(steps):
        pos = pos0 + s
        what = f"{dtype} Hq{Hq} Hkv{Hkv} D{D} max_pos{max_pos} pos{pos.tolist()}"
        qkv = torch.cat([q_raw[:, s].reshape(B, -1), k_raw[ar, pos].reshape(B, -1), v_all[ar, pos].reshape(B, -1)], 1).to(DEV)
        posd = pos.to(torch.int32).to(DEV)
        kc0, vc0 = kc.clone(), vc.clone()
        out = ops.decode_attention(qkv, kc, vc, posd, cos_t, sin_t, Hq, Hkv, D, ws=ws)
        torch.cuda.synchronize()

        # 1. float64 softmax over the row's own keys
        ref = torch.empty((B, Hq, D), dtype=torch.float64)
        for b in range(B):
            n = int(pos[b]) + 1
            qd = q_rot[b, :, s].double()                                            # [Hq, D]
            kd = k_rot[b, :, :n].double().repeat_interleave(G, 0)                   # [Hq, n, D]
            vd = v_all[b, :n].transpose(0, 1).double().repeat_interleave(G, 0)
            p = (torch.einsum("hd,hnd->hn", qd, kd) / math.sqrt(D)).softmax(-1)
            ref[b] = torch.einsum("hn,hnd->hd", p, vd)
        _close(out.reshape(B, Hq, D), ref, _tol(ref, dtype), "ragged decode attention " + what)
        # 2. the appended row
        pd = pos.to(DEV)
        ard = ar.to(DEV)
        _close(kc[ard, :, pd], k_rot[ar, :, pos], _tol(k_rot, dtype, 0.5), "ragged decode appended k " + what)
        assert torch.equal(_bits(vc[ard, :, pd]).cpu(), _bits(v_all[ar, pos])), "ragged decode appended v " + what
        # 3. nothing else in the caches moved
        for c_now, c_old, name in ((kc, kc0, "k"), (vc, vc0, "v")):
            c = c_now.clone()
            c[ard, :, pd] = c_old[ard, :, pd]
            assert torch.equal(_bits(c), _bits(c_old)), f"{name} cache written outside row pos[b]: " + what
        # 4. the tickets are re-armed
        assert int(torch.count_nonzero(tickets)) == 0, ("tickets", tickets.tolist(), what)
        # 5. / 6. the row in a uniform batch of the same size, and alone
        for b in range(B):
            rep = lambda t: t[b:b + 1].expand(B, *t.shape[1:]).contiguous()  # noqa: E731
            out_u = ops.decode_attention(rep(qkv), rep(kc0), rep(vc0), rep(posd), cos_t, sin_t, Hq, Hkv, D, ws=ws_u)
            assert torch.equal(_bits(out_u[b]), _bits(out[b])), f"row {b} differs from its uniform batch: " + what
            assert torch.equal(_bits(out_u), _bits(out_u[:1].expand(B, -1))), f"uniform batch of row {b}: rows differ: " + what
            assert int(torch.count_nonzero(tickets_u)) == 0, ("tickets, uniform batch", b, what)
            if mfma:
                one = lambda t: t[b:b + 1].clone()  # noqa: E731
                out_1 = ops.decode_attention(one(qkv), one(kc0), one(vc0), one(posd), cos_t, sin_t, Hq, Hkv, D, ws=ws_1)
                assert torch.equal(_bits(out_1[0]), _bits(out[b])), f"row {b} differs from the row launched alone: " + what
                assert int(torch.count_nonzero(tickets_1)) == 0, ("tickets, single row", b, what)


@pytest.mark.parametrize("Hq,Hkv,max_pos,pos,steps", [
    # a batch of 8 (BASELINE configs[4]); row 63 -> 64 goes from one live split to two between the launches, row 510 -> 511 fills the cache
    (8, 2, 512, [0, 1, 15, 16, 63, 64, 259, 510], 2),
    # 16 live splits against 17 (the merge reads partials in batches of 16), 63, 1, and 32 -> 33
    (8, 1, 4096, [1023, 1024, 4000, 5, 2047], 2),
    # beyond 64 x 64 positions: 128 keys per block, the waves loop
    (2, 2, 8192, [5000, 100, 127, 8000], 1),
    (4, 2, 1024, [700, 0, 64], 2),  # G = 2
])
def test_decode_attention_ragged_mfma(Hq, Hkv, max_pos, pos, steps):
    _decode_ragged_case(BF16, Hq, Hkv, 128, max_pos, pos, steps)


@pytest.mark.parametrize("dtype,D,Hq,Hkv,max_pos,pos,steps", [
    (F32, 128, 8, 2, 1024, [0, 300, 17, 1022], 2),
    (BF16, 64, 8, 8, 2048, [129, 2046, 0], 2),
    (F32, 16, 4, 2, 512, [0, 1, 2, 511, 255, 256], 1),  # 511 + 2 > max_pos: one launch
    (BF16, 32, 8, 1, 512, [3, 129, 77], 2),
])
def test_decode_attention_ragged_valu(dtype, D, Hq, Hkv, max_pos, pos, steps):
    _decode_ragged_case(dtype, Hq, Hkv, D, max_pos, pos, steps)


# ------------------------------------------------------------------------------------------------ 2. prefill attention, kv_len
def _attn_ref64(q, k, v, causal, lens):
    """float64 softmax(q k^T / sqrt(D) + masks) v, one batch row at a time; a query with no visible key yields zeros
    (include/srgpt.h).  -> (out [B, Tq, Hq, D], visible [B, Tq])"""
    B, Tq, Hq, D = q.shape
    Tk, Hkv = k.shape[1], k.shape[2]
    out = torch.empty((B, Tq, Hq, D), dtype=torch.float64)
    vis = torch.empty((B, Tq), dtype=torch.bool)
    for b in range(B):
        qd = q[b].double().transpose(0, 1)
        kd = k[b].double().transpose(0, 1).repeat_interleave(Hq // Hkv, 0)
        vd = v[b].double().transpose(0, 1).repeat_interleave(Hq // Hkv, 0)
        mask = torch.ones((Tq, Tk), dtype=torch.bool)
        if causal:
            mask &= torch.arange(Tk)[None, :] <= torch.arange(Tq)[:, None] + (Tk - Tq)
        if lens is not None:
            mask &= (torch.arange(Tk) < lens[b])[None, :]
        s = (qd @ kd.transpose(-1, -2) / math.sqrt(D)).masked_fill(~mask[None], float("-inf"))
        vis[b] = mask.any(-1)
        p = torch.where(vis[b][None, :, None], s.softmax(-1), torch.zeros((), dtype=torch.float64))
        out[b] = (p @ vd).transpose(0, 1)
    return out, vis


def _attn_kvlen_case(dtype, B, Tq, Tk, Hq, Hkv, D, causal, lens, seed=400):
    """srgpt_attention with kv_len = lens (None = no kv_len): K and V rows at or behind lens[b] are NaN on the device, zero (and
    masked) in the reference; EVERY query row is compared and must be finite.  The NaN can show only on the one-wave kernel: the MFMA
    flash kernel fetches K / V through buffer descriptors that end at row kv_len[b] - 1 (csrc/flash.hip), so a row behind the length
    reads as zeros there whatever it holds -- on that kernel a wrong length shows as a wrong finite value (a zero key in the softmax).
    -> (out on the CPU, visible [B, Tq])"""
    ops, L = _ops()
    q, k, v = _rand((B, Tq, Hq, D), dtype, seed), _rand((B, Tk, Hkv, D), dtype, seed + 1), _rand((B, Tk, Hkv, D), dtype, seed + 2)
    kd, vd = k.clone(), v.clone()
    if lens is not None:
        assert len(lens) == B and all(0 <= n <= Tk for n in lens)
        for b, n in enumerate(lens):
            k[b, n:] = 0
            v[b, n:] = 0
            kd[b, n:] = float("nan")
            vd[b, n:] = float("nan")
    ref, vis = _attn_ref64(q, k, v, causal, lens)
    kv_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = ops.attention(q.to(DEV), kd.to(DEV), vd.to(DEV), causal=causal, kv_len=kv_len).cpu()
    _close(out, ref, _tol(ref, dtype), f"attention kv_len {dtype} B{B} Tq{Tq} Tk{Tk} Hq{Hq} Hkv{Hkv} D{D} causal{causal} {lens}")
    return out, vis


@pytest.mark.parametrize("dtype,D,Hq,Hkv,Tq,Tk,lens", [
    (BF16, 128, 4, 2, 200, 200, [200, 1, 63, 64, 65, 128, 129, 199]),  # flash: every side of the 64-key tile edges
    (BF16, 64, 8, 2, 130, 130, [130, 64, 7]),
    (BF16, 80, 2, 1, 150, 150, [150, 65]),                             # flash, head padded to 96
    (BF16, 128, 4, 2, 65, 200, [200, 137, 136]),                       # causal offset 135 together with the lengths
    (F32, 128, 2, 2, 130, 130, [130, 1, 64, 65]),                      # one-wave kernel
])
def test_attention_causal_kvlen(dtype, D, Hq, Hkv, Tq, Tk, lens):
    _attn_kvlen_case(dtype, len(lens), Tq, Tk, Hq, Hkv, D, True, lens)


def test_attention_causal_kvlen_bf16_one_wave():
    # attn_prefill_route (csrc/attn_route.h) sends bf16 to the MFMA flash kernel only when `vec_ok`, which needs D % 8 == 0;
    # head_dim 20 therefore runs simple_attn_kernel<bf16_t>, the one-wave kernel: the "ragged bf16 one-wave (head_dim 20)" row of
    # tests/golden/attn_routes.json pins that (and the "ragged ..." rows beside it the family of every other prefill case here)
    _attn_kvlen_case(BF16, 2, 70, 70, 2, 2, 20, True, [70, 3])


NOVIS = [(BF16, 64), (BF16, 20), (F32, 64)]  # flash, one-wave bf16 (D % 8 != 0, see above), one-wave fp32


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype,D", NOVIS)
def test_attention_kvlen_zero_yields_zeros(dtype, D, causal):
    """kv_len[b] = 0: no key is visible to any query of the row (all of its K and V is NaN here) -> exact zeros"""
    out, vis = _attn_kvlen_case(dtype, 2, 70, 70, 4, 2, D, causal, [0, 40])
    assert not bool(vis[0].any()) and bool(vis[1].all())
    assert bool((out[0] == 0).all()), out[0]


@pytest.mark.parametrize("dtype,D", NOVIS)
def test_attention_causal_rows_before_the_first_key_yield_zeros(dtype, D):
    """causal with Tq = 70 > Tk = 40: key s is visible to query t iff s <= t - 30, so queries 0 .. 29 see nothing -> exact zeros"""
    out, vis = _attn_kvlen_case(dtype, 2, 70, 40, 4, 2, D, True, None)
    assert vis[0].tolist() == [False] * 30 + [True] * 40
    assert bool((out[:, :30] == 0).all()), out[:, :30]


# ------------------------------------------------------------------------------------------------ 3. rope + append, per-row pos0
@pytest.mark.parametrize("dtype,B,T,Hq,Hkv,D,max_pos,pos0", [
    (BF16, 3, 37, 8, 2, 128, 256, [0, 100, 219]),  # the last row ends exactly at the cache's end
    (F32, 2, 5, 4, 2, 16, 64, [7, 0]),
])
def test_rope_kv_append_per_row_pos0_vs_oracle(dtype, B, T, Hq, Hkv, D, max_pos, pos0):
    ops, L = _ops()
    assert max(pos0) + T <= max_pos
    cos_t, sin_t = _rope_tables(Hq, Hkv, D, max_pos, dtype)
    qkv = _rand((B, T, (Hq + 2 * Hkv) * D), dtype, 500)
    q_raw = qkv[..., :Hq * D].reshape(B, T, Hq, D)
    k_raw = qkv[..., Hq * D:(Hq + Hkv) * D].reshape(B, T, Hkv, D)
    v_raw = qkv[..., (Hq + Hkv) * D:].reshape(B, T, Hkv, D)
    positions = torch.tensor(pos0)[:, None] + torch.arange(T)[None]
    q_rot = _oracle_rope(q_raw, positions, Hq, Hkv, dtype)  # [B, Hq, T, D]
    k_rot = _oracle_rope(k_raw, positions, Hq, Hkv, dtype)
    kc = torch.full((B, Hkv, max_pos, D), float("nan"), dtype=dtype, device=DEV)
    vc = torch.full((B, Hkv, max_pos, D), float("nan"), dtype=dtype, device=DEV)
    kc0, vc0 = kc.clone(), vc.clone()
    g = qkv.reshape(B * T, -1).to(DEV)
    ops.rope_kv_append(g, kc, vc, cos_t, sin_t, B, T, Hq, Hkv, D, pos0=torch.tensor(pos0, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    _close(g[:, :Hq * D].reshape(B, T, Hq, D), q_rot.transpose(1, 2), _tol(q_rot, dtype, 0.5), "rope q, per-row pos0")
    for b, p in enumerate(pos0):
        _close(kc[b, :, p:p + T], k_rot[b], _tol(k_rot, dtype, 0.5), f"rope k -> cache rows [{p}, {p + T}) of row {b}")
        assert torch.equal(_bits(vc[b, :, p:p + T]).cpu(), _bits(v_raw[b].transpose(0, 1).contiguous())), f"v -> cache, row {b}"
        kc[b, :, p:p + T] = kc0[b, :, p:p + T]
        vc[b, :, p:p + T] = vc0[b, :, p:p + T]
    assert torch.equal(_bits(kc), _bits(kc0)), "k cache written outside [pos0[b], pos0[b] + T)"
    assert torch.equal(_bits(vc), _bits(vc0)), "v cache written outside [pos0[b], pos0[b] + T)"
