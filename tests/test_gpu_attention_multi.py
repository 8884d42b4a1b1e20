"""srgpt_decode_attention_multi at the C ABI: T new tokens per sequence in one launch.

MFMA route (bf16, head_dim 128): output row t must equal, BIT FOR BIT, what srgpt_decode_attention returns for token t's raw q / k / v
at position pos + t over a cache that already holds the roped rows before it -- the comparison cache is built by running the
single-token kernel t times -- and the cache rows pos .. pos + T - 1 must equal the single-token kernel's appends.  `pos` straddles a
16-key wave group, a 64-key split and (max_pos 8192) a 128-key block, so columns meet groups, waves and whole splits in which they see
no key.  Everything around the operands is NaN or a sentinel; the tickets are zero after each launch.

Composed route (fp32, other head widths): against a float64 reference, with the tolerances tests/test_gpu_attention_ragged.py uses."""
import math

import pytest
import torch

from tests.test_gpu_attention_ragged import _bits, _close, _oracle_rope, _rope_tables
from tests.test_gpu_kernels import DEV, _ops, _rand, _tol
from tests.util import check_guarded, guarded, poisoned

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
D = 128
PAD = 32  # NaN rows in front of and behind a cache


def _caches(B, Hkv, max_pos, pos_list, seed, dtype=BF16, d=D):
    """k / v caches inside larger NaN allocations: rows below pos[b] hold random values (they stand for roped history rows: both
    kernels read them as they are), every other row is NaN -> (k_big, k, v_big, v)"""
    out = []
    for i in range(2):
        big = torch.full((B * Hkv * max_pos + 2 * PAD, d), float("nan"), dtype=dtype)
        view = big[PAD:PAD + B * Hkv * max_pos].view(B, Hkv, max_pos, d)
        for b, p in enumerate(pos_list):
            if 0 < p <= max_pos:
                view[b, :, :p] = _rand((Hkv, p, d), dtype, seed + 10 * i + b)
        big = big.to(DEV)
        out += [big, big[PAD:PAD + B * Hkv * max_pos].view(B, Hkv, max_pos, d)]
    return out


def _multi_vs_single(G, T, pos_list, max_pos, Hkv=2, seed=900):
    ops, L = _ops()
    B, Hq = len(pos_list), G * Hkv
    QW = (Hq + 2 * Hkv) * D
    what = f"G{G} T{T} pos{pos_list} max_pos{max_pos}"
    assert all(0 <= p and p + T <= max_pos for p in pos_list)
    cos_t, sin_t = _rope_tables(Hq, Hkv, D, max_pos, BF16)
    qkv_h = _rand((B * T, QW), BF16, seed)
    qkv = poisoned(qkv_h).view(B, T, QW)
    pos = torch.tensor(pos_list, dtype=torch.int32, device=DEV)
    kb_m, kc_m, vb_m, vc_m = _caches(B, Hkv, max_pos, pos_list, seed + 1)
    kb_s, kc_s, vb_s, vc_s = kb_m.clone(), None, vb_m.clone(), None
    kc_s = kb_s[PAD:PAD + B * Hkv * max_pos].view(B, Hkv, max_pos, D)
    vc_s = vb_s[PAD:PAD + B * Hkv * max_pos].view(B, Hkv, max_pos, D)

    # the single-token kernel, T launches: token t at pos + t over the rows the launches before it appended
    ws_s, tickets_s = ops.decode_attention_ws(B, Hq, D, DEV)
    ref = torch.empty((B, T, Hq * D), dtype=BF16, device=DEV)
    for t in range(T):
        ref[:, t] = ops.decode_attention(qkv[:, t].contiguous(), kc_s, vc_s, pos + t, cos_t, sin_t, Hq, Hkv, D, ws=ws_s)
    assert bool(torch.isfinite(ref.float()).all()), what

    ws, tickets = ops.decode_attention_multi_ws(B, T, Hq, D, DEV)
    ws[:ws.numel() - tickets.numel()] = float("nan")  # the partials; the tickets stay zero
    buf, view = guarded(B * T, Hq * D, Hq * D, BF16, row0=1)
    assert view.is_contiguous()
    for launch in range(2):  # the second launch runs over the re-armed tickets (and over its own appended rows: the same bits)
        ops.decode_attention_multi(qkv, kc_m, vc_m, pos, cos_t, sin_t, Hq, Hkv, D, ws=ws, out=view.view(B, T, Hq * D))
        torch.cuda.synchronize()
        assert int(torch.count_nonzero(tickets)) == 0, ("tickets", tickets.tolist(), what)
        got = view.clone().view(B, T, Hq * D)
        for t in range(T):
            assert torch.equal(_bits(got[:, t]), _bits(ref[:, t])), f"row {t} differs from the single-token kernel at pos + {t}: " + what
        # the caches, guard rows included: the T appended rows equal the single-token kernel's, nothing else moved
        assert torch.equal(_bits(kb_m), _bits(kb_s)), "k cache: " + what
        assert torch.equal(_bits(vb_m), _bits(vb_s)), "v cache: " + what
    check_guarded(buf, view, ref.view(B * T, Hq * D), what)
    assert torch.equal(_bits(qkv.reshape(B * T, QW)).cpu(), _bits(qkv_h)), "qkv is only read on the MFMA route: " + what


POS_PAIRS = [(1, 300), (15, 127), (16, 65), (61, 64), (62, 63)]  # every pos of the issue, two different ones per launch


@pytest.mark.parametrize("max_pos", [384, 8192])
@pytest.mark.parametrize("pos", POS_PAIRS)
@pytest.mark.parametrize("G,T", [(4, 2), (4, 4), (1, 16), (8, 2)])
def test_multi_equals_single_token_kernel_bit_for_bit(G, T, pos, max_pos):
    _multi_vs_single(G, T, list(pos), max_pos)


def test_multi_bits_do_not_depend_on_max_pos():
    """the key ranges depend on pos only: a pooled cache of 4096 positions answers with the bits of one of 384"""
    ops, L = _ops()
    G, T, Hkv, pos_list = 4, 4, 2, [300, 62]
    Hq, B = G * Hkv, 2
    qkv = _rand((B, T, (Hq + 2 * Hkv) * D), BF16, 77).to(DEV)
    pos = torch.tensor(pos_list, dtype=torch.int32, device=DEV)
    outs = []
    for max_pos in (384, 4096):
        cos_t, sin_t = _rope_tables(Hq, Hkv, D, max_pos, BF16)
        _, kc, _, vc = _caches(B, Hkv, max_pos, pos_list, 78)
        outs.append(ops.decode_attention_multi(qkv, kc, vc, pos, cos_t, sin_t, Hq, Hkv, D))
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


def test_multi_rows_beyond_the_cache_are_neither_appended_nor_attended():
    """pos + T > max_pos, pos >= max_pos, pos < 0: only rows inside the cache are written -- with the single-token kernel's bits --,
    the rows that exist are attended as usual, nothing outside the caches or the output changes, the tickets are zero"""
    ops, L = _ops()
    G, T, Hkv, max_pos = 4, 4, 2, 128
    Hq = G * Hkv
    QW = (Hq + 2 * Hkv) * D
    pos_list = [max_pos - 2, max_pos + 5, -3, max_pos - 1]
    B = len(pos_list)
    cos_t, sin_t = _rope_tables(Hq, Hkv, D, max_pos, BF16)
    qkv = poisoned(_rand((B * T, QW), BF16, 31)).view(B, T, QW)
    pos = torch.tensor(pos_list, dtype=torch.int32, device=DEV)
    kb_m, kc_m, vb_m, vc_m = _caches(B, Hkv, max_pos, [min(max(p, 0), max_pos) for p in pos_list], 32)
    kb_s, vb_s = kb_m.clone(), vb_m.clone()
    kc_s = kb_s[PAD:PAD + B * Hkv * max_pos].view(B, Hkv, max_pos, D)
    vc_s = vb_s[PAD:PAD + B * Hkv * max_pos].view(B, Hkv, max_pos, D)
    live = {0: 2, 3: 1}  # sequence -> tokens whose rows exist
    ref = {}
    for b, n in live.items():
        ws_s, _ = ops.decode_attention_ws(1, Hq, D, DEV)
        for t in range(n):
            p = torch.tensor([pos_list[b] + t], dtype=torch.int32, device=DEV)
            ref[b, t] = ops.decode_attention(qkv[b:b + 1, t].contiguous(), kc_s[b:b + 1], vc_s[b:b + 1], p, cos_t, sin_t, Hq, Hkv, D, ws=ws_s)[0]
    ws, tickets = ops.decode_attention_multi_ws(B, T, Hq, D, DEV)
    buf, view = guarded(B * T, Hq * D, Hq * D, BF16, row0=1)
    ops.decode_attention_multi(qkv, kc_m, vc_m, pos, cos_t, sin_t, Hq, Hkv, D, ws=ws, out=view.view(B, T, Hq * D))
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(tickets)) == 0
    assert torch.equal(_bits(kb_m), _bits(kb_s)) and torch.equal(_bits(vb_m), _bits(vb_s))
    got = view.clone().view(B, T, Hq * D)
    for (b, t), r in ref.items():
        assert torch.equal(_bits(got[b, t]), _bits(r)), (b, t)
    idt, bits = torch.int16, 0x5A5A
    view.view(idt).fill_(bits)
    assert bool((buf.view(idt) == bits).all()), "written outside out"


# ------------------------------------------------------------------------------------------------ the composed route
@pytest.mark.parametrize("dtype,d,Hq,Hkv,T,max_pos,pos_list", [
    (F32, 16, 4, 2, 3, 64, [0, 5, 61]),        # the tiny goldens' geometry; the last row ends exactly at the cache's end
    (F32, 128, 8, 2, 4, 512, [300, 63]),       # fp32 at the LLM head width: no MFMA kernel
    (BF16, 64, 8, 8, 5, 256, [129, 3]),        # bf16 off head_dim 128
    (BF16, 128, 6, 2, 2, 256, [64, 200]),      # bf16, head_dim 128, but a group of 3: not an instance of the MFMA kernel
])
def test_multi_composed_route_vs_float64(dtype, d, Hq, Hkv, T, max_pos, pos_list):
    ops, L = _ops()
    B, G = len(pos_list), Hq // Hkv
    what = f"{dtype} D{d} Hq{Hq} Hkv{Hkv} T{T} pos{pos_list}"
    pos0 = torch.tensor(pos_list, dtype=torch.int64)
    N = int(pos0.max()) + T
    assert N <= max_pos
    cos_t, sin_t = _rope_tables(Hq, Hkv, d, max_pos, dtype)
    q_raw = _rand((B, T, Hq, d), dtype, 600)
    k_raw = _rand((B, N, Hkv, d), dtype, 601)  # token n of row b sits at position n
    v_all = _rand((B, N, Hkv, d), dtype, 602)
    k_rot = _oracle_rope(k_raw, torch.arange(N)[None].expand(B, -1), Hq, Hkv, dtype)       # [B, Hkv, N, d]
    q_rot = _oracle_rope(q_raw, pos0[:, None] + torch.arange(T)[None], Hq, Hkv, dtype)     # [B, Hq, T, d]
    kc_h = torch.full((B, Hkv, max_pos, d), float("nan"), dtype=dtype)
    vc_h = torch.full((B, Hkv, max_pos, d), float("nan"), dtype=dtype)
    for b, p in enumerate(pos_list):
        kc_h[b, :, :p] = k_rot[b, :, :p]
        vc_h[b, :, :p] = v_all[b, :p].transpose(0, 1)
    kc, vc = kc_h.to(DEV), vc_h.to(DEV)
    new = torch.stack([torch.arange(p, p + T) for p in pos_list])                            # [B, T]
    ar = torch.arange(B)[:, None]
    qkv = torch.cat([q_raw.reshape(B, T, -1), k_raw[ar, new].reshape(B, T, -1), v_all[ar, new].reshape(B, T, -1)], 2).to(DEV)
    kc0, vc0 = kc.clone(), vc.clone()
    out = ops.decode_attention_multi(qkv, kc, vc, pos0.to(torch.int32).to(DEV), cos_t, sin_t, Hq, Hkv, d)
    torch.cuda.synchronize()
    ref = torch.empty((B, T, Hq, d), dtype=torch.float64)
    for b, p in enumerate(pos_list):
        for t in range(T):
            n = p + t + 1
            kd = k_rot[b, :, :n].double().repeat_interleave(G, 0)
            vd = v_all[b, :n].transpose(0, 1).double().repeat_interleave(G, 0)
            pr = (torch.einsum("hd,hnd->hn", q_rot[b, :, t].double(), kd) / math.sqrt(d)).softmax(-1)
            ref[b, t] = torch.einsum("hn,hnd->hd", pr, vd)
    _close(out.reshape(B, T, Hq, d), ref, _tol(ref, dtype), "composed multi attention " + what)
    for b, p in enumerate(pos_list):
        _close(kc[b, :, p:p + T], k_rot[b, :, p:p + T], _tol(k_rot, dtype, 0.5), "appended k " + what)
        assert torch.equal(_bits(vc[b, :, p:p + T]).cpu(), _bits(v_all[b, p:p + T].transpose(0, 1).contiguous())), "appended v " + what
        kc[b, :, p:p + T] = kc0[b, :, p:p + T]
        vc[b, :, p:p + T] = vc0[b, :, p:p + T]
    assert torch.equal(_bits(kc), _bits(kc0)) and torch.equal(_bits(vc), _bits(vc0)), "cache written outside the T new rows: " + what
