"""srgpt_attention_append -- causal attention of new query rows over a live cache, every batch row at a query position of its own --
straight at the C ABI, on both kernel families (the MFMA flash kernel: bf16, head_dim % 8 == 0; the one-wave kernel: fp32 and odd
head widths), against a float64 softmax written here.  K / V are read through CACHE strides (k_ts = D, k_hs = max_pos * D), every
key at or behind kv_len[b] is NaN (the one-wave kernel would return it; the flash kernel reads such rows as zeros through its buffer
descriptors, so there a wrong length shows as a wrong finite value), and the output sits between guard rows that must keep their
bits.  Shapes: the smallest at which the 64-row query block and the 64-key tile can go wrong.  Tolerance: tests/test_gpu_kernels.py's
`_tol` for the same operation.  And the contract that ties the new path to the recorded bits of tests/test_gpu_attn_kat.py: with
q_pos0[b] = Tk - Tq in every row the output IS srgpt_attention(causal = 1)'s, bit for bit."""
import math

import pytest
import torch

from tests.test_gpu_attention_ragged import _bits, _close
from tests.test_gpu_kernels import DEV, _ops, _rand, _tol

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
MAX_POS = 384
B = 3
FAMILIES = [  # (dtype, D, Hq, Hkv)
    pytest.param(BF16, 128, 8, 2, id="flash-d128"),
    pytest.param(BF16, 64, 4, 4, id="flash-d64"),
    pytest.param(F32, 16, 4, 2, id="one-wave-fp32"),
    pytest.param(BF16, 20, 2, 2, id="one-wave-bf16-d20"),
]
Q_POS0 = ([0, 0, 0], [63, 64, 65], [1, 130, 200])
GUARD = 2  # query rows of guard in front of and behind the output


def _ref64(q, kc, vc, q_pos0, kv_len, Tk):
    """float64 softmax(q k^T / sqrt(D)) v per batch row: key s visible to query t iff s <= q_pos0[b] + t and s < min(kv_len[b], Tk);
    q [B, Tq, Hq, D], kc / vc [B, Hkv, max_pos, D] -> [B, Tq, Hq, D] (a query with no visible key: zeros)"""
    nb, Tq, Hq, D = q.shape
    Hkv = kc.shape[1]
    out = torch.zeros((nb, Tq, Hq, D), dtype=torch.float64)
    for b in range(nb):
        n = min(kv_len[b], Tk)
        if n <= 0:
            continue
        qd = q[b].double().transpose(0, 1)                              # [Hq, Tq, D]
        kd = kc[b, :, :n].double().repeat_interleave(Hq // Hkv, 0)      # [Hq, n, D]
        vd = vc[b, :, :n].double().repeat_interleave(Hq // Hkv, 0)
        mask = torch.arange(n)[None, :] <= (q_pos0[b] + torch.arange(Tq))[:, None]
        s = (qd @ kd.transpose(-1, -2) / math.sqrt(D)).masked_fill(~mask[None], float("-inf"))
        out[b] = (s.softmax(-1) @ vd).transpose(0, 1)
    return out


def _launch(q, kc, vc, q_pos0, kv_len, Tk):
    """one srgpt_attention_append call through the C ABI: q [B, Tq, Hq, D] (host), kc / vc [B, Hkv, max_pos, D] (device caches)
    -> the output [B, Tq, Hq, D] on the host; its guard rows are checked here"""
    ops, L = _ops()
    nb, Tq, Hq, D = q.shape
    Hkv, max_pos = kc.shape[1], kc.shape[2]
    qd = q.to(DEV).contiguous()
    buf = torch.full((nb * Tq + 2 * GUARD, Hq, D), 7.25, dtype=q.dtype, device=DEV)
    o = buf[GUARD:GUARD + nb * Tq]
    p0 = torch.tensor(q_pos0, dtype=torch.int32, device=DEV)
    kl = None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32, device=DEV)
    L.check(L.load().srgpt_attention_append(
        qd.data_ptr(), kc.data_ptr(), vc.data_ptr(), o.data_ptr(), nb, Tq, Tk, Hq, Hkv, D, Tq * Hq * D, Hq * D, D,
        Hkv * max_pos * D, D, max_pos * D, Hkv * max_pos * D, D, max_pos * D, 1.0 / math.sqrt(D), p0.data_ptr(),
        None if kl is None else kl.data_ptr(), ops.dt_code(qd), ops._stream()))
    torch.cuda.synchronize()
    guard = torch.cat([buf[:GUARD], buf[GUARD + nb * Tq:]])
    assert bool((guard == 7.25).all()), "srgpt_attention_append wrote outside o[B, Tq, Hq, D]"
    return o.reshape(nb, Tq, Hq, D).cpu()


def _case(dtype, D, Hq, Hkv, Tq, q_pos0, lens, seed):
    """row b appends lens[b] <= Tq rows at q_pos0[b]: kv_len[b] = q_pos0[b] + lens[b], Tk = the host's bound max(q_pos0) + Tq"""
    Tk = max(q_pos0) + Tq
    assert Tk <= MAX_POS
    kv_len = [p + n for p, n in zip(q_pos0, lens)]
    q = _rand((B, Tq, Hq, D), dtype, seed)
    kc = _rand((B, Hkv, MAX_POS, D), dtype, seed + 1)
    vc = _rand((B, Hkv, MAX_POS, D), dtype, seed + 2)
    kd, vd = kc.clone(), vc.clone()
    for b, n in enumerate(kv_len):
        kd[b, :, n:] = float("nan")
        vd[b, :, n:] = float("nan")
    ref = _ref64(q, kc, vc, q_pos0, kv_len, Tk)
    out = _launch(q, kd.to(DEV), vd.to(DEV), q_pos0, kv_len, Tk)
    tol = _tol(ref, dtype)
    for b, n in enumerate(lens):  # padded queries (t >= lens[b]) are unspecified
        _close(out[b, :n], ref[b, :n], tol, f"attention_append {dtype} D{D} Hq{Hq} Hkv{Hkv} Tq{Tq} q_pos0{q_pos0} lens{lens} row {b}")


@pytest.mark.parametrize("Tq", [1, 17, 64, 65, 130])
@pytest.mark.parametrize("dtype,D,Hq,Hkv", FAMILIES)
def test_attention_append_full_segments(dtype, D, Hq, Hkv, Tq):
    for i, q_pos0 in enumerate(Q_POS0):
        _case(dtype, D, Hq, Hkv, Tq, q_pos0, [Tq] * B, seed=700 + 10 * i)


@pytest.mark.parametrize("Tq,lens", [(65, [65, 1, 33]), (130, [64, 130, 65]), (17, [1, 17, 16])])
@pytest.mark.parametrize("dtype,D,Hq,Hkv", FAMILIES)
def test_attention_append_ragged_segments(dtype, D, Hq, Hkv, Tq, lens):
    for i, q_pos0 in enumerate(Q_POS0):
        _case(dtype, D, Hq, Hkv, Tq, q_pos0, lens, seed=800 + 10 * i)


def test_attention_append_null_kv_len_means_tk():
    """kv_len = NULL: every row sees min(q_pos0[b] + t + 1, Tk) keys -- rows whose segment ends before the bound read on up to it"""
    for dtype, D, Hq, Hkv in ((BF16, 64, 4, 4), (F32, 16, 4, 2)):
        Tq, q_pos0 = 65, [63, 64, 65]
        Tk = max(q_pos0) + Tq
        q, kc, vc = _rand((B, Tq, Hq, D), dtype, 900), _rand((B, Hkv, MAX_POS, D), dtype, 901), _rand((B, Hkv, MAX_POS, D), dtype, 902)
        kd, vd = kc.clone(), vc.clone()
        kd[:, :, Tk:] = float("nan")
        vd[:, :, Tk:] = float("nan")
        ref = _ref64(q, kc, vc, q_pos0, [Tk] * B, Tk)
        _close(_launch(q, kd.to(DEV), vd.to(DEV), q_pos0, None, Tk), ref, _tol(ref, dtype), f"attention_append kv_len NULL {dtype}")


def test_attention_append_query_without_visible_key_yields_zeros():
    """kv_len[b] = 0: no key of the row is visible -> exact zeros, on both families"""
    for dtype, D, Hq, Hkv in ((BF16, 64, 4, 4), (F32, 16, 4, 2), (BF16, 20, 2, 2)):
        q = _rand((B, 17, Hq, D), dtype, 910)
        kc = torch.full((B, Hkv, MAX_POS, D), float("nan"), dtype=dtype)
        out = _launch(q, kc.to(DEV), kc.to(DEV), [0, 5, 70], [0, 0, 0], 87)
        assert bool((out == 0).all()), (dtype, D)


@pytest.mark.parametrize("Tq,Tk", [(17, 147), (65, 130)])
@pytest.mark.parametrize("dtype,D,Hq,Hkv", FAMILIES)
def test_uniform_offset_equals_srgpt_attention_bit_for_bit(dtype, D, Hq, Hkv, Tq, Tk):
    """q_pos0[b] = Tk - Tq for every row and the same kv_len: srgpt_attention(causal = 1) to the last bit (no kv_len, and ragged)"""
    ops, L = _ops()
    q = _rand((B, Tq, Hq, D), dtype, 920).to(DEV)
    kc = _rand((B, Hkv, MAX_POS, D), dtype, 921).to(DEV)
    vc = _rand((B, Hkv, MAX_POS, D), dtype, 922).to(DEV)
    k, v = kc.transpose(1, 2)[:, :Tk], vc.transpose(1, 2)[:, :Tk]  # [B, Tk, Hkv, D] views with the cache strides
    assert k.stride() == (Hkv * MAX_POS * D, D, MAX_POS * D, 1)
    p0 = torch.full((B,), Tk - Tq, dtype=torch.int32, device=DEV)
    for lens in (None, [Tk, Tk - Tq + 1, 70]):
        kl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
        want = ops.attention(q, k, v, causal=True, kv_len=kl)
        got = ops.attention_append(q, k, v, p0, kv_len=kl)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(want)), (dtype, D, Tq, Tk, lens)
