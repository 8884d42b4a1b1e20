"""GPU: the lossless 13-bit code of bf16 weights (csrc/pack13.h) -- srgpt_pack13 / srgpt_unpack13 round trips, and srgpt_gemv_p13
against srgpt_gemv on the raw matrix, bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KS = (512, 1024, 4096, 14336)  # 14336: 28 chunk iterations = 7 groups (the whole-row batch); 512 / 1024: a padded group
FUSIONS = ("plain", "norm", "norm_swiglu", "residual", "norm_f32")


def _ops():
    from spatialrgpt_amd import ops
    return ops


def _grid():
    from spatialrgpt_amd import _lib
    return 2 * int(_lib.load().srgpt_device_cus())  # blocks of a full launch: a wave owns units u, u + 4 grid, ...


def _ns():
    g = _grid()
    # a wave's second unit and the cross-unit prefetch (4 grid + 5), a partly filled last round (4 grid - 1), third units (8 grid + 3)
    return (1, 3, 4 * g - 1, 4 * g + 5, 8 * g + 3)


_cache = {}


def _matrix(K, rows=None):
    """one gaussian matrix per K, std 0.02 like synth_state_dict, tall enough for the largest SwiGLU case (or `rows` tall), and its
    packed copy; a product over the first rows of it reads the first rows of the copy (rows are coded independently)"""
    if K not in _cache:
        ops = _ops()
        g = torch.Generator(device="cuda").manual_seed(1000 + K)
        rows = rows or 2 * max(_ns())
        w = torch.randn((rows, K), device="cuda", generator=g) * 0.02
        # the device generator returns an exact 0.0 about once in 1e7 draws (and a value below 2^-30 once in 1e8): not gaussian
        # weights but an exception row each -- those have their own cases below
        w = torch.where(w.abs() < 2.0 ** -30, torch.full_like(w, 0.02), w).to(torch.bfloat16)
        packed, flags, n_exc = ops.pack13(w)
        # the condition of every test below: nothing silently runs on the raw fallback
        assert n_exc == 0 and int((flags[:-1] == -1).sum()) == 0
        x = (torch.randn((1, K), device="cuda", generator=g) * 0.5).to(torch.bfloat16)  # x 0.5: a changed summation order would show
        nw = (1.0 + 0.1 * torch.randn((K,), device="cuda", generator=g)).to(torch.bfloat16)
        res = (torch.randn((1, rows), device="cuda", generator=g) * 0.5).to(torch.bfloat16)
        _cache[K] = (w, packed, flags, x, nw, res)
    return _cache[K]


def _plant(w):
    """exception rows: a value 2^-40 of the row maximum, a NaN, an Inf, an all-zero row -> their indices"""
    K = w.shape[1]
    w[1, K // 3] = w[1].float().abs().max().item() * 2.0 ** -40
    w[2, 0] = float("nan")
    w[w.shape[0] - 1, K - 1] = float("inf")
    w[4] = 0
    return sorted({1, 2, w.shape[0] - 1, 4})


def _both(ops, fusion, x, w, packed, flags, nw, res, N):
    kw = dict(norm_w=nw if fusion.startswith("norm") else None, eps=1e-5, residual=res[:, :N].contiguous() if fusion == "residual" else None,
              swiglu=fusion == "norm_swiglu", out_f32=fusion == "norm_f32")
    return ops.gemv(x, w, **kw), ops.gemv_p13(x, packed, flags, w, **kw)


@pytest.mark.parametrize("K", KS)
def test_pack_unpack_round_trip(K):
    ops = _ops()
    w, packed, flags, *_ = _matrix(K)
    assert packed.numel() == w.shape[0] * ((K + 2047) // 2048) * 3328 and flags.numel() == w.shape[0] + 1
    assert torch.equal(ops.unpack13(packed, flags, w).view(torch.int16), w.view(torch.int16))
    # planted exception rows: counted, flagged, and the matrix still comes back bit for bit (NaN payloads included)
    wp = w[:64].clone()
    rows = _plant(wp)
    pp, fp, n_exc = ops.pack13(wp)
    assert n_exc == len(rows) and int(fp[-1]) == len(rows)
    assert (fp[:-1] == -1).nonzero().flatten().tolist() == rows
    assert torch.equal(ops.unpack13(pp, fp, wp).view(torch.int16), wp.view(torch.int16))
    # a coded row does not depend on the raw matrix any more
    other = torch.zeros_like(wp)
    back = ops.unpack13(pp, fp, other).view(torch.int16)
    coded = [i for i in range(64) if i not in rows]
    assert torch.equal(back[coded], wp.view(torch.int16)[coded]) and int(back[rows].abs().sum()) == 0


@pytest.mark.parametrize("K", KS)
def test_gemv_p13_equals_gemv_bit_for_bit(K):
    ops = _ops()
    w, packed, flags, x, nw, res = _matrix(K)
    for N in _ns():
        for fusion in FUSIONS:
            rows = 2 * N if fusion == "norm_swiglu" else N
            ref, got = _both(ops, fusion, x, w[:rows], packed, flags, nw, res, N)
            assert ref.dtype == got.dtype and torch.equal(ref, got), (K, N, fusion, int((ref != got).sum()))


def test_gemv_p13_equals_gemv_bit_for_bit_looping_prologue():
    """K = 16896 (K % 512 == 0): 2112 activation chunks, more than the 256 * 8 the prologue's threads hold in registers -- the last 64
    are staged, squared and normalised by its loops; 33 chunk iterations = 9 groups, the last one padded with zeros in LDS"""
    ops = _ops()
    K, ns = 16896, (3, 4 * _grid() + 5)
    w, packed, flags, x, nw, res = _matrix(K, rows=max(ns))
    for N in ns:
        for fusion in ("norm", "residual"):
            ref, got = _both(ops, fusion, x, w[:N], packed, flags, nw, res, N)
            assert ref.dtype == got.dtype and torch.equal(ref, got), (K, N, fusion, int((ref != got).sum()))


@pytest.mark.parametrize("K", (512, 4096, 14336))
def test_gemv_p13_exception_rows(K):
    """planted exception rows take the raw loop inside the packed launch; a SwiGLU unit does if only its up row is one"""
    ops = _ops()
    w, _, _, x, nw, res = _matrix(K)
    for N in (3, 4 * _grid() + 5):
        for fusion in FUSIONS:
            rows = 2 * N if fusion == "norm_swiglu" else N
            wp = w[:rows].clone()
            # finite exceptions only, so that every output can be compared: a tiny value and a zero row; the last row of the matrix
            # (SwiGLU: an up row whose gate row is coded) and, where there are enough rows, the first unit of a wave's second round
            planted = {rows - 1, 1 % rows}
            if rows > 4 * _grid():
                planted.add(4 * _grid())
            for i, r in enumerate(sorted(planted)):
                if i % 2:
                    wp[r] = 0
                else:
                    wp[r, K // 2] = wp[r].float().abs().max().item() * 2.0 ** -40
            pp, fp, n_exc = ops.pack13(wp)
            assert n_exc == len(planted)
            ref, got = _both(ops, fusion, x, wp, pp, fp, nw, res, N)
            assert torch.equal(ref, got), (K, N, fusion, int((ref != got).sum()))
    # NaN / Inf rows: the same NaNs and Infs in the same places
    wp = w[:8].clone()
    wp[2, 0], wp[5, K - 1] = float("nan"), float("inf")
    pp, fp, n_exc = ops.pack13(wp)
    assert n_exc == 2
    ref, got = _both(ops, "plain", x, wp, pp, fp, nw, res, 8)
    assert torch.equal(ref.view(torch.int16), got.view(torch.int16)) and bool(ref.float().isnan().any() or ref.float().isinf().any())
