"""CPU: the data of tests/region_exact.py is what its docstring says it is, for every case of tests/test_gpu_vision_exact.py --
every exactness precondition that makes a correct kernel's output unique -- and it tells wrong kernels from the right one: the
reference recomputed under each mistake of region_exact.mutants differs from the right one in at least one element of every
non-empty mask's row (the shares are printed, and appended to SRGPT_EXACT_LOG=<file>; profiles/vision_exact.txt holds them).

Why the data exists: test_box_masks_cannot_see_the_order_of_positions.  The rectangular 0 / 1 masks of
tests/test_gpu_kernels.py::test_region_pool_true_shape_vs_oracle weigh every position inside a box alike, so a kernel that delivers the
positions of a chunk in the wrong order, or pairs a weight with a neighbouring position, returns the same sum inside the box; only
the box edges see it."""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests import region_exact as rx
from tests.util import BF16, F32, rne

SIDES = [(c, s) for c in rx.CASES for s in c.sides]
SIDE_IDS = ["%s-side%d" % (c.id, s) for c, s in SIDES]


def _log(what, kind, value):
    print("%-28s %-58s %s" % (what, kind, "n/a" if value is None else "%.4f" % value))
    path = os.environ.get("SRGPT_EXACT_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", ""), "what": what, "kind": kind, "share": value}) + "\n")


def _is_pow2(x):
    return x > 0 and math.frexp(x)[0] == 0.5


# ------------------------------------------------------------------------------------------------ region pooling
@pytest.mark.parametrize("case", rx.CASES, ids=rx.CASE_IDS)
def test_case_lies_on_the_intended_side_of_every_threshold(case):
    geo = case.geometry()
    for k, want in case.want.items():
        assert geo[k] == want, "%s (%s): %s = %r, the case exists for %r" % (case.id, case.what, k, geo[k], want)
    assert geo["full"] * geo["rows"] + geo["tail"] == case.L and case.M <= (17 if case.dtype == BF16 else rx.RP_MAXM)
    assert case.C % (8 if case.dtype == BF16 else 4) == 0
    for side in case.sides:
        assert side in (case.fw, 2 * case.fw) or 2 * side == case.fw


def test_every_threshold_has_a_case_on_either_side():
    geos = [(c, c.geometry()) for c in rx.CASES]
    mfma = [g for c, g in geos if g["kernel"] == "mfma"]
    valu = [g for c, g in geos if g["kernel"] == "valu"]
    assert {g["ch"] for g in mfma} == {1, 2, 4} and {g["mm"] for g in valu} == {8, 16}
    for fam in (mfma, valu):
        assert {min(g["psum_batches"], 2) for g in fam} == {1, 2} and {min(g["fb_rounds"], 2) for g in fam} == {1, 2}
        assert any(g["tail"] for g in fam) and any(g["full"] and not g["tail"] for g in mfma)
    # every feature x mask type at fw 27 and fw 46 (the GPU test runs every mask type at every case)
    for dtype in (BF16, F32):
        assert {27, 46} <= {c.fw for c in rx.CASES if c.dtype == dtype}


def _fp32_sum(W32, F32_, lanes, reverse):
    """sum_l W[m, l] F[l, c] in fp32: `lanes` running sums over the positions l = lane (mod lanes), forwards or backwards, then the
    lanes one after the other"""
    M, L = W32.shape
    pad = -L % lanes
    W32 = torch.cat([W32, torch.zeros((M, pad), dtype=F32)], 1)
    F32_ = torch.cat([F32_, torch.zeros((pad, F32_.shape[1]), dtype=F32)], 0)
    steps = range(0, L + pad, lanes)
    acc = torch.zeros((M, lanes, F32_.shape[1]), dtype=F32)
    for l0 in (reversed(steps) if reverse else steps):
        acc += W32[:, l0:l0 + lanes, None] * F32_[l0:l0 + lanes]
    out = torch.zeros((M, F32_.shape[1]), dtype=F32)
    for j in (range(lanes - 1, -1, -1) if reverse else range(lanes)):
        out += acc[:, j]
    return out


@pytest.mark.parametrize("case,side", SIDES, ids=SIDE_IDS)
def test_region_data_makes_the_output_unique(case, side):
    from spatialrgpt_amd.mm_utils import cv2_nearest_index
    fw, dtype = case.fw, case.dtype
    feat = rx.features(case)
    assert torch.equal(feat, feat.round()) and float(feat.abs().max()) <= 8 and torch.equal(feat.to(dtype).double(), feat)
    k = rx.mask_k(fw, side)
    S_want = 2.0 ** k * fw * fw / (side * side)
    assert _is_pow2(S_want) and 1 <= S_want <= rx.S_MAX
    sets = rx.mask_sets(case, side)
    assert len(sets) == (2 if case.M == 1 else 1) and sum(z is not None for _, z in sets) == 1  # one all-zero mask per case
    # the wrapper's rscale: exactly 1, 2 or 0.5
    sf = (case.L / (side * side)) ** 0.5
    assert 1.0 / sf in (1.0, 2.0, 0.5) and int(math.floor(side * sf)) == fw
    assert cv2_nearest_index(2 * side, side).tolist() == list(range(0, 2 * side, 2))  # what raw_u8 relies on
    for P, zero in sets:
        assert P.shape == (case.M, side, side) and torch.equal(P, P.round()) and float(P.min()) >= 0 and float(P.max()) <= 3
        live = [m for m in range(case.M) if m != zero]
        assert all(float(P[m].sum()) == 2.0 ** k for m in live) and (zero is None or float(P[zero].abs().max()) == 0)
        for mt in (BF16, F32, torch.uint8):
            assert torch.equal(P.to(mt).double(), P)
        v = rx.resampled(P, fw)
        assert torch.equal(v * 16, (v * 16).round()) and float(v.max()) <= 3 and float(v.min()) >= 0  # 1/16 units
        assert torch.equal(v.to(BF16).double(), v)
        S = v.sum(1)
        assert all(float(S[m]) == S_want for m in live), (S.tolist(), S_want)
        W, den = rx.weights(v, dtype)
        assert all(float(den[m]) == S_want for m in live)  # rnd(rnd(S) + 1e-8) = S
        assert torch.equal(W.to(BF16).double(), W) and torch.equal((v.float() / den.float()[:, None]).double(), W)
        units = (v * 16).sum(1) * 8  # the largest |sum| any subset of a mask's products can reach, in units of 2^-4 / S
        assert float(units.max()) == (128 * S_want if live else 0) and 128 * S_want < 2 ** 24
        ref64 = W @ feat
        assert bool(torch.isfinite(ref64).all())
        for lanes, reverse in ((32, False), (7, True)):
            got = _fp32_sum(W.float(), feat.float(), lanes, reverse)
            assert torch.equal(got.double(), ref64), "%s side %d: an fp32 sum (%d lanes) differs from the float64 sum" % (case.id, side, lanes)
        ref = rx.pooled(W, feat, dtype)
        if zero is not None:
            assert bool((ref[zero].float() == 0).all())
        if dtype == BF16 and case.L >= 729:  # the one rounding is not idle
            assert bool((ref.double() != ref64).any())
        # raw uint8 masks: through the wrapper's tables they give P back, through the test's own the gathered mask
        raw = rx.raw_u8(P)
        assert torch.equal(raw[:, ::2, ::2].double(), P) and int((raw == 255).sum()) == 3 * case.M * side * side
        ys, xs, gather = rx.own_tables(side, case.seed)
        assert torch.equal(raw[:, ys.long()][:, :, xs.long()].double(), gather(P)) and sorted(xs.tolist()) == list(range(0, 2 * side, 2))
        assert not torch.equal(gather(P), P) or zero == 0


@pytest.mark.parametrize("case,side", SIDES, ids=SIDE_IDS)
def test_region_data_tells_wrong_kernels_apart(case, side):
    feat = rx.features(case)
    P, zero = rx.mask_sets(case, side)[0]
    ref = rx.reference(case, P, feat).float()
    live = [m for m in range(case.M) if m != zero]
    muts = rx.mutants(case, P, feat)
    assert len(muts) == 9
    for kind, out in muts.items():
        what = "%s side %d" % (case.id, side)
        if out is None:
            _log(what, kind, None)
            continue
        diff = out.float()[live] != ref[live]
        _log(what, kind, float(diff.float().mean()))
        assert bool(diff.any(1).all()), "%s: '%s' leaves the row of mask(s) %s as it was" % (
            what, kind, [live[i] for i in (~diff.any(1)).nonzero()[:, 0].tolist()])
    # what a case cannot show is what its shape rules out, nothing else
    assert (muts["channels c, c + 8 swapped"] is None) == (case.C < 16) and (muts["masks m, m + 1 exchanged"] is None) == (case.M == 1)


@pytest.mark.parametrize("M,S,fw", [(3, 384, 27), (8, 384, 108), (5, 256, 64)])
def test_box_masks_cannot_see_the_order_of_positions(M, S, fw):
    """Module docstring.  For the box masks of test_region_pool_true_shape_vs_oracle: wherever a position and the partner it would be
    swapped with (p ^ 1, p ^ 4) both lie inside the box -- resampled weight 1 -- the swap changes nothing: a mistake confined to the
    inside of a box is invisible, and only the pairs that straddle an edge column carry any signal (their share is printed).  On the
    exact data more than half of the weighted pairs are of unlike weight, wherever they lie: the test below."""
    v = F.interpolate(rx.box_masks(M, S).float()[None], scale_factor=(fw * fw / (S * S)) ** 0.5, mode="bilinear")[0].double().flatten(1)
    for xor in (1, 4):
        differs, weighted, partner = _differs_from_partner(v, xor)
        inside = (v == 1) & (partner == 1)
        assert not bool((differs & inside).any()) and float(inside.sum()) > 0
        _log("box masks %dx%d -> %d" % (S, S, fw), "weighted pairs (p, p ^ %d) of unlike weight" % xor, float(differs.sum()) / float(weighted.sum()))


def _differs_from_partner(v, xor):
    partner = v[:, rx._pair_perm(v.shape[1], 32, lambda p: p ^ xor)]
    return v != partner, (v > 0) | (partner > 0), partner


@pytest.mark.parametrize("case,side", SIDES, ids=SIDE_IDS)
def test_exact_masks_see_the_order_of_positions_everywhere(case, side):
    v = rx.resampled(rx.mask_sets(case, side)[0][0], case.fw)
    for xor in (1, 4):
        differs, weighted, _ = _differs_from_partner(v, xor)
        share = float(differs.sum()) / float(weighted.sum())
        _log("%s side %d" % (case.id, side), "weighted pairs (p, p ^ %d) of unlike weight" % xor, share)
        assert share > 0.5


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("cols", rx.LN_COLS + (16,))
@pytest.mark.parametrize("bias_bound", [8, rx.GELU_BIAS_BOUND])
def test_layernorm_rows_have_one_output(cols, bias_bound):
    """the kernel's fp32 expression (x - mean) * rstd * g + b rounds to the bf16 value v / 4 * g + b with rstd at -8, 0 and +8 ulps of
    rsqrt(var + eps), eps 1e-6 and 1e-5, with and without a fused multiply-add"""
    x, v, m, s = rx.ln_rows(5, cols, cols)
    g, b = rx.ln_params(cols, cols, bias_bound)
    assert torch.equal(x.to(BF16).double(), x) and torch.equal(g.to(BF16).double(), g) and torch.equal(b.to(BF16).double(), b)
    assert torch.equal(g * 2, (g * 2).round()) and float(g.abs().max()) <= 2
    assert torch.equal((b * 16) % 2, torch.ones_like(b)) and float(b.abs().max()) < bias_bound
    assert set(s.tolist()) == set(rx.LN_S) and set(m.tolist()) == set(rx.LN_M)
    # every partial sum of x (half units) and of (x - mean)^2 (quarter units) is exact in any order
    assert float(x.abs().sum(1).max()) * 2 < 2 ** 24 and torch.equal(x * 2, (x * 2).round())
    assert torch.equal(x.sum(1), m * cols)
    mean = (x.sum(1).float() / torch.tensor(float(cols), dtype=F32))  # one IEEE division
    assert torch.equal(mean.double(), m)
    d = x.float() - mean[:, None]
    assert torch.equal(d.double(), s[:, None] * v)
    q = (d.double() ** 2).sum(1)
    assert float(q.max()) * 4 < 2 ** 24 and torch.equal(q, 16 * s * s * cols)
    var = q.float() / torch.tensor(float(cols), dtype=F32)
    assert torch.equal(var.double(), 16 * s * s)
    want = rx.ln_expected(v, g, b)
    assert torch.equal(want.to(BF16).double(), want) and torch.equal((want * 16) % 2, torch.ones_like(want))
    assert float(want.abs().max()) < 7 / 4 * 2 + bias_bound
    g32, b32 = g.float(), b.float()
    for eps in (1e-6, 1e-5):
        r0 = torch.rsqrt(var + torch.tensor(eps, dtype=F32))
        for ulps in (-8, 0, 8):
            r = (r0.view(torch.int32) + ulps).view(F32)
            p = d * r[:, None]
            plain = p * g32 + b32
            fused = (p.double() * g + b).float()
            for name, t in (("plain", plain), ("fused", fused)):
                assert torch.equal(rne(t).double(), want), "cols %d eps %g rstd %+d ulps, %s: not the bf16 value" % (cols, eps, ulps, name)


@pytest.mark.parametrize("cols", rx.LN_COLS)
def test_gelu_reference_is_rarely_near_a_rounding_boundary(cols):
    _, v, _, _ = rx.ln_rows(5, cols, cols)
    g, b = rx.ln_params(cols, cols, rx.GELU_BIAS_BOUND)
    y = rx.ln_expected(v, g, b)
    assert float(y.abs().max()) < 6
    ref = rx.gelu64(y)
    band = y.abs() * rx.GELU_SLACK
    sel = y >= -1
    near = (rne((ref - band).float()) != rne((ref + band).float())) & sel
    share = float(near.sum()) / float(sel.sum())
    _log("layernorm + gelu cols %d" % cols, "reference within |y| 2^-20 of a bf16 boundary (y >= -1)", share)
    assert share < rx.EXCLUDED_CAP
    assert bool((rx.gelu_limit(y, ref) > 0).all()) and bool((ref != 0).all())


# ------------------------------------------------------------------------------------------------ the references of the plain kernels
@pytest.mark.parametrize("in_w,out_w", rx.AVGPOOL_SHAPES)
def test_avgpool_reference(in_w, out_w):
    from tests.util import ints
    x = ints((2, in_w * in_w, 8), 8, in_w)
    ref = rx.avgpool_reference(x, 2, in_w, out_w, F32)
    tor = F.adaptive_avg_pool2d(x.reshape(2, in_w, in_w, 8).permute(0, 3, 1, 2), out_w).flatten(2).transpose(1, 2)
    assert float((ref.double() - tor).abs().max()) <= 2.0 ** -20
    sizes = {b - a for a, b in rx.avgpool_windows(in_w, out_w)}
    assert sizes == {(108, 27): {4}, (96, 27): {4, 5}, (27, 27): {1}, (24, 7): {4, 5}}[(in_w, out_w)]
    if (in_w, out_w) == (96, 27):  # windows overlap
        w = rx.avgpool_windows(in_w, out_w)
        assert any(w[i][1] > w[i + 1][0] for i in range(out_w - 1))


def test_s2d_and_im2col_references():
    from oracle import srgpt_oracle as so
    from tests.util import ints, load_kat
    for g in (3, 24, 27):
        x = ints((2, g * g, 8), 100, g)
        assert torch.equal(rx.s2d_reference(x, g), so.flat_square(x.reshape(2, g, g, 8)).reshape(2, -1, 32))
    z = load_kat()
    xin = torch.from_numpy(z["s2d.in"]).double()
    assert torch.equal(rx.s2d_reference(xin, int(xin.shape[1] ** 0.5)), torch.from_numpy(z["s2d.out"]).double())
    for S, kp in ((56, 588), (28, 592)):
        img = ints((2, 3, S, S), 100, S)
        col = rx.im2col_reference(img, 14, kp)
        assert torch.equal(col[:, :588], F.unfold(img, kernel_size=14, stride=14).transpose(1, 2).reshape(-1, 588))
        assert float(col[:, 588:].abs().sum()) == 0
