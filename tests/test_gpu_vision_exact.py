"""Region pooling (csrc/region.hip) and the vision tower's row kernels (srgpt_layernorm, srgpt_rmsnorm, srgpt_avgpool,
srgpt_vit_assemble_cls, srgpt_s2d, srgpt_im2col) bit for bit on data for which a correct kernel has ONE possible output, in the manner
of tests/test_gpu_gemm_exact.py and tests/test_gpu_gemv_exact.py.  The data, its float64 references and the reasons they are exact are
in tests/region_exact.py; tests/test_host_region_exact.py asserts every precondition on the CPU and shows that the data tells wrong
kernels from the right one.

Region pooling.  Every case of region_exact.CASES -- the smallest shape at which each path of region.hip exists -- runs with every
mask side of the case and every mask type (bf16, fp32, raw uint8) through the wrappers, twice, `torch.equal` against the reference;
the all-zero mask's row is exactly 0.0.  Raw uint8 masks are twice the processor size with 255 in every pixel the nearest-neighbour
tables do not name, once through ops.region_pool_u8 and once straight at the C ABI with tables of the test's own (rows reversed,
columns permuted).  Straight at the C ABI, for every case of at most 16 masks (one MFMA case per CH, the MFMA case of 25 row slabs,
one VALU case per MM and the VALU case of 17 row slabs among them): the features and masks are followed by NaN rows, `out` is rows
1 .. M of a sentinel-filled allocation, the workspace is filled with 0xFF bytes (NaN partials, garbage tickets) with a sentinel guard
of 1024 floats behind it, and the second call runs on the workspace as the first left it.

Row kernels.  bf16 LayerNorm without activation, RMSNorm, avgpool and the three data movers: `torch.equal`, poisoned input tails,
guarded outputs; LayerNorm also in place (y == x, as model.hip calls it for pre_ln).  fp32 LayerNorm: within 16 * 2^-24 * (|p g| + |b|)
of the float64 value (rsqrtf is not pinned to an ulp; 16 is margin over its few ulps plus three roundings).  LayerNorm + GELU(erf):
within one bf16 ulp of rnd(gelu64(y)) plus |y| 2^-20, and at least 97 % of the elements with y >= -1 EQUAL to it (y is the exact
LayerNorm output, an odd sixteenth below 6: the arguments of erff are a few hundred distinct values, not a continuum).

SRGPT_EXACT_LOG=<file> appends the measured GELU figures (profiles/vision_exact.txt was made from it)."""
import functools
import json
import os

import pytest
import torch

from tests import region_exact as rx
from tests.test_gpu_gemv_exact import _normed, _octet_rows
from tests.util import BF16, F32, SENTINEL, check_guarded, guarded, ints, poisoned, rne

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD_FLOATS = 1024


def _ops():
    from spatialrgpt_amd import _lib, ops
    return ops, _lib


def _abi(name, *args):
    _, L = _ops()
    L.check(getattr(L.load(), name)(*args, torch.cuda.current_stream().cuda_stream))


def _log(what, kind, value):
    path = os.environ.get("SRGPT_EXACT_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", ""), "what": what, "kind": kind, "value": value}) + "\n")


def _bits(t):
    return t.view(SENTINEL[t.dtype][0])


def _poisoned_nd(t, poison=float("nan")):
    """an n-d tensor on the device, contiguous, followed by poison"""
    flat = t.reshape(-1, t.shape[-1])
    return poisoned(flat, poison=poison).view(t.shape)


def _guard_intact(buf, view, what):
    idt, bits = SENTINEL[buf.dtype]
    view.fill_(torch.tensor([bits], dtype=idt).view(buf.dtype).item())
    assert bool((buf.view(idt) == bits).all()), what + ": written outside the output"


# ------------------------------------------------------------------------------------------------ region pooling
@functools.lru_cache(maxsize=None)
def _region_data(ci, side):
    """computed once per (case, mask side), shared and left unchanged: the features, and per mask set (P, the zero mask's index, the
    reference)"""
    case = rx.CASES[ci]
    feat = rx.features(case)
    return feat, [(P, zero, rx.reference(case, P, feat)) for P, zero in rx.mask_sets(case, side)]


def _dev_masks(P, mask_type):
    if mask_type == "u8":
        return rx.raw_u8(P).to(DEV)
    return _poisoned_nd(P.to(BF16 if mask_type == "bf16" else F32))


def _same(got, ref, what):
    got = got.cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    bad = got != ref
    if bool(bad.any()):
        m, c = (int(i) for i in bad.nonzero()[0])
        pytest.fail("%s: %d of %d elements differ, the first at (mask, channel) = (%d, %d): got %r, expected %r"
                    % (what, int(bad.sum()), bad.numel(), m, c, float(got[m, c]), float(ref[m, c])))
    assert torch.equal(got, ref), what
    return got


REGION_RUNS = [(ci, side, mt) for ci, c in enumerate(rx.CASES) for side in c.sides for mt in rx.MASK_TYPES]


@pytest.mark.parametrize("ci,side,mask_type", REGION_RUNS, ids=["%s-side%d-%s" % (rx.CASES[ci].id, s, mt) for ci, s, mt in REGION_RUNS])
def test_region_pool_exact(ci, side, mask_type):
    ops, _ = _ops()
    case = rx.CASES[ci]
    geo = case.geometry()
    assert all(geo[k] == w for k, w in case.want.items()), (case.id, case.what, geo)  # the path the case exists for, from fw alone
    feat, sets = _region_data(ci, side)
    feat_d = poisoned(feat.to(case.dtype))
    for P, zero, ref in sets:
        what = "%s (%s), mask side %d, %s masks%s" % (case.id, case.what, side, mask_type, ", the zero mask" if case.M == 1 and zero == 0 else "")
        masks_d = _dev_masks(P, mask_type)
        first = None
        for run in range(2):
            out = ops.region_pool_u8(feat_d, masks_d, side) if mask_type == "u8" else ops.region_pool(feat_d, masks_d)
            got = _same(out, ref, what + (", second run" if run else ""))
            assert first is None or torch.equal(_bits(got), _bits(first)), what + ": run-to-run difference"
            first = got
        if zero is not None:
            assert bool((_bits(first[zero]) == 0).all()), what + ": the all-zero mask's row is not +0.0"


def _abi_pool(case, side, feat_d, masks_d, out, ws, mask_type, tables=None):
    _, L = _ops()
    rs = float(side) / case.fw
    assert rs in (1.0, 2.0, 0.5)
    dt = L.BF16 if case.dtype == BF16 else L.F32
    if mask_type == "u8":
        ys, xs = tables
        _abi("srgpt_region_pool_u8", feat_d.data_ptr(), masks_d.data_ptr(), ys.data_ptr(), xs.data_ptr(), out.data_ptr(), ws.data_ptr(),
             case.M, masks_d.shape[1], masks_d.shape[2], side, side, case.fw, case.C, rs, rs, dt)
    else:
        _abi("srgpt_region_pool", feat_d.data_ptr(), masks_d.data_ptr(), out.data_ptr(), ws.data_ptr(), case.M, side, side, case.fw,
             case.C, rs, rs, L.BF16 if mask_type == "bf16" else L.F32, dt)


def _ff_workspace(case):
    """srgpt_region_pool_ws_floats floats of 0xFF bytes, a sentinel guard behind them -> (the allocation, check())"""
    _, L = _ops()
    n = int(L.load().srgpt_region_pool_ws_floats(case.M, case.fw, case.C))
    assert n > 0
    alloc = torch.empty((n + GUARD_FLOATS,), dtype=torch.int32, device=DEV)
    alloc[:n] = -1
    alloc[n:] = SENTINEL[F32][1]

    def check(what):
        assert bool((alloc[n:] == SENTINEL[F32][1]).all()), what + ": written behind the workspace"

    return alloc, check


def _abi_twice(case, side, feat_d, masks_d, ref, mask_type, what, tables=None):
    """twice into ONE 0xFF-filled workspace, `out` guarded; the second call finds the workspace as the first left it"""
    ws, ws_check = _ff_workspace(case)
    first = None
    for run in range(2):
        buf, view = guarded(case.M, case.C, case.C, case.dtype, row0=1)
        _abi_pool(case, side, feat_d, masks_d, view, ws, mask_type, tables)
        torch.cuda.synchronize()
        got = check_guarded(buf, view, ref.to(DEV), what + (", second run" if run else ""))
        ws_check(what)
        assert first is None or torch.equal(_bits(got), _bits(first)), what + ": run-to-run difference"
        first = got


# every case one launch takes (M = 17 is the wrapper's 16 + 1): among them one MFMA case per CH, the MFMA kernel's second round of
# partials, one VALU case per MM and the VALU kernel's second round
ABI_CASES = [i for i, c in enumerate(rx.CASES) if c.M <= rx.RP_MAXM]


@pytest.mark.parametrize("ci", ABI_CASES, ids=[rx.CASES[i].id for i in ABI_CASES])
def test_region_pool_surroundings(ci):
    case = rx.CASES[ci]
    geo = case.geometry()
    assert all(geo[k] == w for k, w in case.want.items()), (case.id, geo)
    for si, side in enumerate(case.sides):
        feat, sets = _region_data(ci, side)
        P, _, ref = sets[0]
        mask_type = ("bf16", "f32")[(si + (case.dtype == F32)) % 2]
        what = "%s at the C ABI, mask side %d, %s masks" % (case.id, side, mask_type)
        _abi_twice(case, side, poisoned(feat.to(case.dtype)), _dev_masks(P, mask_type), ref, mask_type, what)


U8_CASES = [i for i, c in enumerate(rx.CASES) if c.fw in (27, 46)]


@pytest.mark.parametrize("ci", U8_CASES, ids=[rx.CASES[i].id for i in U8_CASES])
def test_region_pool_u8_reads_through_the_tables(ci):
    """tables of the test's own -- rows reversed, columns permuted -- into a raw mask that holds 255 wherever they do not point: the
    reference is the float path on the mask gathered through the same tables"""
    case = rx.CASES[ci]
    for side in case.sides:
        feat, sets = _region_data(ci, side)
        P = sets[0][0]
        ys, xs, gather = rx.own_tables(side, case.seed)
        ref = rx.reference(case, gather(P), feat)
        assert not torch.equal(ref, sets[0][2])  # the tables matter
        what = "%s raw uint8 masks, own tables, mask side %d" % (case.id, side)
        _abi_twice(case, side, poisoned(feat.to(case.dtype)), rx.raw_u8(P).to(DEV), ref, "u8", what, tables=(ys.to(DEV), xs.to(DEV)))


# ------------------------------------------------------------------------------------------------ LayerNorm, RMSNorm
LN_SHAPES = [(rows, cols) for cols in rx.LN_COLS for rows in rx.LN_ROWS]


def _ln_operands(rows, cols, dtype, bias_bound=8):
    x, v, m, s = rx.ln_rows(rows, cols, cols)
    g, b = rx.ln_params(cols, cols, bias_bound)
    return (x, v, m, s, g, b), (poisoned(x.to(dtype)), poisoned(g.to(dtype)), poisoned(b.to(dtype)))


@pytest.mark.parametrize("rows,cols", LN_SHAPES)
def test_layernorm_bf16_exact(rows, cols):
    ops, L = _ops()
    (x, v, m, s, g, b), (x_d, g_d, b_d) = _ln_operands(rows, cols, BF16)
    ref = rx.ln_expected(v, g, b).to(BF16).to(DEV)
    for eps in (1e-6, 1e-5):
        what = "layernorm bf16 %d x %d eps %g" % (rows, cols, eps)
        first = None
        for run in range(2):
            buf, view = guarded(rows, cols, cols, BF16, row0=1)
            ops.layernorm(x_d, g_d, b_d, eps, out=view)
            got = check_guarded(buf, view, ref, what + (", second run" if run else ""))
            assert first is None or torch.equal(_bits(got), _bits(first)), what
            first = got
        # in place: y == x
        buf, view = guarded(rows, cols, cols, BF16, row0=1)
        view.copy_(x_d)
        assert ops.layernorm(view, g_d, b_d, eps, out=view).data_ptr() == view.data_ptr()
        got = check_guarded(buf, view, ref, what + ", in place")
        assert torch.equal(_bits(got), _bits(first)), what + ": in place differs from out of place"


@pytest.mark.parametrize("rows,cols", LN_SHAPES)
def test_layernorm_f32_within_rsqrt(rows, cols):
    ops, L = _ops()
    (x, v, m, s, g, b), (x_d, g_d, b_d) = _ln_operands(rows, cols, F32)
    for eps in (1e-6, 1e-5):
        what = "layernorm fp32 %d x %d eps %g" % (rows, cols, eps)
        p = (x - m[:, None]) / torch.sqrt(16 * s * s + eps)[:, None]
        ref = p * g + b
        limit = 16 * 2.0 ** -24 * ((p * g).abs() + b.abs())
        for inplace in (False, True):
            buf, view = guarded(rows, cols, cols, F32, row0=1)
            if inplace:
                view.copy_(x_d)
            ops.layernorm(view if inplace else x_d, g_d, b_d, eps, out=view)
            got = view.cpu().double()
            err = (got - ref).abs()
            print("%s%s: largest error / limit %.3f" % (what, ", in place" if inplace else "", float((err / limit).max())))
            assert bool(torch.isfinite(got).all()) and bool((err <= limit).all()), \
                "%s: %d elements beyond the bound, the worst at %.2f of it" % (what, int((err > limit).sum()), float((err / limit).max()))
            _guard_intact(buf, view, what)


@pytest.mark.parametrize("rows,cols", LN_SHAPES)
def test_layernorm_gelu_bf16(rows, cols):
    ops, L = _ops()
    (x, v, m, s, g, b), (x_d, g_d, b_d) = _ln_operands(rows, cols, BF16, rx.GELU_BIAS_BOUND)
    y = rx.ln_expected(v, g, b)
    assert float(y.abs().max()) < 6
    ref64 = rx.gelu64(y)
    ref = rne(ref64.float())
    limit = rx.gelu_limit(y, ref64)
    what = "layernorm + gelu(erf) bf16 %d x %d" % (rows, cols)
    buf, view = guarded(rows, cols, cols, BF16, row0=1)
    ops.layernorm(x_d, g_d, b_d, 1e-6, act=L.ACT_GELU_ERF, out=view)
    got = view.float().cpu()
    assert bool(torch.isfinite(got).all()), what
    ratio = float(((got.double() - ref.double()).abs() / limit).max())
    sel = y >= -1
    equal = float((got[sel] == ref[sel]).sum()) / float(sel.sum())
    print("%s: largest error / limit %.4f, equal share (y >= -1) %.5f" % (what, ratio, equal))
    _log(what, "largest error / limit", ratio)
    _log(what, "equal share, y >= -1", equal)
    assert ratio <= 1, "%s: an element lies at %.3f of the bound" % (what, ratio)
    assert equal >= 1 - rx.EXCLUDED_CAP, "%s: only %.2f %% of the elements with y >= -1 equal the reference" % (what, 100 * equal)
    _guard_intact(buf, view, what)


@pytest.mark.parametrize("rows,cols", LN_SHAPES)
def test_rmsnorm_bf16_exact(rows, cols):
    ops, L = _ops()
    what = "rmsnorm bf16 %d x %d" % (rows, cols)
    x, rms = _octet_rows(rows, cols, cols + rows)
    nw = ints((cols,), 4, cols + 1)
    for eps in (1e-6, 1e-5):
        ref = _normed(x, rms, nw, eps, what).to(BF16).to(DEV)
        x_d, w_d = poisoned(x.to(BF16)), poisoned(nw.to(BF16))
        first = None
        for run in range(2):
            buf, view = guarded(rows, cols, cols, BF16, row0=1)
            ops.rmsnorm(x_d, w_d, eps, out=view)
            got = check_guarded(buf, view, ref, what + (", second run" if run else ""))
            assert first is None or torch.equal(_bits(got), _bits(first)), what
            first = got


# ------------------------------------------------------------------------------------------------ avgpool and the data movers
def _code(dtype):
    _, L = _ops()
    return L.BF16 if dtype == BF16 else L.F32


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("in_w,out_w", rx.AVGPOOL_SHAPES)
def test_avgpool_exact(in_w, out_w, C, dtype):
    n = 2
    x = ints((n, in_w * in_w, C), 8, in_w + C)
    ref = rx.avgpool_reference(x, n, in_w, out_w, dtype).reshape(n * out_w * out_w, C).to(DEV)
    x_d = _poisoned_nd(x.to(dtype))  # NaN behind the last image
    what = "avgpool %d -> %d, C %d, %s" % (in_w, out_w, C, dtype)
    for run in range(2):
        buf, view = guarded(n * out_w * out_w, C, C, dtype, row0=1)
        _abi("srgpt_avgpool", x_d.data_ptr(), view.data_ptr(), n, in_w, out_w, C, _code(dtype))
        check_guarded(buf, view, ref, what)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("gg", [4, 729])
def test_vit_assemble_cls_exact(gg, C, n, dtype):
    patches, cls, pos = ints((n, gg, C), 100, gg + C), ints((C,), 100, gg + C + 1), ints((gg + 1, C), 100, gg + C + 2)
    ref = torch.cat([(cls + pos[0]).expand(n, 1, C), patches + pos[1:]], 1)
    assert float(ref.abs().max()) < 256 and ref.shape == (n, gg + 1, C)
    ref = ref.reshape(n * (gg + 1), C).to(dtype).to(DEV)
    p_d, c_d, pos_d = _poisoned_nd(patches.to(dtype)), poisoned(cls.to(dtype)), poisoned(pos.to(dtype))
    buf, view = guarded(n * (gg + 1), C, C, dtype, row0=1)
    _abi("srgpt_vit_assemble_cls", p_d.data_ptr(), c_d.data_ptr(), pos_d.data_ptr(), view.data_ptr(), n, gg, C, _code(dtype))
    check_guarded(buf, view, ref, "vit_assemble_cls gg %d C %d n %d %s" % (gg, C, n, dtype))


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("g", [3, 27, 24])
def test_s2d_exact(g, C, dtype):
    n, hb = 2, (g + 1) // 2
    x = ints((n, g * g, C), 100, g + C)
    ref = rx.s2d_reference(x, g).reshape(n * hb * hb, 4 * C).to(dtype).to(DEV)
    if g % 2:  # the padding of the last row and column is there
        assert float(ref.view(n, hb * hb, 4, C)[:, hb - 1, 2:].abs().max()) == 0 and float(ref.view(n, hb * hb, 4, C)[:, -1, 1].abs().max()) == 0
    x_d = _poisoned_nd(x.to(dtype))
    buf, view = guarded(n * hb * hb, 4 * C, 4 * C, dtype, row0=1)
    _abi("srgpt_s2d", x_d.data_ptr(), view.data_ptr(), n, g, C, _code(dtype))
    check_guarded(buf, view, ref, "s2d g %d C %d %s" % (g, C, dtype))


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("kp", [588, 592])
@pytest.mark.parametrize("S", [56, 28])
def test_im2col_exact(S, kp, dtype):
    n, p = 2, 14
    img = ints((n, 3, S, S), 100, S + kp)
    ref = rx.im2col_reference(img, p, kp).to(dtype).to(DEV)
    assert kp == 588 or float(ref[:, 588:].abs().max()) == 0  # pad columns exactly zero
    img_d = _poisoned_nd(img.to(dtype))
    rows = n * (S // p) ** 2
    buf, view = guarded(rows, kp, kp, dtype, row0=1)
    _abi("srgpt_im2col", img_d.data_ptr(), view.data_ptr(), n, S, p, kp, _code(dtype))
    check_guarded(buf, view, ref, "im2col S %d kp %d %s" % (S, kp, dtype))
