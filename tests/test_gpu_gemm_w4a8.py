"""srgpt_gemm_w4a8 (gemm_f8.hip, the W4 instance: e4m3 activations x MXFP4 codes on v_mfma_scale_f32_16x16x128_f8f6f4 with the E8M0
block scales as the instruction's operand) through the C ABI.

1. Exact data, torch.equal against a float64 product, with the recipe of tests/test_gpu_gemm_exact.py (NaN-poisoned surroundings of
   every operand, a guarded output at two row strides -- three where K is split --, fp32 and bf16 stores, bias + residual, the
   caller's own workspace where K is split).  A: integer e4m3 codes, |a| <= 7, unit row scales except a few rows at 2^+-2.  W: e2m1
   codes with block-scale bytes 126 .. 130, i.e. multiples of 0.25 with |w| <= 48.  With s the row's activation scale every partial
   sum, and the sum plus the bias (|bias|, |residual| <= 256, integers), is a multiple of 0.25 s below 7 * 48 * K * s + 512: as a
   count of that unit it is below 4 * 7 * 48 * K + 4 * 512 / s <= 4 * 7 * 48 * K + 8192 < 2^24, so every fp32 sum in every order is
   exact and a correct kernel has ONE possible output.  The instruction's adder aligns the 128 products of a step to a window below
   the largest (scripts/experiments/probe_f8_mfma_accumulation.py: 13 binades are kept); the scale bytes of one row's K tile
   spread over at most 3 here, so products spread over 7 * 6 / (1 * 0.5) * 2^3 < 2^10.
   Precondition, in the same test: srgpt_gemm_w8a8 returns the float64 product exactly on the e4m3 re-encoding of the same W (every
   value is an e4m3 value; row scale 1) -- if it does not, the data is wrong, not the new kernel.
2. Structured exact cases: which scale byte a lane takes, nibble and register order, row / column, zero blocks, the quantiser's
   clamps.
3. Random data at the limit formula of tests/test_gpu_fp8_mfma.py::test_gemm_w8a8_equals_gemm_of_dequantised_operands, next to the
   same ratio of srgpt_gemm_w8a8 on fp8-quantised weights of the same draw (printed).
4. Rejections reach Python as exceptions."""
import pytest
import torch

from tests.test_gpu_gemm_exact import _assert_live, _epilogue, _run_exact
from tests.util import FP8_NAN, build_gemm_route_cli
from tests.util import exact_f32 as _exact_f32, ints as _ints, poisoned as _poisoned, rne as _rne

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], dtype=torch.float64)


def _ops():
    from spatialrgpt_amd import _lib, ops
    return ops, _lib


@pytest.fixture(scope="module")
def route_cli(tmp_path_factory):
    return build_gemm_route_cli(tmp_path_factory.mktemp("gemm_route_w4a8"))


def _pack(codes):
    """codes [N, K] in 0 .. 15 -> bytes [N, K / 2]: element k in byte k / 2, the low nibble holds the even k (include/srgpt.h)"""
    c = codes.to(torch.uint8)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).contiguous()


def _values(codes, sbytes):
    """float64 [N, K] = e2m1(code) * 2^(byte - 127), one byte per 32 consecutive k"""
    return E2M1[codes.long()] * torch.exp2(sbytes.double() - 127).repeat_interleave(32, dim=1)


def _e4m3(x64):
    """the e4m3 bytes of exactly representable values"""
    q = x64.float().to(torch.float8_e4m3fn)
    assert torch.equal(q.double(), x64), "not e4m3 values"
    return q.view(torch.uint8)


def _random_w(N, K, seed):
    """codes 0 .. 15 and scale bytes 126 .. 130 whose spread inside one row's K tile (4 blocks) is at most 3"""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 16, (N, K), generator=g)
    base = torch.randint(126, 128, (N, K // 128, 1), generator=g)
    sbytes = (base + torch.randint(0, 4, (N, K // 128, 4), generator=g)).reshape(N, K // 32).to(torch.uint8)
    assert int(sbytes.min()) >= 126 and int(sbytes.max()) <= 130
    return codes, sbytes


def _splits(route_cli, M, N, K, want):
    """the K splits of this call on this device (gemm_route_fp8 through tests/gemm_route_cli.cpp, entry gemm_w8a8: srgpt_gemm_w4a8
    takes that route unchanged); asserted against `want` where the device has the 256 CUs the case was chosen for"""
    ops, L = _ops()
    cus = L.load().srgpt_device_cus()
    p, nbytes = ops._ws_arg(torch.device(DEV, torch.cuda.current_device()), M, N)
    r = route_cli([("gemm_w8a8", M, N, K, int(p is not None), nbytes)], cus)[0]
    assert r["family"] == "tile_256" and r["bm"] == 256
    if cus == 256:
        assert r["splits"] == want, "M=%d N=%d K=%d takes %d splits at 256 CUs, the case exists for %d" % (M, N, K, r["splits"], want)
    return r["splits"]


# (256, 256, 256): one full tile, two K tiles | (77, 333, 384): ragged M and N, an odd number of K tiles | (300, 520, 256): two row
# tiles | (259, 512, 1024), (64, 300, 2048): K split in 2 and 4 at 256 CUs
@pytest.mark.parametrize("M,N,K,splits256", [(256, 256, 256, 1), (77, 333, 384, 1), (300, 520, 256, 1), (259, 512, 1024, 2),
                                             (64, 300, 2048, 4)])
def test_gemm_w4a8_exact(route_cli, M, N, K, splits256):
    ops, L = _ops()
    what = "gemm_w4a8 M=%d N=%d K=%d" % (M, N, K)
    assert 4 * 7 * 48 * K + 4 * 512 * 4 < 2 ** 24
    splits = _splits(route_cli, M, N, K, splits256)
    a_i = _ints((M, K), 7, M + 3 * N + K)
    ascale = torch.ones((M,), dtype=F32)
    ascale[1::13] = 4.0
    ascale[5::17] = 0.25
    codes, sbytes = _random_w(N, K, M + N + 7 * K)
    w = _values(codes, sbytes)
    assert float(w.abs().max()) <= 48 and torch.equal(w * 4, (w * 4).round())
    bias_i, res_i = _ints((N,), 256, N + K), _ints((M, N), 256, M + N)
    acc = _exact_f32((a_i @ w.T) * ascale.double()[:, None])
    bias, res = bias_i.float(), res_i.float()
    _assert_live(acc, bias, res, what)
    refs = {"plain": _rne(acc).to(BF16).to(DEV), "bias_res": _epilogue(acc, bias, res, _rne).to(BF16).to(DEV)}

    a_d, ascale_d = _poisoned(_e4m3(a_i), col0=16, cols_after=16, poison=FP8_NAN), _poisoned(ascale)
    # precondition: the fp8 x fp8 kernel is exact on this data (W as e4m3 values, row scale 1)
    w8_d, one_d = _poisoned(_e4m3(w), rows_after=5, poison=FP8_NAN), _poisoned(torch.ones((N,), dtype=F32))
    pre = ops.gemm_w8a8(a_d, ascale_d, w8_d, one_d, out_f32=True)
    assert torch.equal(pre, refs["plain"].float()), what + ": srgpt_gemm_w8a8 is not exact on this data -- the data is wrong"

    # codes: 0xFF = two -6 codes behind the rows; scale bytes: 0xFF = the format's NaN
    w4_d, s_d = _poisoned(_pack(codes), rows_after=5, poison=0xFF).contiguous(), _poisoned(sbytes, rows_after=5, poison=0xFF).contiguous()
    bias_d, res_d = _poisoned(bias_i.to(BF16)), _poisoned(res_i.to(BF16))

    def call(out, epi, out_f32, ws):
        b, r = (bias_d, res_d) if epi == "bias_res" else (None, None)
        ops.gemm_w4a8(a_d, ascale_d, w4_d, s_d, b, r, out=out, out_f32=out_f32, ws=ws)

    ldcs = (N, N + 8) + ((N + 2,) if splits > 1 else ())
    _run_exact(call, M, N, refs, splits, ldcs, None, what)


def _exact_plain(a_i, codes, sbytes, what, ascale=None):
    """out (fp32 store) == bf16(float64 product) for every element"""
    ops, _ = _ops()
    M, N = a_i.shape[0], codes.shape[0]
    ascale = torch.ones((M,), dtype=F32) if ascale is None else ascale
    ref = ((a_i @ _values(codes, sbytes).T) * ascale.double()[:, None]).to(BF16)
    assert bool(torch.isfinite(ref.float()).all())
    out = ops.gemm_w4a8(_e4m3(a_i).to(DEV), ascale.to(DEV), _pack(codes).to(DEV), sbytes.to(DEV), out_f32=True)
    bad = out.cpu() != ref.float()
    if bool(bad.any()):
        m, n = (int(i) for i in bad.nonzero()[0])
        pytest.fail("%s: %d of %d elements differ, the first at (m, n) = (%d, %d): got %r, expected %r"
                    % (what, int(bad.sum()), bad.numel(), m, n, float(out[m, n]), float(ref[m, n])))
    return ref


SM, SN, SK = 80, 272, 384  # the structured cases: a ragged row tile, two column tiles, three K tiles


def test_each_lane_takes_the_scale_byte_of_its_own_block():
    """bytes 127, 128, 129, 130 in blocks g = 0 .. 3 of every K tile: another byte per lane changes every element"""
    codes, _ = _random_w(SN, SK, 1)
    sbytes = torch.tensor([127, 128, 129, 130], dtype=torch.uint8).repeat(SN, SK // 128)
    a_i = _ints((SM, SK), 7, 2)
    ref = _exact_plain(a_i, codes, sbytes, "scale bytes 127 .. 130 by block")
    flat = ((a_i @ _values(codes, torch.full_like(sbytes, 127)).T)).to(BF16)
    assert float((ref != flat).float().mean()) > 0.9  # the data tells the bytes apart


def test_nibble_and_register_order():
    """(a) W holds one 1.0 per row, at k = (7 n + 3) % K: out[m, n] = a[m, that k] -- every k position is visited, an exchange of
    nibbles, bytes, registers or K tiles moves a value.  (b) codes that depend on the parity of k and on the dword of the lane's
    fragment ((k % 32) / 8) only, against random A."""
    a_i = _ints((SM, SK), 7, 3)
    n = torch.arange(SN)
    codes = torch.zeros((SN, SK), dtype=torch.int64)
    codes[n, (7 * n + 3) % SK] = 2
    sbytes = torch.full((SN, SK // 32), 127, dtype=torch.uint8)
    ref = _exact_plain(a_i, codes, sbytes, "one-hot rows")
    assert torch.equal(ref.double(), a_i[:, (7 * n + 3) % SK])
    k = torch.arange(SK)
    pattern = torch.tensor([1, 2, 3, 4, 13, 14, 15, 7])[(k % 2) * 4 + (k % 32) // 8]
    codes = pattern[None, :].repeat(SN, 1)
    codes[1::2] = (codes[1::2] + 8) % 16  # odd rows: the other sign
    _exact_plain(a_i, codes, sbytes, "codes by parity of k and dword of the fragment")


def test_identity_rows_give_back_the_weights():
    """A = identity rows: out[m, n] = W[n, m] -- a row / column exchange or a transposed tile shows"""
    K = 256
    codes, sbytes = _random_w(SN, K, 4)
    a_i = torch.eye(K, dtype=torch.float64)
    ref = _exact_plain(a_i, codes, sbytes, "identity A")
    assert torch.equal(ref.double(), _values(codes, sbytes).T)


def test_zero_blocks_and_the_quantisers_clamps():
    """an all-zero block as ops.quantize_mxfp4_rows stores it (byte 127, codes 0) between live blocks; rows whose blocks all sit at
    byte 63 and rows all at 191 (the quantiser's exponent clamps, -64 / +64; never mixed within a row)"""
    a_i = _ints((SM, SK), 7, 5)
    codes, sbytes = _random_w(SN, SK, 6)
    zero = torch.rand((SN, SK // 32), generator=torch.Generator().manual_seed(7)) < 0.3
    sbytes[zero] = 127
    codes[zero.repeat_interleave(32, dim=1)] = 0
    _exact_plain(a_i, codes, sbytes, "zero blocks")
    codes, sbytes = _random_w(SN, SK, 8)
    sbytes[:] = 127
    sbytes[0::3] = 63
    sbytes[1::3] = 191
    ascale = torch.ones((SM,), dtype=F32)
    ascale[2::5] = 0.25
    ref = _exact_plain(a_i, codes, sbytes, "rows at the clamps", ascale)
    assert 0 < float(ref[:, 0::3].abs().max()) < 2.0 ** -40 and float(ref[:, 1::3].abs().max()) > 2.0 ** 60


ACC_COEF = 2e-4  # of sum_k |a_k w_k|: tests/test_gpu_fp8_mfma.py's accumulation term, derived there for the unit-scale form


@pytest.mark.parametrize("M,N,K", [(77, 333, 384), (259, 6144, 4096), (513, 4096, 14336)])
def test_gemm_w4a8_equals_gemm_of_dequantised_operands(M, N, K):
    """Against the fp64 GEMM of the dequantised operands (computed on the device in float64 by torch), test_gpu_fp8_mfma.py's limit:
    half a bf16 ulp of the reference plus ACC_COEF * sum |a w|, and more than 0.95 of the elements equal to the correctly rounded
    reference.  W = ops.quantize_mxfp4_rows(randn * 0.03).  The same ratio for srgpt_gemm_w8a8 on ops.quantize_fp8_rows of the same
    draw is printed beside it: the coefficient was derived for that kernel."""
    from tests.test_gpu_fp8_mfma import _acts, _deq

    ops, L = _ops()
    g = torch.Generator().manual_seed(M + N + K)
    a8, asc, _ = ops.quantize_fp8_rows(_acts(M, K, 1))
    draw = (torch.randn((N, K), generator=g) * 0.03).to(BF16)
    w4, s8, deq = ops.quantize_mxfp4_rows(draw)
    w8, wsc, _ = ops.quantize_fp8_rows(draw)
    A = _deq(a8, asc).to(DEV)

    def ratio(out, W):
        ref = A @ W.T
        acc_tol = ACC_COEF * (A.abs() @ W.abs().T)
        lim = 2.0 ** -8 * (ref.abs() + acc_tol) + acc_tol + 1e-30
        same = float((out.double() == ref.to(BF16).double()).double().mean())
        return float(((out.double() - ref).abs() / lim).max()), same, ref, acc_tol

    r8, same8, _, _ = ratio(ops.gemm_w8a8(a8.to(DEV), asc.to(DEV), w8.to(DEV), wsc.to(DEV), out_f32=True), _deq(w8, wsc).to(DEV))
    W = deq.double().to(DEV)
    assert torch.equal(W.cpu(), _values(((w4[:, :, None] >> torch.tensor([0, 4], dtype=torch.uint8)) & 15).reshape(N, K), s8))
    out = ops.gemm_w4a8(a8.to(DEV), asc.to(DEV), w4.to(DEV), s8.to(DEV), out_f32=True)
    assert out.dtype == F32
    r4, same4, ref, acc_tol = ratio(out, W)
    print(f"\ngemm_w4a8 {M}x{N}x{K}: max err / limit = {r4:.3f}, equal to the rounded reference: {same4:.5f}"
          f"   |   gemm_w8a8 on fp8 weights of the same draw: {r8:.3f}, {same8:.5f}")
    assert r4 <= 1.0, "plain output outside half a bf16 ulp + the accumulation bound"
    assert same4 > 0.95, f"only {same4:.4f} of the elements equal the correctly rounded reference"
    # bias and residual: round(acc * scale + bias) -> round(+ residual), as srgpt_gemm materialises them
    b = (torch.randn((N,), generator=g) * 0.1).to(BF16).to(DEV)
    r = torch.randn((M, N), generator=g).to(BF16).to(DEV)
    mid = (ref + b.double()).to(BF16).double()
    ref2 = (mid + r.double()).to(BF16)
    out2 = ops.gemm_w4a8(a8.to(DEV), asc.to(DEV), w4.to(DEV), s8.to(DEV), bias=b, residual=r)
    assert out2.dtype == BF16
    d = (out2.double() - ref2.double()).abs()
    lim2 = 2.0 ** -7 * (mid.abs() + ref2.double().abs()) + 2 * acc_tol + 1e-30  # one ulp at either rounding point
    same2 = float((out2 == ref2).double().mean())
    print(f"  + bias + residual: max err / limit = {float((d / lim2).max()):.3f}, equal to the rounded reference: {same2:.5f}")
    assert float((d / lim2).max()) <= 1.0, "bias + residual output outside the rounding limits"
    assert same2 > 0.95, f"only {same2:.4f} of the elements equal the correctly rounded reference"


def test_gemm_w4a8_rejections_reach_python():
    ops, L = _ops()
    sc = torch.ones((16,), dtype=F32, device=DEV)

    def operands(K):
        return (torch.zeros((16, K), dtype=torch.uint8, device=DEV), sc, torch.zeros((16, K // 2), dtype=torch.uint8, device=DEV),
                torch.full((16, K // 32), 127, dtype=torch.uint8, device=DEV))

    for K in (192, 128, 64):
        with pytest.raises(NotImplementedError, match="multiple of 128"):
            ops.gemm_w4a8(*operands(K))
    a8, _, w4, s8 = operands(256)
    with pytest.raises(ValueError, match="codes"):  # scales that do not belong to the codes
        ops.gemm_w4a8(a8, sc, w4, s8[:, :4].contiguous())
    with pytest.raises(ValueError, match="K = 256"):
        ops.gemm_w4a8(a8, sc, operands(512)[2], operands(512)[3])
    with pytest.raises(ValueError, match="uint8"):
        ops.gemm_w4a8(a8.float(), sc, w4, s8)
    with pytest.raises(ValueError, match="bf16"):
        ops.gemm_w4a8(a8, sc, w4, s8, bias=torch.zeros((16,), device=DEV))
    wide = torch.zeros((16, 520), dtype=torch.uint8, device=DEV)  # lda = 520: rows not 16-byte aligned
    with pytest.raises(NotImplementedError, match="aligned"):
        ops.gemm_w4a8(wide[:, :256], sc, w4, s8)
    out = ops.gemm_w4a8(a8, sc, w4, s8)  # the operands themselves are fine
    assert out.shape == (16, 16) and not bool(out.any())
