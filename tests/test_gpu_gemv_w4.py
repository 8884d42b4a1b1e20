"""The MXFP4 decode product and expansion (srgpt_gemv_w4, srgpt_dequant_mxfp4; gemv_w4.hip) on the GPU.

1. The code table: every e2m1 code under the scale bytes 1, 64, 127, 190 and 254, in a low nibble, a high nibble and a second block of
   a row, through srgpt_dequant_mxfp4 and through the product with a one-hot x, against float64 `grid[code] * 2^(byte - 127)` rounded
   once to bf16 (byte 1 reaches the subnormals, byte 254 overflows to infinity from code 2.0 on).
2. Bit for bit on data for which a correct kernel has ONE possible output, in the manner of tests/test_gpu_gemv_exact.py (whose
   helpers this file uses): x integers in [-8, 8], weights random e2m1 codes with block scales in {1/2, 1, 2} -- multiples of 1/4 up to
   12 -- so every product is a multiple of 1/4, 4 * 96 * K < 2^24 at K <= 4096 and every fp32 partial sum in every order is exact.
   Reference: the float64 product rounded once, out = rnd(rnd(acc) + residual); out_f32 stores that bf16-valued number widened.
   RMSNorm: the octet rows of test_gpu_gemv_exact.py (normalised rows exactly x / rms * norm_w in quarter units, |.| <= 7: 16 * 84 K <
   2^24).  SwiGLU (odd N): the gate rows hold +-0.25 in 32 places and zeros elsewhere, so |gate| stays under the 32 that module's band
   for __expf is derived for (asserted); elements within that band of a rounding boundary may take either neighbour, capped at 3 %.
   Surroundings: x, codes, scales, norm_w and the residual are followed by NaN / 0xFF (0xFF: a NaN scale), `out` is rows 1 .. B of a
   sentinel-filled allocation that must survive; every call runs twice with equal bits.
3. Random data against fp32 torch on the dequantised weights, within the bf16-rounding bound of tests/test_gpu_kernels.py (_tol)."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_gemv_exact import EXCLUDED_CAP, _normed, _octet_rows, _run_twice, _swiglu_refs
from tests.util import assert_close, ints, poisoned, rne

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def _ops():
    from spatialrgpt_amd import ops
    return ops


def _tol(ref, dtype, k=1.0):  # tests/test_gpu_kernels.py, unchanged
    s = float(ref.float().abs().max()) + 1e-6
    return (2e-2 if dtype == torch.bfloat16 else 2e-5) * s * k


def pack(code):
    """codes 0 .. 15 [N, K] -> bytes [N, K / 2]: even k in the low nibble"""
    code = code.to(torch.uint8)
    return (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()


def values(code, sbytes):
    """float64 [N, K] of codes [N, K] and scale bytes [N, K / 32]"""
    v = GRID[(code & 7).long()] * (1 - 2 * (code >> 3).double())
    return v * torch.ldexp(torch.ones(sbytes.shape, dtype=torch.float64), sbytes.long() - 127).repeat_interleave(32, dim=1)


# ------------------------------------------------------------------------------------------------ 1. the table
def test_every_code_under_five_scale_bytes():
    ops = _ops()
    sb = (1, 64, 127, 190, 254)
    K = 64
    for k in (0, 1, 37):  # low nibble, high nibble, second block
        code = torch.zeros((16 * len(sb), K), dtype=torch.int64)
        sbytes = torch.full((16 * len(sb), K // 32), 127, dtype=torch.uint8)
        for i, b in enumerate(sb):
            code[16 * i:16 * i + 16, k] = torch.arange(16)
            sbytes[16 * i:16 * i + 16, k // 32] = b
        want = values(code, sbytes)
        table = want[:, k].float().to(BF16)  # float64 -> fp32 is exact or infinite here; then ONE rounding to bf16
        w4, sc = poisoned(pack(code), rows_after=5, poison=0xFF), poisoned(sbytes, rows_after=5, poison=0xFF)
        deq = ops.dequant_mxfp4(w4, sc).cpu()
        x = torch.zeros((1, K), dtype=BF16)
        x[0, k] = 1.0
        out = ops.gemv_w4(x.to(DEV), w4, sc).cpu()
        for name, got in (("dequant", deq[:, k]), ("product", out[0])):  # the figures before the assertions
            for r in (got.float() != table.float()).nonzero().flatten().tolist():
                print("k = %d, %s: code %d under byte %d gives %r, the table says %r" % (k, name, r % 16, sb[r // 16], float(got[r]), float(table[r])))
        # by value (code 8 is a zero whatever its sign bit; the infinities of byte 254 equal themselves; a NaN equals nothing)
        assert torch.equal(deq.float(), want.float().to(BF16).float()), "srgpt_dequant_mxfp4, k = %d" % k
        assert torch.equal(out[0].float(), table.float()), "srgpt_gemv_w4 with a one-hot x, k = %d" % k


# ------------------------------------------------------------------------------------------------ 2. exact data
def exact_weights(R, K, seed, gate_rows=0):
    """-> (codes [R, K], scale bytes [R, K / 32]); the first `gate_rows` rows: +-0.25 in 32 places (fewer at K = 32: 8), else zero"""
    g = torch.Generator().manual_seed(seed)
    code = torch.randint(0, 16, (R, K), generator=g)
    sbytes = torch.randint(126, 129, (R, K // 32), generator=g).to(torch.uint8)
    for r in range(gate_rows):
        at = torch.randperm(K, generator=g)[:min(32, K // 4)]
        row = torch.zeros(K, dtype=torch.int64)
        row[at] = 1 + 8 * torch.randint(0, 2, (at.numel(),), generator=g)  # code 1 = 0.5, with or without the sign bit
        code[r] = row
        sbytes[r] = 126  # 0.5 * 2^-1
    return code, sbytes


def device_weights(code, sbytes):
    return poisoned(pack(code), rows_after=5, poison=0xFF), poisoned(sbytes, rows_after=5, poison=0xFF)


def exact_case(B, N, K, seed, variants=("plain", "norm", "swiglu")):
    ops = _ops()
    what0 = "B=%d N=%d K=%d" % (B, N, K)
    assert 4 * 96 * K < 2 ** 24 and 16 * 84 * K < 2 ** 24
    eps = 1e-5
    for variant in variants:
        what = what0 + " " + variant
        if variant == "norm":
            x64, rms = _octet_rows(B, K, seed)
            nw64 = ints((K,), 4, seed + 1)
            xe = _normed(x64, rms, nw64, eps, what)
            norm_w = poisoned(nw64.to(BF16))
        else:
            x64 = xe = ints((B, K), 8, seed)
            norm_w = None
        assert torch.equal(x64.to(BF16).double(), x64)
        x_d = poisoned(x64.to(BF16))
        if variant == "swiglu":
            Ns = N if N % 2 else N + 1  # odd: the tail unit is partly filled in the gate and in the up rows
            code, sbytes = exact_weights(2 * Ns, K, seed + 2, gate_rows=Ns)
            acc = xe @ values(code, sbytes).T
            assert torch.equal(acc.float().double(), acc)
            tally = {}
            ref, alt = _swiglu_refs(acc[:, :Ns].float(), acc[:, Ns:].float(), what, tally)
            n, total = tally["swiglu excluded"]
            assert n <= max(EXCLUDED_CAP * total, 1), "%s: %d of %d elements within the band of a rounding boundary" % (what, n, total)
            w4, sc = device_weights(code, sbytes)
            _run_twice(lambda out: ops.gemv_w4(x_d, w4, sc, swiglu=True, out=out), B, Ns, BF16, ref.to(BF16).to(DEV), alt.to(BF16).to(DEV), what)
            continue
        code, sbytes = exact_weights(N, K, seed + 2)
        acc = xe @ values(code, sbytes).T
        assert torch.equal(acc.float().double(), acc)
        prod = acc.float()
        res_i = ints((B, N), 256, seed + 3)
        refs = {"plain": rne(prod), "res": rne(rne(prod) + res_i.float())}
        res_d = poisoned(res_i.to(BF16))
        w4, sc = device_weights(code, sbytes)
        for epi in ("plain", "res"):
            for out_f32 in (False, True):
                odt = F32 if out_f32 else BF16
                r = res_d if epi == "res" else None
                call = lambda out, r=r, out_f32=out_f32: ops.gemv_w4(x_d, w4, sc, norm_w, eps, r, out=out, out_f32=out_f32)
                _run_twice(call, B, N, odt, refs[epi].to(BF16).to(odt).to(DEV), None, "%s, %s%s" % (what, epi, " -> fp32" if out_f32 else ""))


@pytest.mark.parametrize("B", [1, 2, 4, 5, 9])
@pytest.mark.parametrize("K", [32, 2048, 2080, 4096])
def test_exact_products(B, K):
    """K: one block; one full iteration of 64 chunks; 65 chunks (a second iteration with one live lane); two iterations = one batch.
    B: every template instance but 3 alone, and calls cut into passes of 4 + 1 and 4 + 4 + 1.  N: fewer units than waves, a partly
    filled unit, one wave per unit."""
    for N in (1, 3, 7, 64):
        exact_case(B, N, K, 1000 * B + 7 * N + K)


@pytest.mark.parametrize("B", [1, 3, 4, 5])
def test_exact_products_more_units_than_residual_slots(B):
    """N x K = 40000 x 32: 20000 units over at most 2048 waves -- a wave owns more units than the four whose residual elements the
    prologue stages through LDS, so the later units read theirs from memory"""
    exact_case(B, 40000, 32, 77 + B, variants=("plain",))


@pytest.mark.parametrize("N", [3, 7])
def test_exact_products_looping_prologue(N):
    """4 rows x K = 4128: 4 * 516 = 2064 activation chunks, more than the 256 * 8 the prologue's threads hold in registers -- the
    last 16 chunks (the tail of row 3) are staged, squared and normalised by its loops"""
    exact_case(4, N, 4128, 500 + N, variants=("plain", "norm"))


# ------------------------------------------------------------------------------------------------ 3. random data
def _rand(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


@pytest.mark.parametrize("B,N,K", [(1, 1000, 4096), (2, 4096, 4096), (4, 1001, 2560), (5, 512, 11008), (9, 130, 288), (3, 4096, 14336)])
def test_random_data_vs_torch_on_dequantised_weights(B, N, K):
    ops = _ops()
    x, w = _rand((B, K), BF16, 21), _rand((N, K), BF16, 22, 0.03)
    g, r = (1 + 0.1 * _rand((K,), F32, 23)).to(BF16), _rand((B, N), BF16, 24)
    codes, scales, deq = ops.quantize_mxfp4_rows(w.to(DEV))
    assert torch.equal(ops.dequant_mxfp4(codes, scales), deq)
    wq = deq.float().cpu()
    # the quantiser on real-valued data: half a grid step at the top of a block, i.e. at most amax / 3
    blocks = w.float().reshape(N, K // 32, 32)
    assert bool(((wq.reshape_as(blocks) - blocks).abs().amax(2) <= blocks.abs().amax(2) / 3).all())
    ref = x.float() @ wq.T
    xd = x.to(DEV)
    assert_close(ops.gemv_w4(xd, codes, scales), ref, _tol(ref, BF16), 0, "gemv_w4")
    assert_close(ops.gemv_w4(xd, codes, scales, residual=r.to(DEV)), ref.to(BF16).float() + r.float(), _tol(ref, BF16, 2), 0, "gemv_w4+res")
    lo = ops.gemv_w4(xd, codes, scales, out_f32=True)
    assert lo.dtype == F32
    assert_close(lo, ref, _tol(ref, BF16), 0, "gemv_w4 f32")
    xf = x.float()
    xn = g * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)).to(BF16)
    refn = xn.float() @ wq.T
    assert_close(ops.gemv_w4(xd, codes, scales, norm_w=g.to(DEV), eps=1e-5), refn, _tol(refn, BF16), 0, "rmsnorm+gemv_w4")
    # consistency with the bf16 path on the dequantised weights (what prefill multiplies)
    assert_close(ops.gemv_w4(xd, codes, scales), ops.gemv(xd, deq).float().cpu(), _tol(ref, BF16, 2), 0, "w4 vs bf16(deq)")
    if N % 2 == 0:
        h = N // 2
        gate, up = (x.float() @ wq[:h].T).to(BF16), (x.float() @ wq[h:].T).to(BF16)
        refs = F.silu(gate.float()).to(BF16).float() * up.float()
        assert_close(ops.gemv_w4(xd, codes, scales, swiglu=True), refs, _tol(refs, BF16), 0, "swiglu gemv_w4")
