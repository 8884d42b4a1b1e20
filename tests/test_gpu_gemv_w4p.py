"""The packed MXFP4 decode layout and the MFMA product over it (srgpt_pack_mxfp4, srgpt_unpack_mxfp4, srgpt_gemv_w4p; gemv_w4p.hip and
the W4 mode of skinny.hip) on the GPU.

1. Round trip: unpack(pack(codes, scales)) is the input, the packed array is the one the byte-offset formula of include/srgpt.h
   gives (padding rows: code 0, scale byte 127), surroundings poisoned, a sentinel behind every written array.
2. The code table: every e2m1 code under the scale bytes 2, 64, 127, 190 and 252 (the kernel's documented domain: every value a normal
   finite bf16) at k = 0, 1, 37 and 129 -- low nibble, high nibble, another k step and lane group, the second 16-byte load -- through
   the product with a one-hot x on row 2 of 3, against float64 `grid[code] * 2^(byte - 127)` rounded once to bf16.
3. Exact data, in the manner of tests/test_gpu_gemv_w4.py (its construction, imported): x integers, block scales in {1/2, 1, 2},
   octet rows for the RMSNorm, the SwiGLU band with its 3 % cap -- ONE possible output, the float64 product rounded once.  Every call
   runs twice with equal bits into a guarded output.
4. The bits of the bf16 kernel: random gaussian data through quantize_mxfp4_rows; gemv_w4p == gemv_rowss over the dequantised matrix,
   torch.equal, for every fusion; the published table within the hand-off's bound (row sum within SLOT_RTOL of the float64 sum of
   squares of the output row, slots past the grid zero).
5. Random data against fp32 torch on the dequantised weights, within the bf16-rounding bound of tests/test_gpu_gemv_w4.py (_tol)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_gemv_exact import EXCLUDED_CAP, ROWSS_STRIDE, SLOT_RTOL, _normed, _octet_rows, _run_twice, _swiglu_refs
from tests.test_gpu_gemv_w4 import GRID, _rand, _tol, exact_weights, pack, values
from tests.util import assert_close, ints, poisoned, rne

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
G = 16  # SRGPT_MXFP4_GRANULE


def _ops():
    from spatialrgpt_amd import ops
    return ops


def header_layout(codes, sbytes):
    """the packed array by the byte-offset formula of include/srgpt.h, on the CPU: codes uint8 [R, K / 2], sbytes uint8 [R, K / 32]"""
    R, K = codes.shape[0], codes.shape[1] * 2
    cells, gran = K // 128, (R + G - 1) // G
    out = torch.zeros(gran * cells * 68 * G, dtype=torch.uint8)
    out.view(gran * cells, 68 * G)[:, 64 * G:] = 127  # rows past the matrix: scale byte 127 (their codes: 0)
    n = torch.arange(R)[:, None]
    k = 2 * torch.arange(K // 2)[None, :]  # the even k of a byte; k + 1 is its high nibble
    cell = (n // G) * cells + k // 128
    out[cell * 68 * G + ((k % 32) // 8 * G + n % G) * 16 + (k % 128) // 32 * 4 + (k % 8) // 2] = codes
    k = 32 * torch.arange(K // 32)[None, :]
    cell = (n // G) * cells + k // 128
    out[cell * 68 * G + 64 * G + (n % G) * 4 + (k % 128) // 32] = sbytes
    return out


def sentinel_behind(t, extra=4096, value=0xA5):
    """a uint8 device buffer of t.numel() + extra bytes filled with `value`; -> (buffer, its first t.numel() bytes shaped like t)"""
    buf = torch.full((t.numel() + extra,), value, dtype=torch.uint8, device=DEV)
    return buf, buf[:t.numel()].view(t.shape)


def packed_on_device(code, sbytes, swiglu=False):
    """codes [R, K] (0 .. 15) and scale bytes -> the packed copy, made from poisoned inputs, with a poisoned tail behind it"""
    ops = _ops()
    w4, sc = poisoned(pack(code), rows_after=5, poison=0xFF), poisoned(sbytes, rows_after=5, poison=0xFF)
    pk = ops.pack_mxfp4(w4.contiguous(), sc.contiguous(), swiglu=swiglu)
    buf, view = sentinel_behind(pk, value=0xFF)  # 0xFF: code -6 pairs and a NaN scale behind the array
    view.copy_(pk)
    return view


# ------------------------------------------------------------------------------------------------ 1. the layout
@pytest.mark.parametrize("N,K,swiglu", [(N, K, False) for N in (1, 17, 64) for K in (128, 384, 1408)] + [(16, 128, True), (48, 384, True)])
def test_round_trip_and_header_formula(N, K, swiglu):
    ops = _ops()
    R = 2 * N if swiglu else N
    g = torch.Generator().manual_seed(31 * N + K)
    codes = torch.randint(0, 256, (R, K // 2), generator=g).to(torch.uint8)
    sbytes = torch.randint(0, 256, (R, K // 32), generator=g).to(torch.uint8)  # the layout moves bytes: every value
    w4, sc = poisoned(codes, rows_after=5, poison=0xFF).contiguous(), poisoned(sbytes, rows_after=5, poison=0xFF).contiguous()
    nbytes = ops.mxfp4_packed_bytes(N, K, swiglu)
    assert nbytes == (R + G - 1) // G * (K // 128) * 68 * G
    from spatialrgpt_amd import _lib as L
    buf, pk = sentinel_behind(torch.empty(nbytes, dtype=torch.uint8))
    L.check(L.load().srgpt_pack_mxfp4(w4.data_ptr(), sc.data_ptr(), pk.data_ptr(), N, K, int(swiglu), None))
    torch.cuda.synchronize()
    assert bool((buf[nbytes:] == 0xA5).all()), "written behind the packed array"
    assert torch.equal(pk.cpu(), header_layout(codes, sbytes)), "the packed array is not the header's layout"
    assert torch.equal(ops.pack_mxfp4(w4, sc, swiglu=swiglu), pk)
    cbuf, c_out = sentinel_behind(codes)
    sbuf, s_out = sentinel_behind(sbytes)
    ops.unpack_mxfp4(pk, N, K, swiglu, out=(c_out, s_out))
    assert torch.equal(c_out.cpu(), codes) and torch.equal(s_out.cpu(), sbytes), "the round trip is not exact"
    assert bool((cbuf[codes.numel():] == 0xA5).all()) and bool((sbuf[sbytes.numel():] == 0xA5).all()), "written behind an unpacked array"


def test_shapes_outside_the_domain_are_refused():
    ops = _ops()
    z = lambda r, c: torch.zeros((r, c), dtype=torch.uint8, device=DEV)
    assert ops.mxfp4_packed_bytes(16, 96) == 0 and ops.mxfp4_packed_bytes(24, 128, True) == 0
    with pytest.raises(ValueError):
        ops.pack_mxfp4(z(16, 48), z(16, 3))  # K = 96
    with pytest.raises(ValueError):
        ops.pack_mxfp4(z(48, 64), z(48, 4), swiglu=True)  # 24 gate rows: off the granule
    with pytest.raises(ValueError):
        ops.gemv_w4p(torch.zeros((2, 96), dtype=BF16, device=DEV), z(1, 4096).flatten(), 16)


# ------------------------------------------------------------------------------------------------ 2. the table
def test_every_code_under_five_scale_bytes():
    ops = _ops()
    sb = (2, 64, 127, 190, 252)
    K = 256
    for k in (0, 1, 37, 129):  # low nibble, high nibble, another k step / lane group, the second cell (a second 16-byte load)
        code = torch.zeros((16 * len(sb), K), dtype=torch.int64)
        sbytes = torch.full((16 * len(sb), K // 32), 127, dtype=torch.uint8)
        for i, b in enumerate(sb):
            code[16 * i:16 * i + 16, k] = torch.arange(16)
            sbytes[16 * i:16 * i + 16, k // 32] = b
        want = values(code, sbytes)
        table = want[:, k].float().to(BF16)  # float64 -> fp32 is exact here; then ONE rounding to bf16 (exact too: the domain)
        assert bool(torch.isfinite(table.float()).all()) and torch.equal(table.double(), want[:, k])
        pk = packed_on_device(code, sbytes)
        x = torch.zeros((3, K), dtype=BF16)
        x[2, k] = 1.0
        out = ops.gemv_w4p(poisoned(x), pk, code.shape[0]).cpu()
        for r in (out[2].float() != table.float()).nonzero().flatten().tolist():  # the figures before the assertions
            print("k = %d: code %d under byte %d gives %r, the table says %r" % (k, r % 16, sb[r // 16], float(out[2, r]), float(table[r])))
        assert torch.equal(out[2].float(), table.float()), "srgpt_gemv_w4p with a one-hot x, k = %d" % k  # by value: code 8 is a zero
        assert bool((out[:2] == 0).all()), "the rows of zeros, k = %d" % k


# ------------------------------------------------------------------------------------------------ 3. exact data
def swiglu_data(B, N, K, seed):
    """CPU: tests/test_gpu_gemv_w4.py's SwiGLU construction for N gate + N up rows -> (codes, scale bytes, x float64, ref, alt, tally)"""
    what = "B=%d N=%d K=%d swiglu" % (B, N, K)
    x64 = ints((B, K), 8, seed)
    code, sbytes = exact_weights(2 * N, K, seed + 2, gate_rows=N)
    acc = x64 @ values(code, sbytes).T
    assert torch.equal(acc.float().double(), acc)
    tally = {}
    ref, alt = _swiglu_refs(acc[:, :N].float(), acc[:, N:].float(), what, tally)
    return code, sbytes, x64, ref, alt, tally["swiglu excluded"]


def exact_case(B, N, K, seed, variants):
    ops = _ops()
    what0 = "B=%d N=%d K=%d" % (B, N, K)
    assert 4 * 96 * K < 2 ** 24 and 16 * 84 * K < 2 ** 24
    eps = 1e-5
    for variant in variants:
        what = what0 + " " + variant
        if variant == "swiglu":
            code, sbytes, x64, ref, alt, (n, total) = swiglu_data(B, N, K, seed)
            assert n <= max(EXCLUDED_CAP * total, 1), "%s: %d of %d elements within the band of a rounding boundary" % (what, n, total)
            pk, x_d = packed_on_device(code, sbytes, swiglu=True), poisoned(x64.to(BF16))
            _run_twice(lambda out: ops.gemv_w4p(x_d, pk, 2 * N, swiglu=True, out=out), B, N, BF16, ref.to(BF16).to(DEV), alt.to(BF16).to(DEV), what)
            continue
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
        code, sbytes = exact_weights(N, K, seed + 2)
        acc = xe @ values(code, sbytes).T
        assert torch.equal(acc.float().double(), acc)
        prod = acc.float()
        res_i = ints((B, N), 256, seed + 3)
        refs = {"plain": rne(prod), "res": rne(rne(prod) + res_i.float())}
        res_d = poisoned(res_i.to(BF16))
        pk = packed_on_device(code, sbytes)
        for epi in ("plain", "res"):
            for out_f32 in (False, True):
                odt = F32 if out_f32 else BF16
                r = res_d if epi == "res" else None
                call = lambda out, r=r, out_f32=out_f32: ops.gemv_w4p(x_d, pk, N, norm_w, eps, r, out=out, out_f32=out_f32)
                _run_twice(call, B, N, odt, refs[epi].to(BF16).to(odt).to(DEV), None, "%s, %s%s" % (what, epi, " -> fp32" if out_f32 else ""))


EXACT_B, EXACT_K = (2, 3, 4, 5, 8, 9, 16, 17), (128, 384, 2048, 2176)


def exact_seed(B, N, K):
    return 1000 * B + 7 * N + K


@pytest.mark.parametrize("B", EXACT_B)
@pytest.mark.parametrize("K", EXACT_K)
def test_exact_products(B, K):
    """B: every NI (2, 4, 8 staged row pairs) with full and partly filled tiles, and a call of 16 + 1 rows.  K: less than a 256-k slice
    (one cell), a slice and a half, each of eight waves owning one slice, a ragged last wave (8.5 slices).  N: fewer rows than a
    granule, a partly filled second granule, two and a half tiles, whole tiles."""
    for N in (1, 17, 40, 64):
        exact_case(B, N, K, exact_seed(B, N, K), ("plain", "norm"))
    for N in (16, 48):
        exact_case(B, N, K, exact_seed(B, N, K), ("swiglu",))


# ------------------------------------------------------------------------------------------------ 4. the bits of the bf16 kernel
BITS_SHAPES = [(2, 768, 512, False), (4, 512, 512, False), (3, 1408, 512, True), (8, 512, 1408, False), (16, 130, 384, False),
               (5, 4096, 4096, False)]


@functools.lru_cache(maxsize=None)
def random_case(B, N, K, swiglu):
    """one quantised random matrix per shape, shared by the tests below and left unchanged"""
    ops = _ops()
    R = 2 * N if swiglu else N
    x, w = _rand((B, K), BF16, 21), _rand((R, K), BF16, 22, 0.03)
    codes, scales, deq = ops.quantize_mxfp4_rows(w.to(DEV))
    assert int(scales.min()) >= 2 and int(scales.max()) <= 252  # far inside the kernel's scale-byte domain
    assert torch.equal(ops.dequant_mxfp4(codes, scales), deq)
    return x.to(DEV), codes, scales, deq, ops.pack_mxfp4(codes, scales, swiglu=swiglu)


def skinny_grid(N, norm):
    """gemv_skinny_launch's grid over a packed MXFP4 array (gemv_route.h)"""
    from spatialrgpt_amd import _lib as L
    cus = int(L.load().srgpt_device_cus())
    blocks = cus if norm and (N + cus - 1) // cus <= 32 else 2 * cus
    cw = (max((N + blocks - 1) // blocks, 16) + G - 1) // G * G
    return (N + cw - 1) // cw


@pytest.mark.parametrize("B,N,K,swiglu", BITS_SHAPES)
def test_bits_of_the_bf16_kernel_on_the_dequantised_matrix(B, N, K, swiglu):
    ops = _ops()
    x, codes, scales, deq, pk = random_case(B, N, K, swiglu)
    R = deq.shape[0]
    g = (1 + 0.1 * _rand((K,), F32, 23)).to(BF16).to(DEV)
    eps = 1e-5

    def both(what, **kw):
        got, want = ops.gemv_w4p(x, pk, R, swiglu=swiglu, **kw), ops.gemv_rowss(x, w=deq, swiglu=swiglu, **kw)
        assert got.dtype == want.dtype and torch.equal(got, want), "%s: %d of %d elements differ from the bf16 kernel" % (
            what, int((got != want).sum()), got.numel())
        return got

    both("plain")
    both("norm", norm_w=g, eps=eps)
    # the statistics hand-off in: h and its table from a publishing product (a bf16 square matrix with the residual add)
    wsq = _rand((K, K), BF16, 25, 0.03).to(DEV)
    h, table = ops.gemv_rowss(x, w=wsq, residual=x, publish=True)
    got = ops.gemv_w4p(h, pk, R, norm_w=g, eps=eps, swiglu=swiglu, rowss_in=table)
    assert torch.equal(got, ops.gemv_rowss(h, w=deq, norm_w=g, eps=eps, swiglu=swiglu, rowss_in=table)), "norm with rowss_in"
    if swiglu:
        return
    r = _rand((B, N), BF16, 24).to(DEV)
    both("residual", residual=r)
    both("fp32 out", out_f32=True)
    both("residual, fp32 out", residual=r, out_f32=True)
    both("norm, residual", norm_w=g, eps=eps, residual=r)
    # the hand-off out: the same output bits, the table within the hand-off's bound
    out, t = ops.gemv_w4p(x, pk, R, residual=r, publish=True)
    assert torch.equal(out, ops.gemv_rowss(x, w=deq, residual=r)), "publishing changes the output"
    want = out.double().pow(2).sum(1).cpu()
    t = t.cpu()
    err = (t.double().sum(1) - want).abs() / want
    print("rowss_out B=%d N=%d K=%d: row-sum error %.3g (bound %.3g)" % (B, N, K, float(err.max()), SLOT_RTOL))
    assert t.shape == (B, ROWSS_STRIDE) and bool((err <= SLOT_RTOL).all())
    assert bool((t[:, skinny_grid(N, False):] == 0).all()), "slots past the grid"


# ------------------------------------------------------------------------------------------------ 5. random data
@pytest.mark.parametrize("B,N,K,swiglu", BITS_SHAPES)
def test_random_data_vs_torch_on_dequantised_weights(B, N, K, swiglu):
    ops = _ops()
    x, codes, scales, deq, pk = random_case(B, N, K, swiglu)
    R = deq.shape[0]
    xc, wq = x.cpu(), deq.float().cpu()
    g = (1 + 0.1 * _rand((K,), F32, 23)).to(BF16)
    xf = xc.float()
    xn = g * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)).to(BF16)
    if swiglu:
        for what, xi, kw in (("swiglu", xc, {}), ("rmsnorm+swiglu", xn, dict(norm_w=g.to(DEV), eps=1e-5))):
            gate, up = (xi.float() @ wq[:N].T).to(BF16), (xi.float() @ wq[N:].T).to(BF16)
            refs = F.silu(gate.float()).to(BF16).float() * up.float()
            assert_close(ops.gemv_w4p(x, pk, R, swiglu=True, **kw), refs, _tol(refs, BF16), 0, what + " gemv_w4p")
        return
    ref = xc.float() @ wq.T
    r = _rand((B, N), BF16, 24)
    assert_close(ops.gemv_w4p(x, pk, R), ref, _tol(ref, BF16), 0, "gemv_w4p")
    assert_close(ops.gemv_w4p(x, pk, R, residual=r.to(DEV)), ref.to(BF16).float() + r.float(), _tol(ref, BF16, 2), 0, "gemv_w4p+res")
    lo = ops.gemv_w4p(x, pk, R, out_f32=True)
    assert lo.dtype == F32
    assert_close(lo, ref, _tol(ref, BF16), 0, "gemv_w4p f32")
    refn = xn.float() @ wq.T
    assert_close(ops.gemv_w4p(x, pk, R, norm_w=g.to(DEV), eps=1e-5), refn, _tol(refn, BF16), 0, "rmsnorm+gemv_w4p")
    # consistency with the VALU kernel over the row-major codes (the one-row step's kernel)
    assert_close(ops.gemv_w4p(x, pk, R), ops.gemv_w4(x, codes, scales).float().cpu(), _tol(ref, BF16, 2), 0, "w4p vs w4")
