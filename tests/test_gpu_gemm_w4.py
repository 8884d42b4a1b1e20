"""The W4A16 prefill products (srgpt_gemm_w4, _norm, _swiglu, _rope_kv_append: gemm.hip) against their bf16 counterparts on
ops.dequant_mxfp4 of the same codes: every output compared with torch.equal, on the BITS (integer views), case by case.

Data.  Codes are uniform bytes (all 16 e2m1 values, both zeros).  Scale bytes come from {2, 100, 127, 140, 252} -- the ends of the
documented domain, the quantiser's range and 1.0: each 32-column block of K draws one of them for all rows, and in the blocks that
drew 127 or 140 (block 0 always does) every ROW draws its own of the two, so a scale taken from the wrong row or block is a factor
2^13 or more.  The activations are +-[1, 4) times 2^(127 - byte) of their block (normal bf16 numbers at both ends), so every block
contributes terms of comparable size whatever its scale, nothing overflows, and the fp32 sums round at almost every step: equal
bits need the bf16 instance's k order, accumulators, split ranges and slab order.  The references are asserted finite, so a NaN
can only come from a stray read.
Surroundings.  Codes and scales are slices of larger buffers filled with code byte 0xFF and scale byte 255 (infinity as the
conversion's scale: 0 x inf = NaN).  Outputs are slices of sentinel-filled tensors that must survive outside the slice; the split
products run once more on a caller-owned workspace of exactly splits x M x N x 4 bytes of NaN with a sentinel guard behind; the
`expand` scratch is NULL or a sentinel-filled buffer that must stay untouched where the codes are multiplied in the kernel, and on
the expansion path must hold exactly the dequantised matrix with its guard intact.
Routes.  Every case names the route it exists for and whether the kernel multiplies the codes, and asserts both through
tests/gemm_w4_route_cli.cpp at the device's CU count with the workspace bytes actually passed: at 256 CUs another answer is a
failure, at any other CU count the case is skipped.  The whole-M kernel has no W4 mode (it keeps the expansion), so its rows are
expansion cases; so are the 256 x 256 tiles and K % 64 == 32."""
import subprocess

import pytest
import torch

from tests.util import SENTINEL, _build_route_cli, check_guarded, guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
SCALE_BYTES = (2, 100, 127, 140, 252)


def _ops():
    from spatialrgpt_amd import _lib, ops
    return ops, _lib


@pytest.fixture(scope="module")
def route_cli(tmp_path_factory):
    exe = _build_route_cli(tmp_path_factory.mktemp("gemm_w4_route"), "gemm_w4_route_cli")

    def run(entry, M, N, K, have_ws, ws_bytes, cus):
        out = subprocess.run([exe, str(cus)], input="%s %d %d %d %d %d\n" % (entry, M, N, K, have_ws, ws_bytes), capture_output=True,
                             text=True, check=True).stdout.split()
        return (out[0], int(out[1]), int(out[2]), int(out[3])), int(out[6])

    return run


def _assert_route(route_cli, entry, M, N, K, want, in_kernel):
    """want = (family, bm, nbuf, splits) at 256 CUs with ops.py's workspace for the product; -> the split count"""
    ops, L = _ops()
    cus = L.load().srgpt_device_cus()
    if cus != 256:
        pytest.skip("the routes of these cases are recorded for 256 CUs, this device has %d" % cus)
    rows = 2 * N if entry == "swiglu_w4" else N
    p, nbytes = ops._ws_arg(torch.device(DEV, torch.cuda.current_device()), M, rows)
    got, ik = route_cli(entry, M, N, K, int(p is not None), nbytes, cus)
    what = "%s M=%d N=%d K=%d" % (entry, M, N, K)
    assert got == tuple(want), "%s takes %s, the case exists for %s" % (what, got, tuple(want))
    assert ik == in_kernel, "%s: codes in the kernel = %d, the case exists for %d" % (what, ik, in_kernel)
    assert ops.gemm_w4_in_kernel(M, N, K, swiglu=entry == "swiglu_w4") == bool(in_kernel), what + ": srgpt_gemm_w4_in_kernel disagrees"
    return got[3]


def _inside(t, before, after, poison):
    """the uint8 matrix `t` as a contiguous slice of a larger buffer of `poison` bytes"""
    big = torch.full((before + t.numel() + after,), poison, dtype=torch.uint8, device=DEV)
    big[before:before + t.numel()] = t.reshape(-1)
    return big[before:before + t.numel()].view(t.shape)


def _operands(M, N, K, seed):
    """-> (a [M, K] bf16, codes [N, K / 2], scales [N, K / 32]) as the module docstring describes them"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    nb = K // 32
    table = torch.tensor(SCALE_BYTES, device=DEV)
    base = table[torch.randint(0, 5, (nb,), device=DEV, generator=g)]
    base[0] = 127
    sc = base.expand(N, nb).clone()
    mixed = (base == 127) | (base == 140)
    own = torch.where(torch.randint(0, 2, (N, nb), device=DEV, generator=g) == 1, 127, 140)
    sc[:, mixed] = own[:, mixed]
    mag = torch.rand((M, K), device=DEV, generator=g) * 3 + 1
    sign = torch.randint(0, 2, (M, K), device=DEV, generator=g).float() * 2 - 1
    a = torch.ldexp(mag * sign, (127 - base).repeat_interleave(32).expand(M, K).to(torch.int32)).to(BF16)
    assert bool(torch.isfinite(a).all()) and bool((a.float().abs() >= 2.0 ** -126).all())
    codes = torch.randint(0, 256, (N, K // 2), device=DEV, generator=g, dtype=torch.uint8)
    # 64 bytes in front keep the codes 16-byte aligned; the scales start at an odd address
    return a, _inside(codes, 64, 4096, 0xFF), _inside(sc.to(torch.uint8), 37, 515, 255)


def _sentinel_flat(n, dtype=BF16):
    idt, bits = SENTINEL[dtype]
    t = torch.empty((n,), dtype=dtype, device=DEV)
    t.view(idt).fill_(bits)
    return t


def _bits_equal(x, y):
    idt = {BF16: torch.int16, F32: torch.int32}[x.dtype]
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(idt), y.contiguous().view(idt))


def _expand_arg(in_kernel, N, K):
    """-> (allocation, the `expand` argument): sentinel-filled, N * K elements with 64 guard elements on either side"""
    alloc = _sentinel_flat(N * K + 128)
    return alloc, alloc[64:64 + N * K]


def _check_expand(alloc, in_kernel, deq, what):
    idt, bits = SENTINEL[BF16]
    body = alloc[64:64 + deq.numel()]
    if in_kernel:
        assert bool((alloc.view(idt) == bits).all()), what + ": the scratch was written although the kernel multiplies the codes"
    else:
        assert _bits_equal(body.view(deq.shape), deq), what + ": the scratch does not hold the dequantised matrix"
        assert bool((alloc[:64].view(idt) == bits).all()) and bool((alloc[64 + deq.numel():].view(idt) == bits).all()), \
            what + ": written outside the scratch"


def _owned_ws(nbytes):
    n = nbytes // 4
    alloc = torch.full((n + 1024,), float("nan"), dtype=F32, device=DEV)
    alloc[n:].view(torch.int32).fill_(SENTINEL[F32][1])
    return alloc, alloc[:n]


# (M, N, K), (family, bm, nbuf, splits) at 256 CUs, codes multiplied in the kernel
PRODUCTS = [
    ((33, 72, 64), ("glds", 64, 2, 1), 1),            # one tile, ragged M and N
    ((97, 130, 192), ("glds", 64, 2, 1), 1),          # ragged M, N, three tiles
    ((128, 49152, 64), ("glds", 64, 1, 1), 1),        # single buffer
    ((288, 640, 64), ("glds", 96, 2, 1), 1),          # exact 96-row tiles
    ((2305, 3456, 256), ("glds", 96, 1, 1), 1),       # single buffer
    ((1300, 12288, 128), ("glds", 128, 1, 1), 1),     # 128-row tiles
    ((259, 384, 1088), ("glds", 96, 2, 2), 1),        # uneven split: 9 + 8 of 17 tiles
    ((259, 387, 1024), ("glds", 96, 2, 2), 1),        # N % 4 != 0: scalar reduction
    ((257, 128, 2048), ("glds", 96, 2, 4), 1),
    ((100, 264, 4352), ("glds", 64, 2, 8), 1),        # 8 splits of 9 tiles, the last 5
    ((259, 6144, 4160), ("whole_m_288", 272, 3, 5), 0),   # whole-M kernel: expansion
    ((225, 16384, 1536), ("whole_m_288", 272, 3, 2), 0),
    ((259, 3072, 8192), ("whole_m_288", 272, 3, 8), 0),
    ((272, 24576, 1024), ("whole_m_288", 272, 3, 1), 0),
    ((240, 98304, 256), ("whole_m_288", 272, 3, 1), 0),   # no workspace
    ((576, 600, 2048), ("tile_256", 256, 2, 4), 0),       # 256 x 256 tiles, split: expansion
    ((259, 6144, 4128), ("glds", 96, 2, 3), 0),           # K % 64 == 32 (ragged last tile), split: expansion
]


@pytest.mark.parametrize("shape,route,in_kernel", PRODUCTS, ids=["%dx%dx%d" % s for s, _, _ in PRODUCTS])
def test_gemm_w4_equals_gemm_on_the_dequantised_matrix(route_cli, shape, route, in_kernel):
    ops, L = _ops()
    M, N, K = shape
    what = "gemm_w4 M=%d N=%d K=%d" % shape
    splits = _assert_route(route_cli, "gemm_w4", M, N, K, route, in_kernel)
    a, codes, sc = _operands(M, N, K, seed=M + 3 * N + 7 * K)
    assert len(torch.unique(codes & 15)) == 16 and set(torch.unique(sc).tolist()) <= set(SCALE_BYTES)
    deq = ops.dequant_mxfp4(codes, sc)
    assert bool(torch.isfinite(deq).all())
    res = (torch.randn((M, N), device=DEV, generator=torch.Generator(device=DEV).manual_seed(N + K)) * 64).to(BF16)
    ldc = N + 8
    for residual, out_f32 in ((None, False), (res, False), (res, True)):
        odt = F32 if out_f32 else BF16
        tag = "%s%s%s" % (what, ", residual" if residual is not None else "", " -> fp32" if out_f32 else "")
        _, rview = guarded(M, N, ldc, odt)
        ops.gemm(a, deq, residual=residual, out=rview, out_f32=out_f32)
        ref = rview.clone()
        assert bool(torch.isfinite(ref).all()), tag + ": the reference is not finite"
        for with_scratch in (False, True):
            buf, view = guarded(M, N, ldc, odt)
            if with_scratch or not in_kernel:
                alloc, expand = _expand_arg(in_kernel, N, K)
            else:
                alloc, expand = None, None  # NULL: the kernel multiplies the codes
            ops.gemm_w4(a, codes, sc, residual=residual, out=view, out_f32=out_f32, expand=expand)
            got = view.clone()
            assert _bits_equal(got, ref), "%s: %d of %d elements differ from the bf16 product" % (tag, int((got != ref).sum()), got.numel())
            check_guarded(buf, view, ref, tag)
            if alloc is not None:
                _check_expand(alloc, in_kernel, deq, tag)
    if splits > 1:  # the caller's workspace: exactly the slabs
        alloc_ws, ws = _owned_ws(splits * M * N * 4)
        _, rview = guarded(M, N, N, BF16)
        ops.gemm(a, deq, residual=res, out=rview, ws=ws)
        ref = rview.clone()
        alloc_ws[:ws.numel()].fill_(float("nan"))
        buf, view = guarded(M, N, N, BF16)
        alloc, expand = _expand_arg(in_kernel, N, K)
        ops.gemm_w4(a, codes, sc, residual=res, out=view, expand=expand, ws=ws)
        assert _bits_equal(view.clone(), ref), what + ", caller-owned workspace"
        check_guarded(buf, view, ref, what + ", caller-owned workspace")
        assert bool((alloc_ws[ws.numel():].view(torch.int32) == SENTINEL[F32][1]).all()), what + ": written behind the workspace"
        _check_expand(alloc, in_kernel, deq, what + ", caller-owned workspace")


# (259, 4096, 4096) is the 8B o_proj of the bs = 1 prefill: glds<96, 128, 2>, 4 splits, the norm in the reduction
@pytest.mark.parametrize("shape,route", [((259, 384, 1088), ("glds", 96, 2, 2)), ((259, 4096, 4096), ("glds", 96, 2, 4))])
def test_gemm_w4_norm_equals_gemm_norm(route_cli, shape, route):
    ops, L = _ops()
    M, N, K = shape
    what = "gemm_w4_norm M=%d N=%d K=%d" % shape
    _assert_route(route_cli, "gemm_w4", M, N, K, route, 1)
    a, codes, sc = _operands(M, N, K, seed=11 + M + N + K)
    deq = ops.dequant_mxfp4(codes, sc)
    g = torch.Generator(device=DEV).manual_seed(5)
    res = (torch.randn((M, N), device=DEV, generator=g) * 64).to(BF16)
    nw = (torch.rand((N,), device=DEV, generator=g) + 0.5).to(BF16)
    c_ref, y_ref = ops.gemm_norm(a, deq, res, nw, 1e-5)
    assert bool(torch.isfinite(c_ref).all()) and bool(torch.isfinite(y_ref).all())
    cbuf, cview = guarded(M, N, N, BF16)
    ybuf, yview = guarded(M, N, N, BF16)
    ops.gemm_w4_norm(a, codes, sc, res, nw, 1e-5, out=cview, y=yview)  # expand NULL
    assert _bits_equal(cview.clone(), c_ref) and _bits_equal(yview.clone(), y_ref), what
    check_guarded(cbuf, cview, c_ref, what + ", C")
    check_guarded(ybuf, yview, y_ref, what + ", Y")
    x = res.clone()  # in place on the residual stream, as the layer loop calls it
    c2, y2 = ops.gemm_w4_norm(a, codes, sc, x, nw, 1e-5, out=x)
    assert c2.data_ptr() == x.data_ptr() and _bits_equal(x, c_ref) and _bits_equal(y2, y_ref), what + ", in place"


# 1 x 37 and 3 x 37 at Hq 8 / Hkv 2 / D 64, K 512: un-split, the RoPE launch is separate, codes in the kernel.  1 x 259 at the 8B
# q/k/v shape: whole-M kernel, 5 splits, the rotation in the reduction -- the expansion path.
@pytest.mark.parametrize("B,T,Hq,Hkv,D,K,off,route,in_kernel", [
    (1, 37, 8, 2, 64, 512, False, ("glds", 64, 2, 1), 1), (3, 37, 8, 2, 64, 512, True, ("glds", 64, 2, 1), 1),
    (1, 259, 32, 8, 128, 4096, False, ("whole_m_288", 272, 3, 5), 0), (1, 259, 32, 8, 128, 4096, True, ("whole_m_288", 272, 3, 5), 0)])
def test_gemm_w4_rope_kv_append_equals_the_bf16_call(route_cli, B, T, Hq, Hkv, D, K, off, route, in_kernel):
    ops, L = _ops()
    from spatialrgpt_amd.config import SrgptConfig as PC
    from spatialrgpt_amd.weights import rope_tables
    max_pos = 512
    M, N = B * T, (Hq + 2 * Hkv) * D
    what = "gemm_w4_rope_kv_append B=%d T=%d N=%d K=%d" % (B, T, N, K)
    _assert_route(route_cli, "gemm_w4", M, N, K, route, in_kernel)
    cos_t, sin_t = rope_tables(PC(hidden=Hq * D, heads=Hq, kv_heads=Hkv, rope_theta=500000.0), max_pos, BF16, DEV)
    a, codes, sc = _operands(M, N, K, seed=B + T + K)
    deq = ops.dequant_mxfp4(codes, sc)
    pos0 = torch.tensor([7 * (b + 1) for b in range(B)], dtype=torch.int32, device=DEV) if off else None
    caches = [_sentinel_flat(B * Hkv * max_pos * D).view(B, Hkv, max_pos, D) for _ in range(4)]
    kc_ref, vc_ref, kc, vc = caches
    qkv_ref = ops.gemm_rope_kv_append(a, deq, kc_ref, vc_ref, cos_t, sin_t, B, T, Hq, Hkv, D, pos0=pos0)
    assert bool(torch.isfinite(qkv_ref).all())
    buf, view = guarded(M, N, N, BF16)
    alloc, expand = _expand_arg(in_kernel, N, K)
    ops.gemm_w4_rope_kv_append(a, codes, sc, kc, vc, cos_t, sin_t, B, T, Hq, Hkv, D, pos0=pos0, qkv=view, expand=expand)
    assert _bits_equal(view.clone(), qkv_ref), what + ": the q/k/v buffer"
    assert _bits_equal(kc, kc_ref) and _bits_equal(vc, vc_ref), what + ": the caches"
    check_guarded(buf, view, qkv_ref, what)
    _check_expand(alloc, in_kernel, deq, what)
    if in_kernel:  # and with a NULL scratch
        kc2, vc2 = (_sentinel_flat(kc.numel()).view(kc.shape) for _ in range(2))
        qkv2 = ops.gemm_w4_rope_kv_append(a, codes, sc, kc2, vc2, cos_t, sin_t, B, T, Hq, Hkv, D, pos0=pos0)
        assert _bits_equal(qkv2, qkv_ref) and _bits_equal(kc2, kc_ref) and _bits_equal(vc2, vc_ref), what + ", NULL scratch"


# (259, 8192, 256): the fused form on the whole-M kernel -- the expansion path; (37, 1408, 512): gemm + silu_mul, codes in the kernel
@pytest.mark.parametrize("M,I,K,route,in_kernel", [(259, 8192, 256, ("fused", 0, 0, 1), 0), (37, 1408, 512, ("glds", 64, 2, 1), 1)])
def test_gemm_w4_swiglu_equals_gemm_swiglu(route_cli, M, I, K, route, in_kernel):
    ops, L = _ops()
    what = "gemm_w4_swiglu M=%d I=%d K=%d" % (M, I, K)
    _assert_route(route_cli, "swiglu_w4", M, I, K, route, in_kernel)
    a, codes, sc = _operands(M, 2 * I, K, seed=M + I + K)
    deq = ops.dequant_mxfp4(codes, sc)
    ref = ops.gemm_swiglu(a, deq)
    assert bool(torch.isfinite(ref).all())
    buf, view = guarded(M, I, I, BF16)
    alloc, expand = _expand_arg(in_kernel, 2 * I, K)
    ops.gemm_w4_swiglu(a, codes, sc, out=view, expand=expand)
    assert _bits_equal(view.clone(), ref), what
    check_guarded(buf, view, ref, what)
    _check_expand(alloc, in_kernel, deq, what)
    if in_kernel:
        assert _bits_equal(ops.gemm_w4_swiglu(a, codes, sc), ref), what + ", NULL scratch"
