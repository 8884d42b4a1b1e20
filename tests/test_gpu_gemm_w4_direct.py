"""The `_direct` W4A16 prefill products (srgpt_gemm_w4_direct, _norm_direct, _swiglu_direct, _rope_kv_append_direct: gemm.hip,
gemm288.hip) against their bf16 counterparts on ops.dequant_mxfp4 of the same codes AND against the plain W4 entries: every output
compared with torch.equal on the BITS (integer views).  No tolerances: the contract is equality with the bf16 kernel.

Data, surroundings and guards are tests/test_gpu_gemm_w4.py's (imported): codes and scales sit inside buffers poisoned with code
byte 0xFF and scale byte 255, outputs inside sentinel-filled tensors, split products run once more on a caller-owned NaN workspace
of exactly the slabs, and the `expand` scratch is NULL or a sentinel-filled buffer that must come back untouched wherever the codes
are multiplied in the kernel -- here that includes the whole-M kernel (W4 instance of gemm_bf16_288_kernel) and its fused SwiGLU
form.  Every case asserts its route and `direct_in_kernel` through tests/gemm_w4_direct_route_cli.cpp at the device's CU count with
the workspace actually passed (256 CUs; skipped at another count), and that ops.gemm_w4_in_kernel(..., direct=True) agrees."""
import subprocess

import pytest
import torch

from tests.test_gpu_gemm_w4 import (BF16, DEV, F32, SCALE_BYTES, _bits_equal, _check_expand, _expand_arg, _operands, _owned_ws,
                                    _sentinel_flat)
from tests.util import SENTINEL, _build_route_cli, check_guarded, guarded

pytestmark = pytest.mark.gpu


def _ops():
    from spatialrgpt_amd import _lib, ops
    return ops, _lib


@pytest.fixture(scope="module")
def route_cli(tmp_path_factory):
    exe = _build_route_cli(tmp_path_factory.mktemp("gemm_w4_direct_route"), "gemm_w4_direct_route_cli")

    def run(entry, M, N, K, have_ws, ws_bytes, cus):
        out = subprocess.run([exe, str(cus)], input="%s %d %d %d %d %d\n" % (entry, M, N, K, have_ws, ws_bytes), capture_output=True,
                             text=True, check=True).stdout.split()
        return (out[0], int(out[1]), int(out[2]), int(out[3])), int(out[7])

    return run


def _assert_route(route_cli, entry, M, N, K, want, direct_in_kernel):
    """want = (family, bm, nbuf, splits) at 256 CUs with ops.py's workspace for the product; -> the split count"""
    ops, L = _ops()
    cus = L.load().srgpt_device_cus()
    if cus != 256:
        pytest.skip("the routes of these cases are recorded for 256 CUs, this device has %d" % cus)
    rows = 2 * N if entry == "swiglu_w4" else N
    p, nbytes = ops._ws_arg(torch.device(DEV, torch.cuda.current_device()), M, rows)
    got, dik = route_cli(entry, M, N, K, int(p is not None), nbytes, cus)
    what = "%s M=%d N=%d K=%d" % (entry, M, N, K)
    assert got == tuple(want), "%s takes %s, the case exists for %s" % (what, got, tuple(want))
    assert dik == direct_in_kernel, "%s: codes in the kernel (direct) = %d, the case exists for %d" % (what, dik, direct_in_kernel)
    assert ops.gemm_w4_in_kernel(M, N, K, swiglu=entry == "swiglu_w4", direct=True) == bool(direct_in_kernel), \
        what + ": srgpt_gemm_w4_direct_in_kernel disagrees"
    return got[3]


W288 = "whole_m_288"
# (M, N, K), (family, bm, nbuf, splits) at 256 CUs, codes multiplied in the kernel by the `_direct` entry
PRODUCTS = [
    ((272, 24576, 1024), (W288, 272, 3, 1), 1),   # un-split, 16 tiles (the first case to run on a new build)
    ((259, 6144, 4160), (W288, 272, 3, 5), 1),    # 5 splits of 13 tiles (an odd count per split)
    ((225, 16384, 1536), (W288, 272, 3, 2), 1),
    ((259, 3072, 8192), (W288, 272, 3, 8), 1),
    ((240, 98304, 256), (W288, 272, 3, 1), 1),    # four tiles: the prologue requests all of them; no workspace
    ((256, 24576, 1024), (W288, 272, 3, 1), 1),   # no tail group (has_tail false)
    ((257, 24576, 1024), (W288, 272, 3, 1), 1),   # one tail row
    ((259, 16400, 1536), (W288, 272, 3, 2), 1),   # N % 128 == 16: the last column tile clamps 112 rows beside poisoned bytes
    ((259, 6144, 4288), (W288, 272, 3, 5), 1),    # 67 tiles: four splits of 14, the last of 11 (odd), its table shorter
    ((576, 600, 2048), ("tile_256", 256, 2, 4), 0),  # 256 x 256 tiles: still the expansion
    ((259, 6144, 4128), ("glds", 96, 2, 3), 0),      # K % 64 == 32: still the expansion
]


@pytest.mark.parametrize("shape,route,in_kernel", PRODUCTS, ids=["%dx%dx%d" % s for s, _, _ in PRODUCTS])
def test_gemm_w4_direct_equals_gemm_on_the_dequantised_matrix(route_cli, shape, route, in_kernel):
    ops, L = _ops()
    M, N, K = shape
    what = "gemm_w4 direct M=%d N=%d K=%d" % shape
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
        _, pview = guarded(M, N, ldc, odt)
        ops.gemm_w4(a, codes, sc, residual=residual, out=pview, out_f32=out_f32)
        assert _bits_equal(pview.clone(), ref), tag + ": the plain entry differs from the bf16 product"
        for with_scratch in (False, True):
            buf, view = guarded(M, N, ldc, odt)
            if with_scratch or not in_kernel:
                alloc, expand = _expand_arg(in_kernel, N, K)
            else:
                alloc, expand = None, None  # NULL: the kernel multiplies the codes
            ops.gemm_w4(a, codes, sc, residual=residual, out=view, out_f32=out_f32, expand=expand, direct=True)
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
        ops.gemm_w4(a, codes, sc, residual=res, out=view, expand=expand, ws=ws, direct=True)
        assert _bits_equal(view.clone(), ref), what + ", caller-owned workspace"
        check_guarded(buf, view, ref, what + ", caller-owned workspace")
        assert bool((alloc_ws[ws.numel():].view(torch.int32) == SENTINEL[F32][1]).all()), what + ": written behind the workspace"
        _check_expand(alloc, in_kernel, deq, what + ", caller-owned workspace")


def test_gemm_w4_direct_needs_the_scratch_where_it_expands(route_cli):
    ops, L = _ops()
    M, N, K = 259, 6144, 4128
    _assert_route(route_cli, "gemm_w4", M, N, K, ("glds", 96, 2, 3), 0)
    a, codes, sc = _operands(M, N, K, seed=3)
    out = torch.empty((M, N), device=DEV, dtype=BF16)
    ws, ws_bytes = ops._ws_arg(a.device, M, N)
    rc = L.load().srgpt_gemm_w4_direct(a.data_ptr(), codes.data_ptr(), sc.data_ptr(), None, out.data_ptr(), M, N, K, K, N, 0, None, ws,
                                       ws_bytes, None)
    assert rc == L.ERR_ARG and b"scratch" in L.load().srgpt_last_error()


# (259, 4096, 14336): the 8B down_proj -- 8 splits of 28 tiles (the widest scale range per block of the model), the norm in the reduction
def test_gemm_w4_norm_direct_equals_gemm_norm(route_cli):
    ops, L = _ops()
    M, N, K = 259, 4096, 14336
    what = "gemm_w4_norm direct M=%d N=%d K=%d" % (M, N, K)
    _assert_route(route_cli, "gemm_w4", M, N, K, (W288, 272, 3, 8), 1)
    a, codes, sc = _operands(M, N, K, seed=11 + M + N + K)
    deq = ops.dequant_mxfp4(codes, sc)
    g = torch.Generator(device=DEV).manual_seed(5)
    res = (torch.randn((M, N), device=DEV, generator=g) * 64).to(BF16)
    nw = (torch.rand((N,), device=DEV, generator=g) + 0.5).to(BF16)
    c_ref, y_ref = ops.gemm_norm(a, deq, res, nw, 1e-5)
    assert bool(torch.isfinite(c_ref).all()) and bool(torch.isfinite(y_ref).all())
    c_pl, y_pl = ops.gemm_w4_norm(a, codes, sc, res, nw, 1e-5)
    assert _bits_equal(c_pl, c_ref) and _bits_equal(y_pl, y_ref), what + ": the plain entry"
    cbuf, cview = guarded(M, N, N, BF16)
    ybuf, yview = guarded(M, N, N, BF16)
    ops.gemm_w4_norm(a, codes, sc, res, nw, 1e-5, out=cview, y=yview, direct=True)  # expand NULL
    assert _bits_equal(cview.clone(), c_ref) and _bits_equal(yview.clone(), y_ref), what
    check_guarded(cbuf, cview, c_ref, what + ", C")
    check_guarded(ybuf, yview, y_ref, what + ", Y")
    alloc, expand = _expand_arg(1, N, K)
    x = res.clone()  # in place on the residual stream, as the layer loop calls it; a scratch that must stay untouched
    c2, y2 = ops.gemm_w4_norm(a, codes, sc, x, nw, 1e-5, out=x, expand=expand, direct=True)
    assert c2.data_ptr() == x.data_ptr() and _bits_equal(x, c_ref) and _bits_equal(y2, y_ref), what + ", in place"
    _check_expand(alloc, 1, deq, what)


# 1 x 259 at the 8B q/k/v shape: whole-M kernel, 5 splits, the rotation in the reduction
@pytest.mark.parametrize("off", [False, True])
def test_gemm_w4_rope_kv_append_direct_equals_the_bf16_call(route_cli, off):
    ops, L = _ops()
    from spatialrgpt_amd.config import SrgptConfig as PC
    from spatialrgpt_amd.weights import rope_tables
    B, T, Hq, Hkv, D, K = 1, 259, 32, 8, 128, 4096
    max_pos = 512
    M, N = B * T, (Hq + 2 * Hkv) * D
    what = "gemm_w4_rope_kv_append direct B=%d T=%d N=%d K=%d" % (B, T, N, K)
    _assert_route(route_cli, "gemm_w4", M, N, K, (W288, 272, 3, 5), 1)
    cos_t, sin_t = rope_tables(PC(hidden=Hq * D, heads=Hq, kv_heads=Hkv, rope_theta=500000.0), max_pos, BF16, DEV)
    a, codes, sc = _operands(M, N, K, seed=B + T + K)
    deq = ops.dequant_mxfp4(codes, sc)
    pos0 = torch.tensor([7 * (b + 1) for b in range(B)], dtype=torch.int32, device=DEV) if off else None
    caches = [_sentinel_flat(B * Hkv * max_pos * D).view(B, Hkv, max_pos, D) for _ in range(6)]
    kc_ref, vc_ref, kc, vc, kc_pl, vc_pl = caches
    qkv_ref = ops.gemm_rope_kv_append(a, deq, kc_ref, vc_ref, cos_t, sin_t, B, T, Hq, Hkv, D, pos0=pos0)
    assert bool(torch.isfinite(qkv_ref).all())
    qkv_pl = ops.gemm_w4_rope_kv_append(a, codes, sc, kc_pl, vc_pl, cos_t, sin_t, B, T, Hq, Hkv, D, pos0=pos0)
    assert _bits_equal(qkv_pl, qkv_ref) and _bits_equal(kc_pl, kc_ref) and _bits_equal(vc_pl, vc_ref), what + ": the plain entry"
    buf, view = guarded(M, N, N, BF16)
    alloc, expand = _expand_arg(1, N, K)
    ops.gemm_w4_rope_kv_append(a, codes, sc, kc, vc, cos_t, sin_t, B, T, Hq, Hkv, D, pos0=pos0, qkv=view, expand=expand, direct=True)
    assert _bits_equal(view.clone(), qkv_ref), what + ": the q/k/v buffer"
    assert _bits_equal(kc, kc_ref) and _bits_equal(vc, vc_ref), what + ": the caches"
    check_guarded(buf, view, qkv_ref, what)
    _check_expand(alloc, 1, deq, what)
    kc2, vc2 = (_sentinel_flat(kc.numel()).view(kc.shape) for _ in range(2))  # and with a NULL scratch
    qkv2 = ops.gemm_w4_rope_kv_append(a, codes, sc, kc2, vc2, cos_t, sin_t, B, T, Hq, Hkv, D, pos0=pos0, direct=True)
    assert _bits_equal(qkv2, qkv_ref) and _bits_equal(kc2, kc_ref) and _bits_equal(vc2, vc_ref), what + ", NULL scratch"


# (259, 8192, 256): the fused form at four tiles; (259, 8192, 4096): the fused form at the model's K, 64 tiles of scales (16.25 KiB of
# table under the hand-over's LDS); (37, 1408, 512): gemm + silu_mul on the direct-to-LDS kernel, as the plain entry
SWIGLU = [(259, 8192, 256, ("fused", 0, 0, 1), 1), (259, 8192, 4096, ("fused", 0, 0, 1), 1), (37, 1408, 512, ("glds", 64, 2, 1), 1)]


@pytest.mark.parametrize("M,I,K,route,in_kernel", SWIGLU, ids=["%dx%dx%d" % s[:3] for s in SWIGLU])
def test_gemm_w4_swiglu_direct_equals_gemm_swiglu(route_cli, M, I, K, route, in_kernel):
    ops, L = _ops()
    what = "gemm_w4_swiglu direct M=%d I=%d K=%d" % (M, I, K)
    _assert_route(route_cli, "swiglu_w4", M, I, K, route, in_kernel)
    a, codes, sc = _operands(M, 2 * I, K, seed=M + I + K)
    deq = ops.dequant_mxfp4(codes, sc)
    ref = ops.gemm_swiglu(a, deq)
    assert bool(torch.isfinite(ref).all())
    assert _bits_equal(ops.gemm_w4_swiglu(a, codes, sc), ref), what + ": the plain entry"
    buf, view = guarded(M, I, I, BF16)
    alloc, expand = _expand_arg(in_kernel, 2 * I, K)
    ops.gemm_w4_swiglu(a, codes, sc, out=view, expand=expand, direct=True)
    assert _bits_equal(view.clone(), ref), what
    check_guarded(buf, view, ref, what)
    _check_expand(alloc, in_kernel, deq, what)
    assert _bits_equal(ops.gemm_w4_swiglu(a, codes, sc, direct=True), ref), what + ", NULL scratch"
