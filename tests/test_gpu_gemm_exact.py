"""The prefill GEMM family (gemm.hip, gemm256.hip, gemm288.hip, gemm_f8.hip and the split-K reductions) bit for bit on exact
integer data.

A holds integers in [-7, 7], W in [-8, 8] (both exact in bf16 and in OCP e4m3), bias and residual integers in [-256, 256] (exact
in bf16).  |sum| <= 56 K < 2^24, so every partial sum in every order is an exact fp32 value and a correct kernel has ONE possible
output whatever its tile, K split or summation order: float64 `A @ W.T` on the CPU, then the documented roundings
rnd(acc * wscale + bias), rnd(... + residual) with rnd = round-to-nearest-even to bf16 (`out_f32`: the same value, stored
widened; fp32 operands: no rounding at all).  The fp8 codes' power-of-two scales only move the binary point of those sums.
Every comparison is torch.equal.

Around every operand lie NaNs (the gap of a strided A, the rows behind A / W / residual, the tail of bias and the scales), the
output is a slice of a larger tensor pre-filled with a sentinel bit pattern that must survive outside the slice (ldc = N with
guard rows, ldc = N + 8, and ldc = N + 2 for the split products, which drops the reduction to its scalar kernel), and the
split-K workspace is once the caller's: exactly splits * M * N * 4 bytes of NaN with a sentinel guard behind.

Every case names the route (spatialrgpt_amd/csrc/gemm_route.h) it exists for and asserts it through tests/gemm_route_cli.cpp at
the device's CU count with the workspace bytes actually passed: at 256 CUs another route is a failure, at any other CU count the
case is skipped.  Liveness: for every case the reference alone must tell the documented roundings from three wrong ones (no
intermediate rounding, bias added after the rounding, truncation; for the plain product truncation and ties-away) in at least
1 % of the elements -- except the K = 8 and K = 20 cases, whose sums need no rounding: they pin the mapping and the K tail."""
import pytest
import torch
import torch.nn.functional as F

from tests.util import FP8_NAN, SENTINEL, build_gemm_route_cli
from tests.util import away as _away, check_guarded as _check_guarded, exact_f32 as _exact_f32, guarded as _guarded, ints as _ints
from tests.util import poisoned as _poisoned, rne as _rne, trunc as _trunc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
LIVE_FLOOR = 0.01


def _ops():
    from spatialrgpt_amd import _lib, ops
    return ops, _lib


@pytest.fixture(scope="module")
def route_cli(tmp_path_factory):
    return build_gemm_route_cli(tmp_path_factory.mktemp("gemm_route"))


def _assert_route(route_cli, entry, M, N, K, have_ws, ws_bytes, want):
    """`want` = (family, bm, nbuf, splits, tiles_per_split), recorded at 256 CUs; -> the split count"""
    cus = _ops()[1].load().srgpt_device_cus()
    if cus != 256:
        pytest.skip("the routes of these cases are recorded for 256 CUs, this device has %d" % cus)
    r = route_cli([(entry, M, N, K, int(have_ws), ws_bytes)], cus)[0]
    got = (r["family"], r["bm"], r["nbuf"], r["splits"], r["tps"])
    assert got == tuple(want), "%s M=%d N=%d K=%d ws=%d/%d takes %s, the case exists for %s" % (entry, M, N, K, have_ws, ws_bytes,
                                                                                                got, tuple(want))
    return r["splits"]


# ------------------------------------------------------------------------------------------------ the CPU side
def _epilogue(acc, bias, res, rnd):
    v = rnd(acc if bias is None else acc + bias)
    return v if res is None else rnd(v + res)


def _share(x, ref):
    return float((x != ref).float().mean())


def _assert_live(acc, bias, res, what):
    """the data of this case tells the documented roundings from the wrong ones (module docstring)"""
    plain = _rne(acc)
    shares = {"plain, truncation": _share(_trunc(acc), plain), "plain, ties away": _share(_away(acc), plain)}
    if bias is not None or res is not None:
        ref = _epilogue(acc, bias, res, _rne)
        if res is not None:
            shares["no intermediate rounding"] = _share(_rne((acc if bias is None else acc + bias) + res), ref)
        if bias is not None:
            shares["bias after the rounding"] = _share(_epilogue(_rne(_rne(acc) + bias), None, res, _rne), ref)
        shares["truncation"] = _share(_epilogue(acc, bias, res, _trunc), ref)
    for k, s in shares.items():
        assert s >= LIVE_FLOOR, "%s: '%s' differs from the reference in %.2f %% of the elements only" % (what, k, 100 * s)
    return shares


# ------------------------------------------------------------------------------------------------ the device side
def _owned_ws(nbytes):
    """-> (allocation, workspace): exactly `nbytes` of NaN with 4 KiB of sentinel behind them"""
    n = nbytes // 4
    alloc = torch.full((n + 1024,), float("nan"), dtype=F32, device=DEV)
    alloc[n:].view(torch.int32).fill_(SENTINEL[F32][1])
    return alloc, alloc[:n]


def _run_exact(call, R, Cc, refs, splits, ldcs, ws_bytes, what):
    """call(out, epi, out_f32, ws) writes `out` [R, Cc]; epi = "plain" / "bias_res"; refs[epi] = the expected bf16 (fp32 operands:
    fp32) values on the device.  ws None = whatever the case passes by default."""
    dtype = refs["plain"].dtype
    for epi, out_f32 in (("plain", False), ("bias_res", False), ("bias_res", True)):
        odt = F32 if out_f32 else dtype
        ref = refs[epi].to(odt)  # bf16 -> fp32 is exact
        for ldc in ldcs:
            tag = "%s, %s%s, ldc = N + %d" % (what, epi, " -> fp32" if out_f32 else "", ldc - Cc)
            first = None
            for run in range(2):
                buf, view = _guarded(R, Cc, ldc, odt)
                call(view, epi, out_f32, None)
                got = _check_guarded(buf, view, ref, tag + (", second run" if run else ""))
                if first is not None:
                    assert torch.equal(got.view(SENTINEL[odt][0]), first.view(SENTINEL[odt][0])), tag + ": run-to-run difference"
                first = got
    if splits > 1:  # the caller's workspace: exactly the slabs, NaN before, a guard behind
        assert ws_bytes is None or ws_bytes == splits * R * Cc * 4
        alloc, ws = _owned_ws(splits * R * Cc * 4)
        buf, view = _guarded(R, Cc, Cc, dtype)
        call(view, "bias_res", False, ws)
        _check_guarded(buf, view, refs["bias_res"], what + ", caller-owned workspace")
        assert bool((alloc[ws.numel():].view(torch.int32) == SENTINEL[F32][1]).all()), what + ": written behind the workspace"


def _product_case(route_cli, entry, M, N, K, route, dtype=BF16, ws_bytes=None, res_mod=0, live=True):
    """one product through srgpt_gemm (entry "gemm"), srgpt_gemm_w8 or srgpt_gemm_w8a8 with everything of the module docstring"""
    ops, L = _ops()
    what = "%s %s M=%d N=%d K=%d" % (entry, str(dtype)[6:], M, N, K)
    assert 56 * K + 512 < 2 ** 24
    splits = 1
    if route is not None:
        if ws_bytes is not None:
            have_ws, nbytes = True, ws_bytes
        else:
            p, nbytes = ops._ws_arg(torch.device(DEV, torch.cuda.current_device()), M, N)  # what the wrappers pass by default
            have_ws = p is not None
        splits = _assert_route(route_cli, entry, M, N, K, have_ws, nbytes, route)
    a_i, w_i = _ints((M, K), 7, M + 3 * N + K), _ints((N, K), 8, M + N + 7 * K)
    bias_i, res_i = _ints((N,), 256, N + K), _ints((res_mod or M, N), 256, M + N)
    acc = _exact_f32(a_i @ w_i.T)
    bias, res = bias_i.float(), res_i.float().repeat(M // res_mod, 1) if res_mod else res_i.float()
    rnd = _rne if dtype == BF16 else (lambda x: x)
    if live and dtype == BF16:
        _assert_live(acc, bias, res, what)
    refs = {"plain": rnd(acc).to(dtype).to(DEV), "bias_res": _epilogue(acc, bias, res, rnd).to(dtype).to(DEV)}
    edt = dtype if entry == "gemm" else BF16
    bias_d, res_d = _poisoned(bias_i.to(edt)), _poisoned(res_i.to(edt))
    if entry == "gemm":
        a_d, w_d = _poisoned(a_i.to(dtype), col0=8, cols_after=8), _poisoned(w_i.to(dtype), rows_after=5)
    else:  # fp8 codes and power-of-two scales from the host; they must give back the integers
        w8, wscale, deq = ops.quantize_fp8_rows(w_i.to(BF16))
        assert torch.equal(deq.double(), w_i)
        assert torch.equal(w8.view(torch.float8_e4m3fn).float().double() * wscale.double()[:, None], w_i)
        w_d, wscale_d = _poisoned(w8, rows_after=5, poison=FP8_NAN), _poisoned(wscale)
        if entry == "gemm_w8":
            a_d = _poisoned(a_i.to(BF16), col0=8, cols_after=8)
        else:
            a8, ascale, _ = ops.quantize_fp8_rows(a_i.to(BF16))
            assert torch.equal(a8.view(torch.float8_e4m3fn).float().double() * ascale.double()[:, None], a_i)
            a_d, ascale_d = _poisoned(a8, col0=16, cols_after=16, poison=FP8_NAN), _poisoned(ascale)
    default_ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=DEV) if ws_bytes is not None else None

    def call(out, epi, out_f32, ws):
        b, r = (bias_d, res_d) if epi == "bias_res" else (None, None)
        ws = default_ws if ws is None else ws
        if entry == "gemm":
            ops.gemm(a_d, w_d, b, r, out=out, out_f32=out_f32, res_mod=res_mod if r is not None else 0, ws=ws)
        elif entry == "gemm_w8":
            ops.gemm_w8(a_d, w_d, wscale_d, b, r, out=out, out_f32=out_f32, ws=ws)
        else:
            ops.gemm_w8a8(a_d, ascale_d, w_d, wscale_d, b, r, out=out, out_f32=out_f32, ws=ws)

    ldcs = (N, N + 8) + ((N + 2,) if splits > 1 else ())
    _run_exact(call, M, N, refs, splits, ldcs, ws_bytes, what)


GLDS, WHOLE_M, T256 = "glds", "whole_m_288", "tile_256"

# M, N, K, workspace bytes (None: what ops.py passes -- 32 M N bytes of the shared pool, nothing when M N > 2^24), the route at
# 256 CUs (family, rows of a tile, LDS buffers, K splits, K tiles per split), what the case pins
BF16_CASES = [
    (33, 72, 8, None, (GLDS, 64, 2, 1, 1), "one ragged K tile only (mapping and tail: no rounding)"),
    (64, 64, 64, None, (GLDS, 64, 2, 1, 1), "one whole tile"),
    (97, 130, 200, None, (GLDS, 64, 2, 1, 4), "ragged M, N, K"),
    (128, 49152, 64, None, (GLDS, 64, 1, 1, 1), "single-buffer 64-row tiles"),
    (130, 200, 136, None, (GLDS, 96, 2, 1, 3), "ragged K through registers"),
    (288, 640, 64, None, (GLDS, 96, 2, 1, 1), "exact 96-row tiles"),
    (2305, 3456, 256, None, (GLDS, 96, 1, 1, 4), "single-buffer 96-row tiles"),
    (1300, 12288, 72, None, (GLDS, 128, 1, 1, 2), "128-row tiles, ragged K"),
    (259, 384, 1032, None, (GLDS, 96, 2, 2, 9), "uneven split (9 + 8 of 17 tiles), the ragged K tile in the last split"),
    (259, 387, 1024, None, (GLDS, 96, 2, 2, 8), "N % 4 != 0: scalar reduction"),
    (257, 128, 2048, None, (GLDS, 96, 2, 4, 8), "splitk_reduce4<., 4> at its limit"),
    (100, 264, 4304, None, (GLDS, 64, 2, 8, 9), "splitk_reduce4<., 8>, a last split of 5 of 68 tiles"),
    (259, 6144, 4160, None, (WHOLE_M, 272, 3, 5, 13), "odd tile count (65), the ring wraps mid-split"),
    (225, 16384, 1536, None, (WHOLE_M, 272, 3, 2, 12), "no tail rows"),
    (259, 3072, 8192, None, (WHOLE_M, 272, 3, 8, 16), "8 splits"),
    (272, 24576, 1024, None, (WHOLE_M, 272, 3, 1, 16), "un-split, the full 272 rows"),
    (240, 98304, 256, None, (WHOLE_M, 272, 3, 1, 4), "no workspace (M N > 2^24), minimum K: 4 tiles"),
    (3841, 3841, 256, None, (T256, 256, 2, 1, 4), "minimum K (4 tiles): prologue / tail only, one block per tile"),
    (4000, 4400, 2048, None, (T256, 256, 2, 1, 32), "no workspace, 272 tiles > CUs: the persistent form"),
    (576, 600, 2048, None, (T256, 256, 2, 4, 8), "4 splits"),
    (1000, 6000, 2112, None, (T256, 256, 2, 3, 11), "3 splits of 33 tiles"),
    (1000, 3000, 2048, 24000000, (T256, 256, 2, 2, 16), "the workspace-limited branch: 4 splits wanted, 2 slabs fit"),
]


@pytest.mark.parametrize("M,N,K,ws_bytes,route,what", BF16_CASES, ids=["%dx%dx%d" % c[:3] for c in BF16_CASES])
def test_gemm_bf16_exact(route_cli, M, N, K, ws_bytes, route, what):
    _product_case(route_cli, "gemm", M, N, K, route, ws_bytes=ws_bytes, live=K != 8)


@pytest.mark.parametrize("M,N,K", [(130, 200, 136), (33, 72, 8), (65, 65, 20)])
def test_gemm_f32_exact(route_cli, M, N, K):
    """gemm_f32_simple: the same data, no rounding anywhere (K = 8 and K = 20: mapping and tail)"""
    _product_case(route_cli, "gemm", M, N, K, None, dtype=F32)


@pytest.mark.parametrize("M,N,K,res_mod,route", [(96, 80, 64, 32, (GLDS, 96, 2, 1, 1)),
                                                 (300, 200, 1024, 100, (GLDS, 64, 2, 2, 8))])  # res_mod: scalar reduction
def test_gemm_row_modulo_residual_exact(route_cli, M, N, K, res_mod, route):
    _product_case(route_cli, "gemm", M, N, K, route, res_mod=res_mod)


@pytest.mark.parametrize("M,N,K,route", [(259, 512, 1024, (T256, 256, 2, 2, 8)), (300, 1000, 512, (T256, 256, 2, 1, 8)),
                                         (64, 300, 2048, (T256, 256, 2, 4, 8)),
                                         (37, 130, 72, None), (210, 64, 160, None)])  # K % 64 != 0: gemm_w8_simple
def test_gemm_w8_exact(route_cli, M, N, K, route):
    _product_case(route_cli, "gemm_w8", M, N, K, route)


@pytest.mark.parametrize("M,N,K,route", [(259, 512, 1024, (T256, 256, 2, 2, 4)), (64, 300, 2048, (T256, 256, 2, 4, 4)),
                                         (300, 520, 256, (T256, 256, 2, 1, 2))])  # K tiles of 128
def test_gemm_w8a8_exact(route_cli, M, N, K, route):
    _product_case(route_cli, "gemm_w8a8", M, N, K, route)


@pytest.mark.parametrize("n_img,g,C,route", [(1, 27, 64, (GLDS, 96, 2, 1, 1)), (2, 6, 64, (GLDS, 96, 2, 1, 1))])
def test_gemm_deconv2x_exact(route_cli, n_img, g, C, route):
    """SRGPT_OUT_DECONV2X: ConvTranspose2d(C, C, 2, 2) as a product with the pixel shuffle in the store, bias per channel, against
    float64 conv_transpose2d (test_gemm_deconv2x of test_gpu_kernels.py has the activation and the tolerance; its grids, with 64
    channels on both: at K = 32 truncation of the product alone shows in 0.7 % of the elements, under the liveness floor)"""
    ops, L = _ops()
    M, N, K = n_img * g * g, 4 * C, C
    what = "deconv2x n_img=%d g=%d C=%d" % (n_img, g, C)
    p, nbytes = ops._ws_arg(torch.device(DEV, torch.cuda.current_device()), M, N)
    assert _assert_route(route_cli, "gemm", M, N, K, p is not None, nbytes, route) == 1
    x_i, wt_i, bias_i = _ints((n_img, g * g, C), 7, g + C), _ints((C, C, 2, 2), 8, g + 2 * C), _ints((C,), 256, C)
    acc = F.conv_transpose2d(x_i.reshape(n_img, g, g, C).permute(0, 3, 1, 2), wt_i, None, stride=2)
    acc = _exact_f32(acc.flatten(2).transpose(1, 2).reshape(-1, C).contiguous())  # channels-last [n_img * 2g * 2g, C]
    bias = bias_i.float()
    _assert_live(acc, bias, None, what)
    refs = {"plain": _rne(acc).to(BF16).to(DEV), "bias_res": _epilogue(acc, bias, None, _rne).to(BF16).to(DEV)}
    a_d = _poisoned(x_i.reshape(-1, C).to(BF16), col0=8, cols_after=8)
    w_d = _poisoned(wt_i.permute(2, 3, 1, 0).reshape(4 * C, C).contiguous().to(BF16), rows_after=5)
    bias_d = _poisoned(bias_i.to(BF16))

    def call(out, epi, out_f32, ws):
        ops.gemm(a_d, w_d, bias_d if epi == "bias_res" else None, out=out, out_f32=out_f32, bias_mod=C, out_mode=L.OUT_DECONV2X,
                 gw=g)

    _run_exact(call, 4 * M, C, refs, 1, (C,), None, what)


# srgpt_gemm_norm: C as above, Y = the norm kernels' output for that C.  The reduction behind each route: splitk_reduce_norm_kernel
# <slabs in flight (4 up to 4 splits, else 8), chunks per thread (2 up to N = 4096, else 4)>
@pytest.mark.parametrize("M,N,K,layer,route", [(259, 384, 1032, False, (GLDS, 96, 2, 2, 9)),     # <4, 2>
                                               (100, 264, 4304, True, (GLDS, 64, 2, 8, 9)),      # <8, 2>
                                               (259, 8192, 2048, True, (GLDS, 96, 2, 2, 16)),    # <4, 4>
                                               (259, 6144, 4160, False, (WHOLE_M, 272, 3, 5, 13))])  # <8, 4>, whole-M kernel
def test_gemm_norm_exact(route_cli, M, N, K, layer, route):
    ops, L = _ops()
    what = "gemm_norm M=%d N=%d K=%d %s" % (M, N, K, "LayerNorm" if layer else "RMSNorm")
    assert 56 * K + 512 < 2 ** 24
    p, nbytes = ops._ws_arg(torch.device(DEV, torch.cuda.current_device()), M, N)
    splits = _assert_route(route_cli, "gemm", M, N, K, p is not None, nbytes, route)
    assert splits > 1
    a_i, w_i = _ints((M, K), 7, M + 3 * N + K), _ints((N, K), 8, M + N + 7 * K)
    bias_i, res_i = (_ints((N,), 256, N + K) if layer else None), _ints((M, N), 256, M + N)
    acc = _exact_f32(a_i @ w_i.T)
    bias, res = (bias_i.float() if layer else None), res_i.float()
    _assert_live(acc, bias, res, what)
    c_ref = _epilogue(acc, bias, res, _rne).to(BF16).to(DEV)
    g = torch.Generator().manual_seed(N)
    a_d, w_d = _poisoned(a_i.to(BF16)), _poisoned(w_i.to(BF16), rows_after=5)  # dense rows: the entry point takes no strides
    res_d, bias_d = _poisoned(res_i.to(BF16)), (_poisoned(bias_i.to(BF16)) if layer else None)
    nw = _poisoned((1 + 0.1 * torch.randn((N,), generator=g)).to(BF16))
    nb = _poisoned(torch.randn((N,), generator=g).to(BF16)) if layer else None
    eps = 1e-6 if layer else 1e-5
    y_ref = ops.layernorm(c_ref, nw, nb, eps) if layer else ops.rmsnorm(c_ref, nw, eps)
    assert bool(torch.isfinite(y_ref).all())
    first = None
    for ws_owned in (False, False, True):  # twice with the shared workspace, once with the caller's
        alloc, ws = _owned_ws(splits * M * N * 4) if ws_owned else (None, None)
        cbuf, c = _guarded(M, N, N, BF16)
        ybuf, y = _guarded(M, N, N, BF16)
        ops.gemm_norm(a_d, w_d, res_d, nw, eps, bias=bias_d, norm_b=nb, out=c, y=y, ws=ws)
        _check_guarded(cbuf, c, c_ref, what + ": C" + (", caller-owned workspace" if ws_owned else ""))
        got = _check_guarded(ybuf, y, y_ref, what + ": Y" + (", caller-owned workspace" if ws_owned else ""))
        if ws_owned:
            assert bool((alloc[ws.numel():].view(torch.int32) == SENTINEL[F32][1]).all()), what + ": written behind the workspace"
        assert first is None or torch.equal(got.view(torch.int16), first.view(torch.int16)), what + ": run-to-run difference"
        first = got
    # in place on the residual stream, as the layer loops call it
    xbuf, x = _guarded(M, N, N, BF16)
    x.copy_(res_d)
    ybuf, y = _guarded(M, N, N, BF16)
    c2, _ = ops.gemm_norm(a_d, w_d, x, nw, eps, bias=bias_d, norm_b=nb, out=x, y=y)
    assert c2.data_ptr() == x.data_ptr()
    _check_guarded(xbuf, x, c_ref, what + ": C over the residual")
    _check_guarded(ybuf, y, y_ref, what + ": Y, C over the residual")
