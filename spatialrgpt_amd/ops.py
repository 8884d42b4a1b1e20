"""Tensor-level wrappers over the C ABI (include/srgpt.h).  torch is used only for device memory and
streams: every arithmetic op below is a HIP kernel from libsrgpt_hip.so, launched on the caller's
current torch stream.  Inputs must be CUDA(HIP) tensors; there is no CPU path."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib as L

_DT = {torch.float32: L.F32, torch.bfloat16: L.BF16}


def dt_code(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise ValueError(f"srgpt kernels support float32 and bfloat16 tensors, got {t.dtype}") from None


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("srgpt ops need tensors on the GPU (no CPU fallback)")


def _same_dtype(op: str, ref: torch.Tensor, **others):
    """The kernels take ONE dtype code per call (the activation's): a weight / bias / residual buffer in another dtype would
    be read with the wrong element size (bf16 weights read as fp32 run 2x past their end).  torch raises a dtype-mismatch
    RuntimeError for the same call; so do we."""
    for name, t in others.items():
        if t is not None and t.dtype != ref.dtype:
            raise RuntimeError(f"{op}: expected {name} to have the activation dtype {ref.dtype}, got {t.dtype}")


def _c(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


_gemm_ws = {}


def _splitk_ws(device, M, N):
    """fp32 split-K workspace (grown on demand, one per device; same-stream reuse is ordered by the stream)."""
    need = 8 * M * N * 4
    t = _gemm_ws.get(device)
    if t is None or t.numel() < need:
        t = torch.empty((need,), device=device, dtype=torch.uint8)
        _gemm_ws[device] = t
    return t


def _ws_arg(device, M, N, enabled=True, ws=None):
    """(pointer, byte count) of the split-K workspace for an [M, N] product as the C ABI takes them; (None, 0) -- no split-K --
    when the caller's condition is off or the slabs would be too large.  `ws`: a caller-owned workspace (any contiguous tensor on
    the device; all of its bytes are offered) in place of the shared one."""
    if ws is not None:
        _dev(ws)
        assert ws.is_contiguous() and ws.data_ptr() % 16 == 0
        return ws.data_ptr(), ws.numel() * ws.element_size()
    if not (enabled and M * N <= (1 << 24)):
        return None, 0
    ws = _splitk_ws(device, M, N)
    return ws.data_ptr(), ws.numel()


def gemm(a, w, bias=None, residual=None, act=L.ACT_NONE, out=None, out_f32=False, bias_mod=0, res_mod=0,
         out_mode=L.OUT_PLAIN, gw=0, out_shape=None, ws=None):
    """act(a @ w.T + bias) + residual.  a [M,K] (row stride may exceed K), w [N,K].  ws: a caller-owned split-K workspace
    (None = the shared one, sized by this module)."""
    _dev(a, w, bias, residual)
    _same_dtype("gemm", a, weight=w, bias=bias, residual=residual)
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K and a.stride(1) == 1 and w.is_contiguous()
    if out is None:
        shape = out_shape if out_shape is not None else (M, N)
        out = torch.empty(shape, device=a.device, dtype=torch.float32 if out_f32 else a.dtype)
    ldc = N if out_mode != L.OUT_PLAIN else out.stride(0) if out.dim() == 2 else N
    ws, ws_bytes = _ws_arg(a.device, M, N, a.dtype == torch.bfloat16, ws)
    L.check(L.load().srgpt_gemm(_p(a), _p(w), _p(bias), _p(residual), _p(out), M, N, K, a.stride(0), ldc, act,
                                bias_mod, res_mod, int(out_f32), out_mode, gw, ws, ws_bytes,
                                dt_code(a), _stream()))
    return out


def gemm_norm(a, w, residual, norm_w, eps, bias=None, norm_b=None, out=None, y=None, ws=None):
    """(a @ w.T + bias + residual, norm(that)): the tail of an attention / MLP block and the next block's input norm in one call --
    RMSNorm (norm_b None: Llama) or LayerNorm (ViT).  `out` may be `residual` (in place), `y` may be `a`.  Bit-identical to gemm(...)
    followed by rmsnorm(...) / layernorm(...).  ws: as for gemm."""
    _dev(a, w, residual, norm_w, bias, norm_b)
    _same_dtype("gemm_norm", a, weight=w, residual=residual, norm_weight=norm_w, bias=bias, norm_bias=norm_b)
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K and a.is_contiguous() and w.is_contiguous() and (residual is None or residual.is_contiguous())
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=a.dtype)
    if y is None:
        y = torch.empty((M, N), device=a.device, dtype=a.dtype)
    ws, ws_bytes = _ws_arg(a.device, M, N, a.dtype == torch.bfloat16, ws)
    kind = L.NORM_RMS if norm_b is None else L.NORM_LAYER
    L.check(L.load().srgpt_gemm_norm(_p(a), _p(w), _p(bias), _p(residual), _p(out), M, N, K, ws, ws_bytes,
                                     kind, _p(norm_w), _p(norm_b), _p(y), float(eps), dt_code(a), _stream()))
    return out, y


def gemv(x, w, norm_w=None, eps=0.0, residual=None, swiglu=False, out=None, out_f32=False):
    """decode GEMV: x [B,K], w [N(,2N if swiglu),K] -> [B,N]."""
    _dev(x, w, norm_w, residual)
    _same_dtype("gemv", x, weight=w, norm_weight=norm_w, residual=residual)
    B, K = x.shape
    N = w.shape[0] // 2 if swiglu else w.shape[0]
    if out is None:
        out = torch.empty((B, N), device=x.device, dtype=torch.float32 if out_f32 else x.dtype)
    L.check(L.load().srgpt_gemv(_p(_c(x)), _p(w), _p(norm_w), float(eps), _p(residual), _p(out), B, N, K, int(swiglu),
                                int(out_f32), dt_code(x), _stream()))
    return out


def quantize_fp8_rows(w: torch.Tensor):
    """Weight-only fp8 quantisation used by the decode path.  Per output row: scale = the smallest power of two with
    max|row| / scale <= 448 (exact on every device: frexp / ldexp, no division), codes = OCP e4m3fn bytes of row / scale
    (round to nearest even).  A power-of-two scale costs a floating-point format nothing in relative precision.
    Returns (codes uint8 [N, K], scale fp32 [N], dequantised weights in w.dtype)."""
    wf = w.float()
    m, e = torch.frexp(wf.abs().amax(dim=1).clamp_min(2.0 ** -100))  # amax = m * 2^e, m in [0.5, 1)
    k = e - 9 + (m > 0.875).to(e.dtype)                              # 448 = 0.875 * 2^9
    scale = torch.ldexp(torch.ones_like(m), k)
    q = (wf * torch.ldexp(torch.ones_like(m), -k)[:, None]).to(torch.float8_e4m3fn)
    deq = (q.float() * scale[:, None]).to(w.dtype)
    return q.view(torch.uint8).contiguous(), scale.contiguous(), deq.contiguous()


def gemv_w8(x, w8, wscale, norm_w=None, eps=0.0, residual=None, swiglu=False, out=None, out_f32=False):
    """decode product with fp8 weights: x [B,K] bf16, w8 uint8 [N(,2N if swiglu),K], wscale fp32 [rows] -> [B,N]."""
    _dev(x, w8, wscale, norm_w, residual)
    _same_dtype("gemv_w8", x, norm_weight=norm_w, residual=residual)
    if x.dtype != torch.bfloat16 or w8.dtype != torch.uint8 or wscale.dtype != torch.float32:
        raise ValueError("gemv_w8: x must be bf16, w8 uint8, wscale fp32")
    B, K = x.shape
    N = w8.shape[0] // 2 if swiglu else w8.shape[0]
    if out is None:
        out = torch.empty((B, N), device=x.device, dtype=torch.float32 if out_f32 else x.dtype)
    L.check(L.load().srgpt_gemv_w8(_p(_c(x)), _p(w8), _p(wscale), _p(norm_w), float(eps), _p(residual), _p(out), B, N, K,
                                   int(swiglu), int(out_f32), _stream()))
    return out


_E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # magnitudes of the OCP e2m1 codes 0 .. 7 (bit 3 of a code: the sign)


def quantize_mxfp4_rows(w: torch.Tensor):
    """Weight-only MXFP4 quantisation (OCP Microscaling FP4; include/srgpt.h, srgpt_gemv_w4): w [N, K], K % 32 == 0.  Per block of
    32 consecutive values of a row: scale = the smallest power of two with max|block| / scale <= 6 (quantize_fp8_rows' rule: frexp /
    ldexp, exact on every device, nothing saturates), its exponent clamped to [-64, 64]; codes = round to nearest even of
    block / scale onto the e2m1 grid {0, .5, 1, 1.5, 2, 3, 4, 6} with a sign bit.  An all-zero block gets scale 1 and zero codes.
    Returns (codes uint8 [N, K / 2]: element k in byte k / 2, low nibble = even k; scales uint8 [N, K / 32]: E8M0 bytes, value
    2^(byte - 127), never 0 or 255; the dequantised weights code * scale in w.dtype -- exact in bf16).
    Like fp8 the format is opt-in and changes the numbers; its accuracy cost on a trained checkpoint is unmeasured."""
    if w.dim() != 2 or w.shape[1] % 32:
        raise ValueError(f"quantize_mxfp4_rows: a matrix [N, K] with K % 32 == 0, got {tuple(w.shape)}")
    N, K = w.shape
    wf = w.float().reshape(N, K // 32, 32)
    amax = wf.abs().amax(dim=2)
    m, e = torch.frexp(amax.clamp_min(2.0 ** -100))                 # amax = m * 2^e, m in [0.5, 1)
    k = (e - 3 + (m > 0.75).to(e.dtype)).clamp(-64, 64)              # 6 = 0.75 * 2^3
    k = torch.where(amax == 0, torch.zeros_like(k), k)
    a = (wf * torch.ldexp(torch.ones_like(m), -k)[:, :, None]).abs().clamp_max(6.0)  # (only a clamped exponent can exceed 6)
    # round to nearest even on the grid: steps of 0.5 below 2, of 1 below 4, of 2 above -- torch.round is half-to-even, and the even
    # multiples of each step are the codes with a zero mantissa bit
    r = torch.where(a < 2, torch.round(a * 2) / 2, torch.where(a < 4, torch.round(a), torch.round(a / 2) * 2))
    grid = torch.tensor(_E2M1_GRID, device=w.device, dtype=torch.float32)
    mag = torch.bucketize(r, grid)                                    # r is on the grid: its index
    neg = (wf < 0) & (mag > 0)                                        # (no negative zero: a zero has code 0)
    code = (mag | neg.to(mag.dtype) << 3).to(torch.uint8).reshape(N, K)
    codes = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    scales = (k + 127).to(torch.uint8).contiguous()
    deq = (torch.where(neg, -r, r) * torch.ldexp(torch.ones_like(m), k)[:, :, None]).reshape(N, K).to(w.dtype)
    return codes, scales, deq.contiguous()


def _check_mxfp4(op: str, w4: torch.Tensor, wscale8: torch.Tensor):
    if w4.dtype != torch.uint8 or wscale8.dtype != torch.uint8 or w4.dim() != 2 or wscale8.dim() != 2:
        raise ValueError(f"{op}: codes and scales must be uint8 matrices")
    if not (w4.is_contiguous() and wscale8.is_contiguous()) or w4.shape[0] != wscale8.shape[0] or w4.shape[1] != 16 * wscale8.shape[1]:
        raise ValueError(f"{op}: codes [N, K / 2] and scales [N, K / 32] must be contiguous and agree, got {tuple(w4.shape)} and "
                         f"{tuple(wscale8.shape)}")


def gemv_w4(x, w4, wscale8, norm_w=None, eps=0.0, residual=None, swiglu=False, out=None, out_f32=False):
    """decode product with MXFP4 weights: x [B,K] bf16, w4 uint8 [N(,2N if swiglu),K/2] codes, wscale8 uint8 [rows,K/32] -> [B,N]."""
    _dev(x, w4, wscale8, norm_w, residual)
    _same_dtype("gemv_w4", x, norm_weight=norm_w, residual=residual)
    if x.dtype != torch.bfloat16:
        raise ValueError("gemv_w4: x must be bf16")
    _check_mxfp4("gemv_w4", w4, wscale8)
    B, K = x.shape
    if w4.shape[1] * 2 != K:
        raise ValueError(f"gemv_w4: x has K = {K}, the codes {w4.shape[1] * 2}")
    N = w4.shape[0] // 2 if swiglu else w4.shape[0]
    if out is None:
        out = torch.empty((B, N), device=x.device, dtype=torch.float32 if out_f32 else x.dtype)
    L.check(L.load().srgpt_gemv_w4(_p(_c(x)), _p(w4), _p(wscale8), _p(norm_w), float(eps), _p(residual), _p(out), B, N, K,
                                   int(swiglu), int(out_f32), _stream()))
    return out


def dequant_mxfp4(w4, wscale8, out=None):
    """the exact bf16 matrix [N, K] of MXFP4 codes [N, K / 2] and E8M0 block scales [N, K / 32] (srgpt_dequant_mxfp4)."""
    _dev(w4, wscale8)
    _check_mxfp4("dequant_mxfp4", w4, wscale8)
    N, K = w4.shape[0], w4.shape[1] * 2
    if out is None:
        out = torch.empty((N, K), device=w4.device, dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape == (N, K)
    L.check(L.load().srgpt_dequant_mxfp4(_p(w4), _p(wscale8), _p(out), N, K, _stream()))
    return out


def kv_beam_reorder(kcache, vcache, beam_idx, num_beams: int, live: int) -> bool:
    """srgpt_kv_beam_reorder: in-place permutation of the live cache rows by the beam indices (kcache / vcache [layers, batch *
    num_beams, kv_heads, max_pos, head_dim], beam_idx int64 [batch * num_beams] on the device).  False: this beam count is not
    served by the kernel (the caller permutes with torch ops)."""
    if not 2 <= num_beams <= 8:
        return False
    _dev(kcache, vcache, beam_idx)
    Ly, R, Hkv, P, D = kcache.shape
    L.check(L.load().srgpt_kv_beam_reorder(_p(kcache), _p(vcache), _p(beam_idx.to(torch.int64).contiguous()), Ly, R // num_beams,
                                           int(num_beams), Hkv, P, D, int(live), dt_code(kcache), _stream()))
    return True


def gemv_rowss_supported(batch: int, fp8: bool = False) -> bool:
    """does a (batch, bf16 activations, bf16 / fp8 weights) decode product take the kernel with the row-statistics hand-off?"""
    return bool(L.load().srgpt_gemv_rowss_supported(int(batch), L.BF16, int(fp8)))


def pack_decode_weights(w, rows: int):
    """srgpt_pack_decode_weights: the packed decode layout (granules of `rows` = 4 / 8 / 16 weight rows in MFMA-operand order,
    include/srgpt.h ABI 9) of a row-major matrix [N, K] (uint8 = fp8 bytes, or bf16).  Returns a flat uint8 tensor; a SwiGLU matrix
    [gate; up] is packed as the one matrix of 2 N rows it is."""
    _dev(w)
    if w.dim() != 2 or not w.is_contiguous() or w.dtype not in (torch.uint8, torch.bfloat16):
        raise ValueError("pack_decode_weights: a contiguous uint8 (fp8) or bf16 matrix")
    N, K = w.shape
    eb = w.element_size()
    lib = L.load()
    out = torch.empty((int(lib.srgpt_packed_bytes(N, K, eb, int(rows))),), device=w.device, dtype=torch.uint8)
    L.check(lib.srgpt_pack_decode_weights(_p(w), _p(out), N, K, eb, int(rows), _stream()))
    return out


def pack13_eligible(w) -> bool:
    """can this matrix be held as lossless 13-bit codes (include/srgpt.h, srgpt_pack13)?  bf16 [N, K] with K % 512 == 0."""
    return w is not None and w.dim() == 2 and w.dtype == torch.bfloat16 and w.is_contiguous() and w.shape[1] % 512 == 0


def pack13(w):
    """srgpt_pack13: the lossless 13-bit code of a contiguous bf16 matrix [N, K], K % 512 == 0 (a SwiGLU matrix [gate; up] as the one
    matrix of 2 N rows it is).  Returns (packed uint8, flags int32 [N + 1], number of exception rows); synchronises the stream."""
    _dev(w)
    if not pack13_eligible(w):
        raise ValueError("pack13: a contiguous bf16 matrix [N, K] with K % 512 == 0")
    N, K = w.shape
    lib = L.load()
    fb = C.c_size_t(0)
    nbytes = int(lib.srgpt_pack13_bytes(N, K, C.byref(fb)))
    packed = torch.empty((nbytes,), device=w.device, dtype=torch.uint8)
    flags = torch.empty((fb.value // 4,), device=w.device, dtype=torch.int32)
    n_exc = lib.srgpt_pack13(_p(w), N, K, _p(packed), _p(flags), _stream())
    if n_exc < 0:
        L.check(n_exc)
    return packed, flags, int(n_exc)


def unpack13(packed, flags, w_raw, out=None):
    """srgpt_unpack13: the exact bf16 matrix of a packed copy (exception rows are copied from w_raw, the matrix it was packed from)."""
    _dev(packed, flags, w_raw)
    N, K = w_raw.shape
    if out is None:
        out = torch.empty((N, K), device=w_raw.device, dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape == (N, K)
    L.check(L.load().srgpt_unpack13(_p(packed), _p(flags), _p(w_raw), N, K, _p(out), _stream()))
    return out


def gemv_p13(x, packed, flags, w_raw, norm_w=None, eps=0.0, residual=None, swiglu=False, out=None, out_f32=False):
    """srgpt_gemv_p13: gemv() for ONE bf16 row over the 13-bit packed copy (pack13) of w_raw, bit for bit gemv(x, w_raw, ...)."""
    _dev(x, packed, flags, w_raw, norm_w, residual)
    _same_dtype("gemv_p13", x, weight=w_raw, norm_weight=norm_w, residual=residual)
    B, K = x.shape
    if B != 1 or x.dtype != torch.bfloat16 or w_raw.shape[1] != K or not w_raw.is_contiguous():
        raise ValueError("gemv_p13: one bf16 row of x [1, K] and the contiguous raw matrix [rows, K]")
    N = w_raw.shape[0] // 2 if swiglu else w_raw.shape[0]
    if out is None:
        out = torch.empty((B, N), device=x.device, dtype=torch.float32 if out_f32 else x.dtype)
    L.check(L.load().srgpt_gemv_p13(_p(_c(x)), _p(packed), _p(flags), _p(w_raw), _p(norm_w), float(eps), _p(residual), _p(out), N, K,
                                    int(swiglu), int(out_f32), _stream()))
    return out


def pack13_bind(w_raw, packed, flags) -> None:
    """srgpt_pack13_bind: from now on the batch-1 decode step of a bf16 engine streams `packed` where its weights point at w_raw."""
    L.check(L.load().srgpt_pack13_bind(_p(w_raw), _p(packed), _p(flags), int(w_raw.shape[0]), int(w_raw.shape[1])))


def pack13_unbind(w_raw) -> bool:
    return bool(L.load().srgpt_pack13_unbind(_p(w_raw)))


def pack13_bound(w_raw) -> bool:
    return bool(L.load().srgpt_pack13_bound(_p(w_raw)))


def gemv_wide_pass_rows(batch: int, n: int, k: int, fp8: bool = False, packed_rows: int = 0, w4: bool = False, norm: bool = False,
                        swiglu: bool = False) -> int:
    """srgpt_gemv_wide_pass_rows: rows per weight pass the `wide=True` products take for such a call -- 32, or 16 for a product
    (or a call of 16 rows or fewer) that keeps passes of 16."""
    return int(L.load().srgpt_gemv_wide_pass_rows(int(batch), int(fp8), int(packed_rows), int(w4), int(n), int(k), int(norm), int(swiglu)))


def gemv_rowss(x, w=None, w8=None, wscale=None, norm_w=None, eps=0.0, residual=None, swiglu=False, out=None, out_f32=False,
               rowss_in=None, publish=False, packed_rows=0, n_rows=None, table=None, wide=False):
    """srgpt_gemv_rowss: the decode product of 2+ bf16 rows as the batched decode step runs it.  `rowss_in`: the statistics
    table of x's rows ([B, 512] fp32, from the call that produced x) replaces the RMSNorm's own reduction; `publish`: also
    return the table of the output rows.  `packed_rows` > 0: w / w8 is the flat packed array of pack_decode_weights (n_rows = the
    matrix' row count, 2 N for SwiGLU).  `table`: with `publish`, the caller's contiguous fp32 [B, 512] tensor to publish into (None: a
    new one).  `wide`: srgpt_gemv_rowss_wide -- chunks of 17 - 32 rows in one weight pass (every row the bits of a 16-row pass holding it).
    Returns out, or (out, table)."""
    wt = w8 if w8 is not None else w
    _dev(x, wt, wscale, norm_w, residual, rowss_in)
    _same_dtype("gemv_rowss", x, norm_weight=norm_w, residual=residual)
    if x.dtype != torch.bfloat16:
        raise ValueError("gemv_rowss: bf16 activations only")
    B, K = x.shape
    if packed_rows:
        if n_rows is None:
            raise ValueError("gemv_rowss: a packed matrix needs n_rows")
        rows_total = int(n_rows)
    else:
        rows_total = wt.shape[0]
    N = rows_total // 2 if swiglu else rows_total
    if out is None:
        out = torch.empty((B, N), device=x.device, dtype=torch.float32 if out_f32 else x.dtype)
    if table is not None:
        _dev(table)
        if not publish or table.dtype != torch.float32 or tuple(table.shape) != (B, L.ROWSS_STRIDE) or not table.is_contiguous():
            raise ValueError("gemv_rowss: table must be a contiguous fp32 [batch, 512] tensor, with publish=True")
    elif publish:
        table = torch.empty((B, L.ROWSS_STRIDE), device=x.device, dtype=torch.float32)
    if rowss_in is not None and (rowss_in.dtype != torch.float32 or tuple(rowss_in.shape) != (B, L.ROWSS_STRIDE)
                                 or not rowss_in.is_contiguous()):
        raise ValueError("gemv_rowss: rowss_in must be a contiguous fp32 [batch, 512] table")
    fn = L.load().srgpt_gemv_rowss_wide if wide else L.load().srgpt_gemv_rowss
    L.check(fn(_p(_c(x)), _p(w) if w8 is None else None, _p(w8), _p(wscale), _p(norm_w), float(eps),
               _p(residual), _p(out), B, N, K, int(swiglu), int(out_f32), _p(rowss_in), _p(table), int(packed_rows), _stream()))
    return (out, table) if publish else out


MXFP4_GRANULE = 16  # SRGPT_MXFP4_GRANULE: weight rows per granule of the packed MXFP4 layout


def mxfp4_packed_bytes(n: int, k: int, swiglu: bool = False) -> int:
    """srgpt_mxfp4_packed_bytes: bytes of the packed copy of an MXFP4 matrix of n rows (a SwiGLU matrix: n gate + n up rows);
    0 outside the layout's domain (K % 128 == 0; swiglu: n % 16 == 0)."""
    return int(L.load().srgpt_mxfp4_packed_bytes(int(n), int(k), int(swiglu)))


def _mxfp4_shape(op: str, w4, wscale8, swiglu: bool):
    _check_mxfp4(op, w4, wscale8)
    rows, K = w4.shape[0], w4.shape[1] * 2
    if swiglu and rows % 2:
        raise ValueError(f"{op}: a SwiGLU matrix has gate rows followed by as many up rows, got {rows} rows")
    return (rows // 2 if swiglu else rows), K


def pack_mxfp4(w4, wscale8, swiglu: bool = False):
    """srgpt_pack_mxfp4: the packed decode layout (codes in MFMA-operand order with their E8M0 bytes beside them, granules of 16
    rows; include/srgpt.h) of codes [rows, K / 2] and scales [rows, K / 32], K % 128 == 0.  Returns a flat uint8 tensor."""
    _dev(w4, wscale8)
    N, K = _mxfp4_shape("pack_mxfp4", w4, wscale8, swiglu)
    nbytes = mxfp4_packed_bytes(N, K, swiglu)
    if nbytes == 0:
        raise ValueError(f"pack_mxfp4: K = {K} must be a multiple of 128, and a SwiGLU half ({N} rows) whole granules of {MXFP4_GRANULE}")
    packed = torch.empty((nbytes,), device=w4.device, dtype=torch.uint8)
    L.check(L.load().srgpt_pack_mxfp4(_p(w4), _p(wscale8), _p(packed), N, K, int(swiglu), _stream()))
    return packed


def unpack_mxfp4(packed, n: int, k: int, swiglu: bool = False, out=None):
    """srgpt_unpack_mxfp4: (codes, scales) of a packed copy, exactly what pack_mxfp4 was given.  out: (codes, scales) to write into."""
    _dev(packed)
    rows = 2 * int(n) if swiglu else int(n)
    if out is None:
        out = (torch.empty((rows, k // 2), device=packed.device, dtype=torch.uint8),
               torch.empty((rows, k // 32), device=packed.device, dtype=torch.uint8))
    w4, wscale8 = out
    _check_mxfp4("unpack_mxfp4", w4, wscale8)
    if tuple(w4.shape) != (rows, k // 2) or packed.numel() < mxfp4_packed_bytes(n, k, swiglu):
        raise ValueError("unpack_mxfp4: the outputs or the packed array do not have the shape's size")
    L.check(L.load().srgpt_unpack_mxfp4(_p(packed), _p(w4), _p(wscale8), int(n), int(k), int(swiglu), _stream()))
    return w4, wscale8


def gemv_w4p(x, packed, n_rows: int, norm_w=None, eps=0.0, residual=None, swiglu=False, out=None, out_f32=False, rowss_in=None,
             publish=False, table=None, wide=False):
    """srgpt_gemv_w4p: gemv_rowss's product over the packed copy (pack_mxfp4) of an MXFP4 matrix of `n_rows` rows (2 N for SwiGLU),
    any batch >= 1, on the MFMA kernel; bit for bit gemv_rowss(x, w=dequant_mxfp4(codes, scales), ...).  rowss_in / publish / table
    as for gemv_rowss; `wide`: srgpt_gemv_w4p_wide.  Returns out, or (out, table)."""
    _dev(x, packed, norm_w, residual, rowss_in)
    _same_dtype("gemv_w4p", x, norm_weight=norm_w, residual=residual)
    if x.dtype != torch.bfloat16 or packed.dtype != torch.uint8 or not packed.is_contiguous():
        raise ValueError("gemv_w4p: bf16 activations and a contiguous uint8 packed array")
    B, K = x.shape
    N = int(n_rows) // 2 if swiglu else int(n_rows)
    need = mxfp4_packed_bytes(N, K, swiglu)
    if need and packed.numel() < need:
        raise ValueError(f"gemv_w4p: the packed array holds {packed.numel()} bytes, the shape needs {need}")
    if out is None:
        out = torch.empty((B, N), device=x.device, dtype=torch.float32 if out_f32 else x.dtype)
    if table is not None:
        _dev(table)
        if not publish or table.dtype != torch.float32 or tuple(table.shape) != (B, L.ROWSS_STRIDE) or not table.is_contiguous():
            raise ValueError("gemv_w4p: table must be a contiguous fp32 [batch, 512] tensor, with publish=True")
    elif publish:
        table = torch.empty((B, L.ROWSS_STRIDE), device=x.device, dtype=torch.float32)
    if rowss_in is not None and (rowss_in.dtype != torch.float32 or tuple(rowss_in.shape) != (B, L.ROWSS_STRIDE)
                                 or not rowss_in.is_contiguous()):
        raise ValueError("gemv_w4p: rowss_in must be a contiguous fp32 [batch, 512] table")
    fn = L.load().srgpt_gemv_w4p_wide if wide else L.load().srgpt_gemv_w4p
    L.check(fn(_p(_c(x)), _p(packed), _p(norm_w), float(eps), _p(residual), _p(out), B, N, K, int(swiglu), int(out_f32), _p(rowss_in),
               _p(table), _stream()))
    return (out, table) if publish else out


def mxfp4_bind(w4, packed, swiglu: bool = False) -> None:
    """srgpt_mxfp4_bind: from now on a decode-shaped step of 2+ rows of an MXFP4 engine multiplies `packed` where its weights point
    at the code array w4 [rows, K / 2] -- once every layer matrix of the engine is bound."""
    rows, K = int(w4.shape[0]), int(w4.shape[1]) * 2
    L.check(L.load().srgpt_mxfp4_bind(_p(w4), _p(packed), rows // 2 if swiglu else rows, K, int(swiglu)))


def mxfp4_unbind(w4) -> bool:
    return bool(L.load().srgpt_mxfp4_unbind(_p(w4)))


def mxfp4_bound(w4) -> bool:
    return bool(L.load().srgpt_mxfp4_bound(_p(w4)))


def gemm_w8(a, w8, wscale, bias=None, residual=None, act=L.ACT_NONE, out=None, out_f32=False, ws=None):
    """act((a @ fp8(w8).T) * wscale + bias) + residual: a [M,K] bf16 (row stride may exceed K), w8 uint8 [N,K] (OCP e4m3fn),
    wscale fp32 [N].  ws: as for gemm."""
    _dev(a, w8, wscale, bias, residual)
    _same_dtype("gemm_w8", a, bias=bias, residual=residual)
    if a.dtype != torch.bfloat16 or w8.dtype != torch.uint8 or wscale.dtype != torch.float32:
        raise ValueError("gemm_w8: a must be bf16, w8 uint8, wscale fp32")
    M, K = a.shape
    N = w8.shape[0]
    assert w8.shape[1] == K and a.stride(1) == 1 and w8.is_contiguous() and wscale.numel() == N
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.float32 if out_f32 else a.dtype)
    ws, ws_bytes = _ws_arg(a.device, M, N, ws=ws)
    L.check(L.load().srgpt_gemm_w8(_p(a), _p(w8), _p(wscale), _p(bias), _p(residual), _p(out), M, N, K, a.stride(0), out.stride(0),
                                   act, int(out_f32), ws, ws_bytes, _stream()))
    return out


def quant_rows_e4m3(x):
    """per-row (per-token) fp8 quantisation of activations: x [M,K] bf16 (row stride may exceed K) -> (codes uint8 [M,K],
    scale fp32 [M]); the power-of-two rule of quantize_fp8_rows, on the device (srgpt_quant_rows_e4m3)."""
    _dev(x)
    if x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("quant_rows_e4m3: x must be a bf16 matrix with contiguous rows")
    M, K = x.shape
    q = torch.empty((M, K), device=x.device, dtype=torch.uint8)
    sc = torch.empty((M,), device=x.device, dtype=torch.float32)
    L.check(L.load().srgpt_quant_rows_e4m3(_p(x), _p(q), _p(sc), M, K, x.stride(0), _stream()))
    return q, sc


def quant_rows_e4m3_rmsnorm(x, norm_w, eps):
    """quant_rows_e4m3(rmsnorm(x, norm_w, eps)) in one launch (bit-identical to the two; the W8A8 prefill's form)."""
    _dev(x, norm_w)
    if x.dtype != torch.bfloat16 or norm_w.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("quant_rows_e4m3_rmsnorm: x must be a bf16 matrix with contiguous rows, norm_w bf16")
    M, K = x.shape
    q = torch.empty((M, K), device=x.device, dtype=torch.uint8)
    sc = torch.empty((M,), device=x.device, dtype=torch.float32)
    L.check(L.load().srgpt_quant_rows_e4m3_rmsnorm(_p(x), _p(norm_w), float(eps), _p(q), _p(sc), M, K, x.stride(0), _stream()))
    return q, sc


def quant_rows_e4m3_swiglu(gate_up):
    """quant_rows_e4m3(silu_mul(gate_up)) in one launch: gate_up [M, 2 * inter] = [gate | up], contiguous."""
    _dev(gate_up)
    if gate_up.dtype != torch.bfloat16 or gate_up.dim() != 2 or not gate_up.is_contiguous() or gate_up.shape[1] % 2:
        raise ValueError("quant_rows_e4m3_swiglu: gate_up must be a contiguous bf16 [M, 2 * inter] matrix")
    M, inter = gate_up.shape[0], gate_up.shape[1] // 2
    q = torch.empty((M, inter), device=gate_up.device, dtype=torch.uint8)
    sc = torch.empty((M,), device=gate_up.device, dtype=torch.float32)
    L.check(L.load().srgpt_quant_rows_e4m3_swiglu(_p(gate_up), _p(q), _p(sc), M, inter, _stream()))
    return q, sc


def gemm_w8a8(a8, ascale, w8, wscale, bias=None, residual=None, out=None, out_f32=False, ws=None):
    """((fp8(a8) @ fp8(w8).T) * ascale[:,None] * wscale[None,:] + bias) + residual on the fp8 matrix pipe: a8 uint8 [M,K],
    w8 uint8 [N,K] (OCP e4m3fn), ascale fp32 [M], wscale fp32 [N]; bias / residual / out bf16 (out fp32 if out_f32).  ws: as
    for gemm."""
    _dev(a8, ascale, w8, wscale, bias, residual)
    if a8.dtype != torch.uint8 or w8.dtype != torch.uint8 or ascale.dtype != torch.float32 or wscale.dtype != torch.float32:
        raise ValueError("gemm_w8a8: a8 / w8 must be uint8, ascale / wscale fp32")
    for name, t in (("bias", bias), ("residual", residual)):
        if t is not None and t.dtype != torch.bfloat16:
            raise ValueError(f"gemm_w8a8: {name} must be bf16")
    M, K = a8.shape
    N = w8.shape[0]
    assert w8.shape[1] == K and a8.stride(1) == 1 and w8.is_contiguous() and ascale.numel() == M and wscale.numel() == N
    if out is None:
        out = torch.empty((M, N), device=a8.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    ws, ws_bytes = _ws_arg(a8.device, M, N, ws=ws)
    L.check(L.load().srgpt_gemm_w8a8(_p(a8), _p(ascale), _p(w8), _p(wscale), _p(bias), _p(residual), _p(out), M, N, K,
                                     a8.stride(0), out.stride(0), int(out_f32), ws, ws_bytes,
                                     _stream()))
    return out


def gemm_w4a8(a8, ascale, w4, wscale8, bias=None, residual=None, out=None, out_f32=False, ws=None):
    """gemm_w8a8 with MXFP4 weights (W4A8): ((fp8(a8) @ dequant(w4, wscale8).T) * ascale[:,None] + bias) + residual on the
    block-scaled fp8 x fp4 MFMA -- a8 uint8 [M,K] + ascale fp32 [M] as for gemm_w8a8, w4 uint8 [N,K/2] codes and wscale8 uint8
    [N,K/32] E8M0 bytes as quantize_mxfp4_rows stores them; nothing is expanded.  bias / residual / out / ws: as for gemm_w8a8."""
    _dev(a8, ascale, w4, wscale8, bias, residual)
    if a8.dtype != torch.uint8 or ascale.dtype != torch.float32:
        raise ValueError("gemm_w4a8: a8 must be uint8, ascale fp32")
    _check_mxfp4("gemm_w4a8", w4, wscale8)
    for name, t in (("bias", bias), ("residual", residual)):
        if t is not None and t.dtype != torch.bfloat16:
            raise ValueError(f"gemm_w4a8: {name} must be bf16")
    M, K = a8.shape
    N = w4.shape[0]
    if w4.shape[1] * 2 != K:
        raise ValueError(f"gemm_w4a8: a8 has K = {K}, the codes {w4.shape[1] * 2}")
    assert a8.stride(1) == 1 and ascale.numel() == M
    if out is None:
        out = torch.empty((M, N), device=a8.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    ws, ws_bytes = _ws_arg(a8.device, M, N, ws=ws)
    L.check(L.load().srgpt_gemm_w4a8(_p(a8), _p(ascale), _p(w4), _p(wscale8), _p(bias), _p(residual), _p(out), M, N, K,
                                     a8.stride(0), out.stride(0), int(out_f32), ws, ws_bytes, _stream()))
    return out


def layernorm(x, w, b, eps, act=L.ACT_NONE, out=None):
    _dev(x, w, b)
    _same_dtype("layernorm", x, weight=w, bias=b, out=out)
    x = _c(x)
    cols = x.shape[-1]
    rows = x.numel() // cols
    if out is None:
        out = torch.empty_like(x)
    L.check(L.load().srgpt_layernorm(_p(x), _p(w), _p(b), _p(out), rows, cols, float(eps), act, dt_code(x), _stream()))
    return out


def rmsnorm(x, w, eps, out=None):
    _dev(x, w)
    _same_dtype("rmsnorm", x, weight=w, out=out)
    x = _c(x)
    cols = x.shape[-1]
    rows = x.numel() // cols
    if out is None:
        out = torch.empty_like(x)
    L.check(L.load().srgpt_rmsnorm(_p(x), _p(w), _p(out), rows, cols, float(eps), dt_code(x), _stream()))
    return out


def attention(q, k, v, causal=False, scale=None, kv_len=None):
    """q [B,Tq,Hq,D], k/v [B,Tk,Hkv,D] (arbitrary strides with unit last stride) -> [B,Tq,Hq,D]."""
    _dev(q, k, v)
    _same_dtype("attention", q, k=k, v=v)
    B, Tq, Hq, D = q.shape
    Tk, Hkv = k.shape[1], k.shape[2]
    assert q.stride(3) == 1 and k.stride(3) == 1 and v.stride(3) == 1
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    o = torch.empty((B, Tq, Hq, D), device=q.device, dtype=q.dtype)
    L.check(L.load().srgpt_attention(_p(q), _p(k), _p(v), _p(o), B, Tq, Tk, Hq, Hkv, D, q.stride(0), q.stride(1),
                                     q.stride(2), k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1),
                                     v.stride(2), float(scale), int(causal), _p(kv_len), dt_code(q), _stream()))
    return o


def attention_append(q, k, v, q_pos0, kv_len=None, Tk=None, scale=None):
    """srgpt_attention_append: q [B,Tq,Hq,D] new query rows, row b at positions q_pos0[b] + t (int32 [B], device); k/v [B,>=Tk,Hkv,D]
    the live cache (arbitrary strides with unit last stride); Tk = the host's bound on the keys any row may see (default: all of k);
    kv_len (int32 [B], optional) the keys row b may see -> [B,Tq,Hq,D]."""
    _dev(q, k, v, q_pos0)
    _same_dtype("attention_append", q, k=k, v=v)
    B, Tq, Hq, D = q.shape
    Hkv = k.shape[2]
    Tk = k.shape[1] if Tk is None else int(Tk)
    assert q.stride(3) == 1 and k.stride(3) == 1 and v.stride(3) == 1 and Tk <= k.shape[1] and Tk <= v.shape[1]
    assert q_pos0.dtype == torch.int32 and q_pos0.shape == (B,) and q_pos0.is_contiguous()
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    o = torch.empty((B, Tq, Hq, D), device=q.device, dtype=q.dtype)
    L.check(L.load().srgpt_attention_append(_p(q), _p(k), _p(v), _p(o), B, Tq, Tk, Hq, Hkv, D, q.stride(0), q.stride(1),
                                            q.stride(2), k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1),
                                            v.stride(2), float(scale), _p(q_pos0), _p(kv_len), dt_code(q), _stream()))
    return o


def gemm_swiglu(a, wgu, out=None):
    """silu(a @ wg.T) * (a @ wu.T) for the stacked weight wgu = [wg; wu] ([2 I, K]): gemm + silu_mul in one call."""
    _dev(a, wgu)
    _same_dtype("gemm_swiglu", a, weight=wgu)
    M, K = a.shape
    I = wgu.shape[0] // 2
    assert wgu.shape == (2 * I, K) and a.is_contiguous() and wgu.is_contiguous()
    if out is None:
        out = torch.empty((M, I), device=a.device, dtype=a.dtype)
    scratch = torch.empty((M, 2 * I), device=a.device, dtype=a.dtype)
    ws, ws_bytes = _ws_arg(a.device, M, 2 * I, a.dtype == torch.bfloat16)
    L.check(L.load().srgpt_gemm_swiglu(_p(a), _p(wgu), _p(out), M, I, K, _p(scratch), ws, ws_bytes,
                                       dt_code(a), _stream()))
    return out


def gemm_rope_kv_append(a, w, kcache, vcache, cos_tab, sin_tab, B, T, Hq, Hkv, D, pos0=None, qkv=None):
    """qkv = a @ w.T for the B * T token rows, RoPE on q (in qkv) and k, k / v appended to the caches: gemm + rope_kv_append in one call."""
    _dev(a, w, kcache, vcache, cos_tab, sin_tab)
    M, K = a.shape
    N = (Hq + 2 * Hkv) * D
    assert M == B * T and w.shape == (N, K) and a.is_contiguous() and w.is_contiguous()
    if qkv is None:
        qkv = torch.empty((M, N), device=a.device, dtype=a.dtype)
    ws, ws_bytes = _ws_arg(a.device, M, N, a.dtype == torch.bfloat16)
    max_pos = kcache.shape[-2]
    L.check(L.load().srgpt_gemm_rope_kv_append(_p(a), _p(w), _p(qkv), K, ws, ws_bytes, _p(kcache),
                                               _p(vcache), _p(pos0), _p(cos_tab), _p(sin_tab), B, T, Hq, Hkv, D, max_pos,
                                               dt_code(a), _stream()))
    return qkv


def _w4_operand(op, a, w4, wscale8, rows=None):
    """checks of a W4A16 product's operands -> (M, N, K): a [M, K] bf16 (dense), codes [N, K / 2], scales [N, K / 32]."""
    _dev(a, w4, wscale8)
    if a.dtype != torch.bfloat16:
        raise ValueError(f"{op}: a must be bf16")
    _check_mxfp4(op, w4, wscale8)
    M, K = a.shape
    if w4.shape[1] * 2 != K:
        raise ValueError(f"{op}: a has K = {K}, the codes {w4.shape[1] * 2}")
    if rows is not None and w4.shape[0] != rows:
        raise ValueError(f"{op}: the codes have {w4.shape[0]} rows, the product needs {rows}")
    return M, w4.shape[0], K


def _w4_expand(op, expand, in_kernel, N, K, device):
    """the bf16 scratch [N, K] the codes are expanded into where no kernel multiplies them: the caller's, or a fresh one on the
    expansion path (None where the codes are multiplied in the kernel: it is neither written nor read there)."""
    if expand is not None:
        _dev(expand)
        if expand.dtype != torch.bfloat16 or not expand.is_contiguous() or expand.numel() < N * K:
            raise ValueError(f"{op}: expand must be a contiguous bf16 buffer of at least {N} x {K} elements")
        return expand
    return None if in_kernel else torch.empty((N, K), device=device, dtype=torch.bfloat16)


def gemm_w4_in_kernel(M, N, K, swiglu=False, device=None, ws=None, direct=False) -> bool:
    """srgpt_gemm_w4_in_kernel with the split-K workspace this module passes: True when gemm_w4 / gemm_w4_norm /
    gemm_w4_rope_kv_append of an [M, K] x [N, K] product (gemm_w4_swiglu with N = I) multiply the MXFP4 codes inside the GEMM kernel
    on this device, False when they expand the codes into the bf16 scratch first.  direct: the answer for the same calls with
    direct=True (srgpt_gemm_w4_direct_in_kernel)."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    ws, ws_bytes = _ws_arg(device, M, 2 * N if swiglu else N, True, ws)
    return _w4_in_kernel(M, N, K, swiglu, ws, ws_bytes, direct)


def _w4_in_kernel(M, N, K, swiglu, ws, ws_bytes, direct=False) -> bool:
    fn = L.load().srgpt_gemm_w4_direct_in_kernel if direct else L.load().srgpt_gemm_w4_in_kernel
    return bool(fn(M, N, K, int(swiglu), int(ws is not None), ws_bytes))


def _w4_entry(name, direct):
    """the C entry point `name`, or its `_direct` form (include/srgpt.h): the whole-M kernel multiplies the codes too"""
    return getattr(L.load(), name + "_direct" if direct else name)


def gemm_w4(a, w4, wscale8, residual=None, out=None, out_f32=False, expand=None, ws=None, direct=False):
    """a @ dequant(w4, wscale8).T + residual with MXFP4 weights (codes [N, K / 2], E8M0 scales [N, K / 32]): bit for bit
    gemm(a, dequant_mxfp4(w4, wscale8), residual=...).  a [M, K] bf16 (row stride may exceed K).  expand: the bf16 [N, K] scratch of
    the expansion path (see gemm_w4_in_kernel; None: allocated when needed).  ws: as for gemm.  direct (here and on the three
    products below): the `_direct` entry point -- the same bits, the codes multiplied in the whole-M kernel too (opt-in)."""
    M, N, K = _w4_operand("gemm_w4", a, w4, wscale8)
    _dev(residual)
    _same_dtype("gemm_w4", a, residual=residual)
    assert a.stride(1) == 1
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.float32 if out_f32 else a.dtype)
    ws, ws_bytes = _ws_arg(a.device, M, N, True, ws)
    expand = _w4_expand("gemm_w4", expand, _w4_in_kernel(M, N, K, False, ws, ws_bytes, direct), N, K, a.device)
    L.check(_w4_entry("srgpt_gemm_w4", direct)(_p(a), _p(w4), _p(wscale8), _p(residual), _p(out), M, N, K, a.stride(0), out.stride(0),
                                   int(out_f32), _p(expand), ws, ws_bytes, _stream()))
    return out


def gemm_w4_norm(a, w4, wscale8, residual, norm_w, eps, out=None, y=None, expand=None, ws=None, direct=False):
    """(a @ dequant(w4, wscale8).T + residual, rmsnorm(that)): gemm_norm (RMSNorm, no bias) with MXFP4 weights, bit for bit
    gemm_norm(a, dequant_mxfp4(w4, wscale8), ...).  expand / ws: as for gemm_w4."""
    M, N, K = _w4_operand("gemm_w4_norm", a, w4, wscale8)
    _dev(residual, norm_w)
    _same_dtype("gemm_w4_norm", a, residual=residual, norm_weight=norm_w)
    assert a.is_contiguous() and (residual is None or residual.is_contiguous())
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=a.dtype)
    if y is None:
        y = torch.empty((M, N), device=a.device, dtype=a.dtype)
    ws, ws_bytes = _ws_arg(a.device, M, N, True, ws)
    expand = _w4_expand("gemm_w4_norm", expand, _w4_in_kernel(M, N, K, False, ws, ws_bytes, direct), N, K, a.device)
    L.check(_w4_entry("srgpt_gemm_w4_norm", direct)(_p(a), _p(w4), _p(wscale8), _p(residual), _p(out), M, N, K, _p(expand), ws, ws_bytes,
                                        _p(norm_w), _p(y), float(eps), _stream()))
    return out, y


def gemm_w4_swiglu(a, wgu4, wscale8, out=None, expand=None, direct=False):
    """silu(a @ wg.T) * (a @ wu.T) for the stacked MXFP4 matrix [2 I, K]: bit for bit gemm_swiglu(a, dequant_mxfp4(wgu4, wscale8)).
    expand: the bf16 [2 I, K] scratch of the expansion path (None: allocated when needed)."""
    M, N2, K = _w4_operand("gemm_w4_swiglu", a, wgu4, wscale8)
    I = N2 // 2
    assert N2 == 2 * I and a.is_contiguous()
    if out is None:
        out = torch.empty((M, I), device=a.device, dtype=a.dtype)
    scratch = torch.empty((M, 2 * I), device=a.device, dtype=a.dtype)
    ws, ws_bytes = _ws_arg(a.device, M, 2 * I, True)
    expand = _w4_expand("gemm_w4_swiglu", expand, _w4_in_kernel(M, I, K, True, ws, ws_bytes, direct), 2 * I, K, a.device)
    L.check(_w4_entry("srgpt_gemm_w4_swiglu", direct)(_p(a), _p(wgu4), _p(wscale8), _p(out), M, I, K, _p(scratch), _p(expand), ws, ws_bytes,
                                          _stream()))
    return out


def gemm_w4_rope_kv_append(a, w4, wscale8, kcache, vcache, cos_tab, sin_tab, B, T, Hq, Hkv, D, pos0=None, qkv=None, expand=None,
                           direct=False):
    """gemm_rope_kv_append with MXFP4 weights: bit for bit (qkv and both caches) the bf16 call on dequant_mxfp4(w4, wscale8)."""
    N = (Hq + 2 * Hkv) * D
    M, _, K = _w4_operand("gemm_w4_rope_kv_append", a, w4, wscale8, rows=N)
    _dev(kcache, vcache, cos_tab, sin_tab)
    assert M == B * T and a.is_contiguous()
    if qkv is None:
        qkv = torch.empty((M, N), device=a.device, dtype=a.dtype)
    ws, ws_bytes = _ws_arg(a.device, M, N, True)
    expand = _w4_expand("gemm_w4_rope_kv_append", expand, _w4_in_kernel(M, N, K, False, ws, ws_bytes, direct), N, K, a.device)
    max_pos = kcache.shape[-2]
    L.check(_w4_entry("srgpt_gemm_w4_rope_kv_append", direct)(_p(a), _p(w4), _p(wscale8), _p(qkv), K, _p(expand), ws, ws_bytes, _p(kcache),
                                                  _p(vcache), _p(pos0), _p(cos_tab), _p(sin_tab), B, T, Hq, Hkv, D, max_pos,
                                                  _stream()))
    return qkv


def rope_kv_append(qkv, kcache, vcache, cos_tab, sin_tab, B, T, Hq, Hkv, D, pos0=None):
    _dev(qkv, kcache, vcache, cos_tab, sin_tab)
    max_pos = kcache.shape[-2]
    L.check(L.load().srgpt_rope_kv_append(_p(qkv), _p(kcache), _p(vcache), _p(pos0), _p(cos_tab), _p(sin_tab), B, T, Hq,
                                          Hkv, D, max_pos, dt_code(qkv), _stream()))


def decode_attention_ws(B, Hq, D, device):
    """Workspace of srgpt_decode_attention for B sequences, zeroed -> (ws, tickets): `tickets` is the int32 view of the arrival
    tickets behind the B * Hq * 64 * (D + 2) partial floats (include/srgpt.h), sharing ws's memory."""
    n = int(L.load().srgpt_decode_attn_ws_floats(B, Hq, D))
    ws = torch.zeros((n,), device=device, dtype=torch.float32)
    return ws, ws[B * Hq * 64 * (D + 2):].view(torch.int32)


def decode_attention(qkv, kcache, vcache, pos, cos_tab, sin_tab, Hq, Hkv, D, ws=None):
    """ws: a caller-owned workspace (decode_attention_ws) whose tickets are zero, reused from launch to launch; None = a fresh one."""
    _dev(qkv, kcache, vcache, pos)
    B = qkv.shape[0]
    max_pos = kcache.shape[-2]
    out = torch.empty((B, Hq * D), device=qkv.device, dtype=qkv.dtype)
    if ws is None:
        ws = decode_attention_ws(B, Hq, D, qkv.device)[0]  # tickets start at 0
    else:
        _dev(ws)
        assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= L.load().srgpt_decode_attn_ws_floats(B, Hq, D)
    L.check(L.load().srgpt_decode_attention(_p(qkv), _p(kcache), _p(vcache), _p(pos), _p(cos_tab), _p(sin_tab), _p(out),
                                            _p(ws), B, Hq, Hkv, D, max_pos, dt_code(qkv), _stream()))
    return out


def decode_attention_multi_ws(B, T, Hq, D, device):
    """Workspace of srgpt_decode_attention_multi, zeroed -> (ws, tickets): `tickets` is the int32 view of the arrival tickets behind the
    B * T * Hq * 64 * (D + 2) partial floats (include/srgpt.h), sharing ws's memory."""
    n = int(L.load().srgpt_decode_attn_multi_ws_floats(B, T, Hq, D))
    ws = torch.zeros((n,), device=device, dtype=torch.float32)
    return ws, ws[B * T * Hq * 64 * (D + 2):].view(torch.int32)


def decode_attention_multi(qkv, kcache, vcache, pos, cos_tab, sin_tab, Hq, Hkv, D, ws=None, out=None):
    """qkv [B, T, (Hq + 2 Hkv) D] raw projections of T new tokens per sequence -> out [B, T, Hq D]; the caches receive rows
    pos[b] .. pos[b] + T - 1.  Off the bf16 / head_dim-128 route the q heads of `qkv` are rotated in place (include/srgpt.h)."""
    _dev(qkv, kcache, vcache, pos)
    B, T = qkv.shape[0], qkv.shape[1]
    max_pos = kcache.shape[-2]
    if out is None:
        out = torch.empty((B, T, Hq * D), device=qkv.device, dtype=qkv.dtype)
    if ws is None:
        ws = decode_attention_multi_ws(B, T, Hq, D, qkv.device)[0]
    else:
        _dev(ws)
        assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= L.load().srgpt_decode_attn_multi_ws_floats(B, T, Hq, D)
    L.check(L.load().srgpt_decode_attention_multi(_p(qkv), _p(kcache), _p(vcache), _p(pos), _p(cos_tab), _p(sin_tab), _p(out), _p(ws),
                                                  B, T, Hq, Hkv, D, max_pos, dt_code(qkv), _stream()))
    return out


def lookup_draft(prompt_ids, out_ids, step, K: int, max_ngram: int, vocab: int):
    """srgpt_lookup_draft: prompt_ids int64 [n] (or None), out_ids int64 [max_new], step int32 [1], all on the device ->
    (draft int64 [K], n_draft int32 [1])"""
    _dev(out_ids, step)
    n_prompt = 0 if prompt_ids is None else int(prompt_ids.numel())
    draft = torch.empty((K,), dtype=torch.int64, device=out_ids.device)
    n_draft = torch.empty((1,), dtype=torch.int32, device=out_ids.device)
    L.check(L.load().srgpt_lookup_draft(_p(prompt_ids) if n_prompt else None, n_prompt, _p(out_ids), _p(step), int(out_ids.numel()), K,
                                        max_ngram, vocab, _p(draft), _p(n_draft), _stream()))
    return draft, n_draft


def lookup_accept(picks, draft, n_draft, tok, out_ids, pos, step, max_pos: int, tok_emb=None, stats=None):
    """srgpt_lookup_accept on the state's buffers (batch 1), in place"""
    _dev(picks, draft, n_draft, tok, out_ids, pos, step)
    L.check(L.load().srgpt_lookup_accept(_p(picks), _p(draft), _p(n_draft), int(picks.numel()), _p(tok), _p(out_ids), _p(pos), _p(step),
                                         int(out_ids.numel()), max_pos, _p(tok_emb), _p(stats), _stream()))


def lookup_draft_batch(prompt_ids, n_prompt, out_ids, steps, K: int, max_ngram: int, vocab: int, draft=None, n_draft=None):
    """srgpt_lookup_draft_batch: prompt_ids int64 [B, ld] (or None), n_prompt int32 [B], out_ids int64 [B, max_new], steps int32 [B],
    all on the device -> (draft int64 [B, K], n_draft int32 [B]); `draft` / `n_draft`: the caller's buffers instead of fresh ones"""
    _dev(n_prompt, out_ids, steps)
    B, max_new = out_ids.shape
    ld = 0 if prompt_ids is None else int(prompt_ids.shape[1])
    assert out_ids.is_contiguous() and (prompt_ids is None or (prompt_ids.is_contiguous() and prompt_ids.shape[0] == B))
    if draft is None:
        draft = torch.empty((B, K), dtype=torch.int64, device=out_ids.device)
    if n_draft is None:
        n_draft = torch.empty((B,), dtype=torch.int32, device=out_ids.device)
    assert draft.is_contiguous() and draft.shape == (B, K) and n_draft.shape == (B,)
    L.check(L.load().srgpt_lookup_draft_batch(_p(prompt_ids) if ld else None, ld, _p(n_prompt), _p(out_ids), _p(steps), B, max_new, K,
                                              max_ngram, vocab, _p(draft), _p(n_draft), _stream()))
    return draft, n_draft


def lookup_accept_batch(picks, draft, n_draft, tok, out_ids, pos, steps, step, max_pos: int, tok_emb=None, stats=None):
    """srgpt_lookup_accept_batch on the state's buffers, in place: picks int64 [B * T], draft [B, T - 1], out_ids [B, max_new]"""
    _dev(picks, draft, n_draft, tok, out_ids, pos, steps, step)
    B, max_new = out_ids.shape
    T = int(draft.shape[1]) + 1
    assert picks.numel() == B * T and out_ids.is_contiguous() and draft.is_contiguous()
    L.check(L.load().srgpt_lookup_accept_batch(_p(picks), _p(draft), _p(n_draft), B, T, _p(tok), _p(out_ids), _p(pos), _p(steps), _p(step),
                                               max_new, max_pos, _p(tok_emb), _p(stats), _stream()))


def region_pool(feat, masks, fw: Optional[int] = None):
    """MaskPooling for one image: feat [L,C], masks [M,mh,mw] (float32 or bfloat16) -> [M,C]."""
    _dev(feat, masks)
    Lf, Cc = feat.shape
    M, mh, mw = masks.shape
    sf = (Lf / (mh * mw)) ** 0.5  # base_extractor.py:53-54 (python float = double)
    oh, ow = int(math.floor(mh * sf)), int(math.floor(mw * sf))  # F.interpolate(scale_factor=...) output size
    if oh * ow != Lf or oh != ow:
        raise RuntimeError(f"mask of size {mh}x{mw} resamples to {oh}x{ow}, which does not match {Lf} feature tokens")
    if masks.dtype not in (torch.float32, torch.bfloat16):
        masks = masks.float()  # reference: mask.float()
    masks = _c(masks)
    rs = 1.0 / sf  # ATen passes static_cast<float>(1.0 / scale_factor)
    outs = []
    lib = L.load()
    for m0 in range(0, M, 16):
        mm = min(16, M - m0)
        out = torch.empty((mm, Cc), device=feat.device, dtype=feat.dtype)
        ws = torch.empty((lib.srgpt_region_pool_ws_floats(mm, oh, Cc),), device=feat.device, dtype=torch.float32)
        L.check(lib.srgpt_region_pool(_p(_c(feat)), _p(masks[m0:m0 + mm]), _p(out), _p(ws), mm, mh, mw, oh, Cc, rs, rs,
                                      _DT[masks.dtype], dt_code(feat), _stream()))
        outs.append(out)
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


def region_pool_u8(feat, masks_u8, size: int):
    """MaskPooling straight from raw uint8 masks [M, H, W]: the cv2-nearest resize to the processor size
    (`size` x `size`, image_aspect_ratio == "resize"), float(uint8) and the bilinear resample run inside the pooling kernel.
    Bit-identical to region_pool(feat, process_regions_device(masks, ...))."""
    from .mm_utils import cv2_nearest_index

    _dev(feat, masks_u8)
    if masks_u8.dtype != torch.uint8 or masks_u8.dim() != 3:
        raise ValueError("region_pool_u8: masks must be a uint8 tensor [M, H, W]")
    Lf, Cc = feat.shape
    M, rh, rw = masks_u8.shape
    mh = mw = int(size)
    sf = (Lf / (mh * mw)) ** 0.5
    oh, ow = int(math.floor(mh * sf)), int(math.floor(mw * sf))
    if oh * ow != Lf or oh != ow:
        raise RuntimeError(f"mask of size {mh}x{mw} resamples to {oh}x{ow}, which does not match {Lf} feature tokens")
    ys = torch.from_numpy(cv2_nearest_index(rh, mh)).to(feat.device)
    xs = torch.from_numpy(cv2_nearest_index(rw, mw)).to(feat.device)
    masks_u8 = _c(masks_u8)
    rs = 1.0 / sf
    lib = L.load()
    outs = []
    for m0 in range(0, M, 16):
        mm = min(16, M - m0)
        out = torch.empty((mm, Cc), device=feat.device, dtype=feat.dtype)
        ws = torch.empty((lib.srgpt_region_pool_ws_floats(mm, oh, Cc),), device=feat.device, dtype=torch.float32)
        L.check(lib.srgpt_region_pool_u8(_p(_c(feat)), _p(masks_u8[m0:m0 + mm]), _p(ys), _p(xs), _p(out), _p(ws), mm, rh, rw, mh, mw,
                                         oh, Cc, rs, rs, dt_code(feat), _stream()))
        outs.append(out)
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


def avgpool(x, n_img, in_w, out_w):
    _dev(x)
    Cc = x.shape[-1]
    y = torch.empty((n_img, out_w * out_w, Cc), device=x.device, dtype=x.dtype)
    L.check(L.load().srgpt_avgpool(_p(_c(x)), _p(y), n_img, in_w, out_w, Cc, dt_code(x), _stream()))
    return y


def s2d(x):
    """DownSampleBlock: [n, g*g, C] -> [n, ceil(g/2)^2, 4C]."""
    _dev(x)
    n, Lx, Cc = x.shape
    g = int(Lx ** 0.5)
    hb = (g + 1) // 2
    y = torch.empty((n, hb * hb, 4 * Cc), device=x.device, dtype=x.dtype)
    L.check(L.load().srgpt_s2d(_p(_c(x)), _p(y), n, g, Cc, dt_code(x), _stream()))
    return y


def im2col(images, patch, kp):
    _dev(images)
    n, ch, S, _ = images.shape
    assert ch == 3
    g = S // patch
    out = torch.empty((n * g * g, kp), device=images.device, dtype=images.dtype)
    L.check(L.load().srgpt_im2col(_p(_c(images)), _p(out), n, S, patch, kp, dt_code(images), _stream()))
    return out


def embed_rows(table, ids):
    """rows of `table` at `ids`; ids must already be validated against the table height (engine._check_ids)."""
    _dev(table, ids)
    ids = _c(ids.to(torch.int64)).reshape(-1)
    out = torch.empty((ids.numel(), table.shape[1]), device=table.device, dtype=table.dtype)
    L.check(L.load().srgpt_embed_rows(_p(table), _p(ids), _p(out), ids.numel(), table.shape[1], dt_code(table), _stream()))
    return out


def rows_match(a: torch.Tensor, b: torch.Tensor, rows: int, out: torch.Tensor) -> torch.Tensor:
    """out[0] (int32, device) = the number of leading rows of `a` equal to the same rows of `b` BYTE FOR BYTE (srgpt_rows_match);
    a, b: contiguous tensors of one dtype (torch slices at any alignment) whose first `rows` entries along dim 0 are compared.
    Only enqueues: the caller reads `out` back with whatever else it reads."""
    _dev(a, b, out)
    _same_dtype("rows_match", a, b=b)
    assert a.is_contiguous() and b.is_contiguous() and out.dtype == torch.int32 and out.numel() >= 1
    row_bytes = (a[0].numel() if a.dim() > 0 and a.shape[0] > 0 else 1) * a.element_size()
    if rows > 0 and (a.shape[0] < rows or b.shape[0] < rows or a.shape[1:] != b.shape[1:]):
        raise ValueError(f"rows_match: {rows} rows of {tuple(a.shape)} against {tuple(b.shape)}")
    L.check(L.load().srgpt_rows_match(_p(a), _p(b), int(rows), max(int(row_bytes), 1), _p(out), _stream()))
    return out


def splice_match(desc_new, len_new: int, desc_old, n_old_rows: int, gen_old, n_gen_old: int, n_regions_common: int,
                 out: torch.Tensor) -> torch.Tensor:
    """out[0] (int32, device) = the leading rows of ONE prompt's splice table `desc_new` [>= len_new, 2] that name the sources of the
    old row sequence: `desc_old`'s first n_old_rows rows, then the ids gen_old[:n_gen_old] (int64) as text rows; region rows beyond
    `n_regions_common` never match (srgpt_splice_match).  Only enqueues."""
    _dev(desc_new, desc_old, gen_old, out)
    assert desc_new.dtype == torch.int32 and desc_old.dtype == torch.int32 and gen_old.dtype == torch.int64 and out.dtype == torch.int32
    assert desc_new.is_contiguous() and desc_old.is_contiguous() and gen_old.is_contiguous() and out.numel() >= 1
    if len_new * 2 > desc_new.numel() or n_old_rows * 2 > desc_old.numel() or n_gen_old > gen_old.numel():
        raise ValueError("splice_match: a length exceeds its table")
    L.check(L.load().srgpt_splice_match(_p(desc_new), int(len_new), _p(desc_old), int(n_old_rows), _p(gen_old), int(n_gen_old),
                                        int(n_regions_common), _p(out), _stream()))
    return out


def scatter_rows(src, idx, dst, src_idx=None):
    """dst[idx[i]] = src[src_idx[i] if src_idx is given else i]"""
    _dev(src, idx, dst, src_idx)
    _same_dtype("scatter_rows", src, dst=dst)
    assert idx.dtype == torch.int32 and src.is_contiguous() and dst.is_contiguous()
    assert src_idx is None or (src_idx.dtype == torch.int32 and src_idx.numel() == idx.numel())
    n = idx.numel()
    if n == 0:
        return dst
    L.check(L.load().srgpt_scatter_rows(_p(src), _p(src_idx), _p(idx), _p(dst), n, src.shape[-1], dt_code(src), _stream()))
    return dst


def silu_mul(gu):
    _dev(gu)
    rows, two_i = gu.shape
    out = torch.empty((rows, two_i // 2), device=gu.device, dtype=gu.dtype)
    L.check(L.load().srgpt_silu_mul(_p(_c(gu)), _p(out), rows, two_i // 2, dt_code(gu), _stream()))
    return out


def argmax(logits):
    _dev(logits)
    assert logits.dtype == torch.float32 and logits.is_contiguous()
    B, V = logits.shape
    out = torch.empty((B,), device=logits.device, dtype=torch.int64)
    L.check(L.load().srgpt_argmax(_p(logits), _p(out), B, V, _stream()))
    return out


def cross_entropy(shift_logits: torch.Tensor, shift_labels: torch.Tensor, ignore_index: int = -100):
    """mean cross entropy over the rows whose label is not `ignore_index`: shift_logits fp32 [rows, V] (already shifted),
    shift_labels int64 [rows].  Returns (loss 0-d fp32 tensor, number of targets 0-d tensor)."""
    _dev(shift_logits, shift_labels)
    if shift_logits.dtype != torch.float32 or shift_labels.dtype != torch.int64:
        raise ValueError("cross_entropy: logits must be fp32 and labels int64")
    rows, V = shift_logits.shape
    row_loss = torch.empty((rows,), device=shift_logits.device, dtype=torch.float32)
    out = torch.empty((2,), device=shift_logits.device, dtype=torch.float32)
    L.check(L.load().srgpt_cross_entropy(_p(_c(shift_logits)), _p(_c(shift_labels)), _p(row_loss), _p(out), rows, V,
                                         int(ignore_index), _stream()))
    return out[0], out[1]


class SamplingParams:
    """The device-resident parameter block of the device-side draw (srgpt_sampling, include/srgpt.h): temperature -> top-k ->
    top-p -> categorical, HF GenerationMixin.sample's warper chain.  `supported()` says whether a setting is served by the top-k-64
    sampler (top_k 1..64 with any top_p; or no top-k and no top-p: pure temperature sampling by Gumbel-max); `sampler()` says which
    device sampler serves a setting at all (the full sampler takes every other one)."""

    def __init__(self, device, batch: int, keep_kept_sets: bool = False):
        self.device = torch.device(device)
        self.buf = torch.zeros((C.sizeof(L.Sampling),), dtype=torch.uint8, device=self.device)
        self.kept = torch.zeros((batch, L.SAMPLING_KEPT_MAX + 1), dtype=torch.int32, device=self.device) if keep_kept_sets else None
        self.host = L.Sampling()

    @staticmethod
    def supported(temperature, top_k, top_p, vocab: int) -> bool:
        if temperature is None or not temperature > 0 or vocab > L.SAMPLING_VOCAB_MAX:
            return False
        k = 0 if top_k is None else int(top_k)
        p_on = top_p is not None and top_p < 1.0
        if k == 0:
            return not p_on
        return 1 <= k <= L.SAMPLING_TOP_K_MAX

    @staticmethod
    def sampler(temperature, top_k, top_p, vocab: int) -> Optional[int]:
        """L.SAMPLER_TOPK64 where `supported()`, else L.SAMPLER_FULL for any temperature > 0 over a vocabulary <= 262144; None:
        no device sampler serves the setting."""
        if temperature is None or not temperature > 0 or vocab > L.SAMPLING_VOCAB_MAX:
            return None
        return L.SAMPLER_TOPK64 if SamplingParams.supported(temperature, top_k, top_p, vocab) else L.SAMPLER_FULL

    def set(self, temperature: float, top_k, top_p, seed: int, counter: int = 0):
        """one small H2D copy on the current stream"""
        h = self.host
        h.temperature = float(temperature)
        h.top_k = 0 if top_k is None else min(int(top_k), 2 ** 31 - 1)  # any top_k >= V means V
        tp = 1.0 if top_p is None else float(top_p)
        h.top_p = tp
        h.top_p_rm = float(torch.tensor(1.0 - tp, dtype=torch.float64).to(torch.float32))  # HF compares against (1 - top_p) in fp32
        h.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        h.counter = int(counter)
        h.kept_out = None if self.kept is None else self.kept.data_ptr()
        src = torch.frombuffer(bytearray(bytes(h)), dtype=torch.uint8)
        self.buf.copy_(src, non_blocking=False)
        return self

    def ptr(self):
        return self.buf.data_ptr()


def _seq_rows(logits: torch.Tensor, steps: torch.Tensor, T: int):
    """the (steps, B, T) of a `_seq_rows` call, checked: logits [B * T, V], steps int32 [B] on the device"""
    _dev(steps)
    B, T = int(steps.numel()), int(T)
    if steps.dtype != torch.int32 or not steps.is_contiguous() or B < 1 or T < 1 or logits.ndim != 2 or logits.shape[0] != B * T:
        raise ValueError("sample_seq_rows: steps must be int32 [B] and logits fp32 [B * T, V]")
    return steps, B, T


def _sample(entry: str, logits: torch.Tensor, params: SamplingParams, check: bool, out: Optional[torch.Tensor], seq=None) -> torch.Tensor:
    """seq = (steps, B, T): an entry over B sequences x T steps, which takes the counts behind the block and (B, T) for the rows"""
    _dev(logits)
    if logits.dtype != torch.float32 or logits.ndim != 2:
        raise ValueError("sample: logits must be fp32 [B, V]")
    B, V = logits.shape
    lib = L.load()
    ws = torch.empty((lib.srgpt_sample_ws_bytes(B),), dtype=torch.uint8, device=logits.device)
    if out is None:
        out = torch.empty((B,), dtype=torch.int64, device=logits.device)
    else:
        _dev(out)
        assert out.dtype == torch.int64 and out.is_contiguous() and out.numel() == B
    if seq is None:
        L.check(getattr(lib, entry)(_p(_c(logits)), params.ptr(), _p(out), _p(ws), B, V, _stream()))
    else:
        L.check(getattr(lib, entry)(_p(_c(logits)), params.ptr(), _p(seq[0]), _p(out), _p(ws), seq[1], seq[2], V, _stream()))
    if check:  # settings the device sampler does not serve raise instead of drawing from a clamped distribution
        L.check(lib.srgpt_sample_status(_p(ws), B, _stream()))
    return out


def sample(logits: torch.Tensor, params: SamplingParams, check: bool = False) -> torch.Tensor:
    """one draw per row of fp32 logits [B, V] with the device-side sampler; advances params' counter.  -> int64 [B]"""
    return _sample("srgpt_sample", logits, params, check, None)


def sample_rows(logits: torch.Tensor, params: SamplingParams, check: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """srgpt_sample_rows: the rows of fp32 logits [T, V] are T successive steps of ONE sequence -- row t draws at params' counter + t,
    what T calls of `sample` on the rows one by one return; advances the counter by T.  `out` (int64 [T], optional): where the ids go.
    A kept-set hook (SamplingParams(keep_kept_sets=True)) must hold T rows.  -> int64 [T]"""
    return _sample("srgpt_sample_rows", logits, params, check, out)


def sample_seq_rows(logits: torch.Tensor, params: SamplingParams, steps: torch.Tensor, T: int, check: bool = False,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """srgpt_sample_seq_rows: the rows of fp32 logits [B * T, V] are B sequences x T successive steps (row b * T + t) that have emitted
    steps[b] ids (int32 [B] on the device).  With m = min max(steps, 0), row (b, t) draws where row b of a B-row `sample` call at
    params' counter + (max(steps[b], 0) - m) + t draws.  The counter is NOT advanced.  A kept-set hook must hold B * T rows.
    -> int64 [B * T]"""
    return _sample("srgpt_sample_seq_rows", logits, params, check, out, _seq_rows(logits, steps, T))


def sample_full(logits: torch.Tensor, params: SamplingParams, kept_mask: bool = False):
    """one draw per row of fp32 logits [B, V] with the full device sampler (every temperature / top_k / top_p); advances params'
    counter.  -> int64 [B], or (ids, kept bool [B, V]) with kept_mask=True (the kept set, the parity hook)."""
    return _sample_full("srgpt_sample_full", logits, params, kept_mask, None)


def sample_full_rows(logits: torch.Tensor, params: SamplingParams, kept_mask: bool = False, out: Optional[torch.Tensor] = None):
    """srgpt_sample_full_rows: `sample_full` over rows that are T successive steps of ONE sequence (row t draws at params' counter + t;
    the counter advances by T).  `out` (int64 [T], optional): where the ids go.  -> int64 [T], or (ids, kept bool [T, V])"""
    return _sample_full("srgpt_sample_full_rows", logits, params, kept_mask, out)


def sample_full_seq_rows(logits: torch.Tensor, params: SamplingParams, steps: torch.Tensor, T: int, kept_mask: bool = False,
                         out: Optional[torch.Tensor] = None):
    """srgpt_sample_full_seq_rows: `sample_full` over rows that are B sequences x T successive steps, addressed as `sample_seq_rows`
    addresses them; the counter is NOT advanced.  -> int64 [B * T], or (ids, kept bool [B * T, V])"""
    return _sample_full("srgpt_sample_full_seq_rows", logits, params, kept_mask, out, _seq_rows(logits, steps, T))


def _sample_full(entry: str, logits: torch.Tensor, params: SamplingParams, kept_mask: bool, out: Optional[torch.Tensor], seq=None):
    _dev(logits)
    if logits.dtype != torch.float32 or logits.ndim != 2:
        raise ValueError("sample_full: logits must be fp32 [B, V]")
    B, V = logits.shape
    lib = L.load()
    nbytes = lib.srgpt_sample_full_ws_bytes(B, V)
    if nbytes < 0:
        raise ValueError("sample_full: empty shape")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=logits.device)
    if out is None:
        out = torch.empty((B,), dtype=torch.int64, device=logits.device)
    else:
        _dev(out)
        assert out.dtype == torch.int64 and out.is_contiguous() and out.numel() == B
    nw = (V + 31) // 32
    mask = torch.empty((B, nw), dtype=torch.int32, device=logits.device) if kept_mask else None
    if seq is None:
        L.check(getattr(lib, entry)(_p(_c(logits)), params.ptr(), _p(out), _p(mask), _p(ws), B, V, _stream()))
    else:
        L.check(getattr(lib, entry)(_p(_c(logits)), params.ptr(), _p(seq[0]), _p(out), _p(mask), _p(ws), seq[1], seq[2], V, _stream()))
    if not kept_mask:
        return out
    bits = torch.arange(32, device=logits.device, dtype=torch.int32)
    kept = ((mask[:, :, None] >> bits) & 1).bool().reshape(B, nw * 32)[:, :V]
    return out, kept


class LogitsProcParams:
    """The device-resident parameter block of the logits processors (srgpt_logits_proc, include/srgpt.h): HF's
    RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and MinLength / MinNewTokensLength processors.  One address for
    the owner's lifetime (a captured decode step holds it); `set()` rewrites the contents."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.buf = torch.zeros((C.sizeof(L.LogitsProc),), dtype=torch.uint8, device=self.device)
        self.host = L.LogitsProc()
        self.set()

    @staticmethod
    def active(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, eos_token_ids=None) -> bool:
        """does this setting change any score?  (a minimum length without an EOS id bans nothing)"""
        return bool((repetition_penalty is not None and float(repetition_penalty) != 1.0) or int(no_repeat_ngram_size or 0) > 0
                    or (int(min_new_tokens or 0) > 0 and eos_token_ids))

    def set(self, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, eos_token_ids=None):
        """one small H2D copy on the current stream"""
        eos = [int(e) for e in (eos_token_ids or [])] if int(min_new_tokens or 0) > 0 else []
        if len(eos) > L.LOGITS_PROC_EOS_MAX:
            raise NotImplementedError(f"a minimum length with {len(eos)} EOS ids (the device block holds {L.LOGITS_PROC_EOS_MAX})")
        h = self.host
        h.repetition_penalty = 1.0 if repetition_penalty is None else float(repetition_penalty)
        h.no_repeat_ngram = min(int(no_repeat_ngram_size or 0), 2 ** 31 - 1)
        h.min_new_tokens = min(int(min_new_tokens or 0), 2 ** 31 - 1)
        h.n_eos = len(eos)
        for j in range(L.LOGITS_PROC_EOS_MAX):
            h.eos[j] = eos[j] if j < len(eos) else 0
        self.buf.copy_(torch.frombuffer(bytearray(bytes(h)), dtype=torch.uint8), non_blocking=False)
        return self

    def ptr(self):
        return self.buf.data_ptr()


def logits_process(scores: torch.Tensor, params: LogitsProcParams, ids: torch.Tensor, n) -> torch.Tensor:
    """the logits processors of `params` over fp32 scores [B, V], IN PLACE; ids int64 [B, ld], the first n of a row are its history.
    n: an int, or a device int32 tensor of one element (read by the kernel, clamped to ld).  Returns `scores`."""
    _dev(scores, ids)
    if scores.dtype != torch.float32 or scores.ndim != 2 or not scores.is_contiguous():
        raise ValueError("logits_process: scores must be contiguous fp32 [B, V]")
    if ids.dtype != torch.int64 or ids.ndim != 2 or ids.shape[0] != scores.shape[0]:
        raise ValueError("logits_process: ids must be int64 [B, ld]")
    B, V = scores.shape
    ids = _c(ids)
    n_dev = None
    if isinstance(n, torch.Tensor):
        _dev(n)
        if n.dtype != torch.int32 or n.numel() != 1:
            raise ValueError("logits_process: a device count must be one int32")
        n_dev, n = n, 0
    L.check(L.load().srgpt_logits_process(_p(scores), params.ptr(), _p(ids), ids.shape[1], int(n), _p(n_dev), B, V, _stream()))
    return scores
