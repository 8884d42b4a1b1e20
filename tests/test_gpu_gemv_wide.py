"""The wide weight pass of the MFMA decode products (srgpt_gemv_rowss_wide, srgpt_gemv_w4p_wide; the NI = 16 instances of skinny.hip)
on the GPU, product against product: for R rows, row r of the wide entry's output must be torch.equal to the 16-row entry's output
for that row -- the existing entry called on a 16-row window that holds the row, a pass of the NI = 8 instance.  Inside a wide chunk
of n rows (17 - 32) the windows are [0:16] for r < 16 and [n - 16:n] for r >= 16; a tail of 16 rows or fewer behind a chunk of 32 (33 =
32 + 1, 40 = 32 + 8) is the last pass of the existing entry's call on the 16 rows in front of it and the tail (16 + 1, 16 + 8): the
launch the pass loop gives it.  The published statistics
slots and the outputs of a consumer fed with the tables are compared the same way.  Outputs and tables sit between rows of NaN.

Data: activations N(0, 1) * 0.5, weights N(0, 0.02), seeded.  Shapes (N, K) at 256 CUs: (4096, 4096) one tile per block, NW = 4;
(6144, 4096) NW = 8, cw = 24, a partial second tile; (14336, 4096) SwiGLU, cw = 28, four sub-units; (4096, 14336) a long K range per
wave; (4098, 4096) N % 16 != 0, a short last block, fp32 out; (40960, 256) cw = 80: two passes of sub-units, waves with one slice or
none; (40, 264) and (17, 64): K % 256 != 0, K below one slice per wave, blocks whose only tile is partial (row-major formats only)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
GUARD = 3  # rows of NaN in front of and behind every output and table
EPS = 1e-5
ROWS = (17, 24, 31, 32)
MORE_ROWS = (33, 40)  # at one shape per format: the pass loop's offsets into x, the residual, out and both tables

# format -> (fp8, packed rows per granule, MXFP4)
FORMATS = {"bf16": (False, 0, False), "fp8": (True, 0, False), "fp8_packed4": (True, 4, False), "fp8_packed16": (True, 16, False),
           "bf16_packed16": (False, 16, False), "mxfp4_packed": (False, 16, True)}
# Products gemv_wide_route keeps at passes of 16 rows: format name -> the route's reason (they are then compared at 16, not skipped)
KEPT_AT_16 = {"bf16_packed16": "the wide instance of packed bf16 weights spills 2 VGPRs: not built"}

# (N, K, fusion): fusion in res (residual in place + ss_out), norm (with ss_in and without), swiglu (+ norm + ss_in), f32 (norm + out_f32),
# plain
SHAPES = [(4096, 4096, "res"), (6144, 4096, "norm"), (14336, 4096, "swiglu"), (4096, 14336, "res"), (4098, 4096, "f32"),
          (40960, 256, "plain"), (40, 264, "norm"), (17, 64, "norm")]


def allowed(fmt, N, K):
    fp8, packed, w4 = FORMATS[fmt]
    if w4:
        return K % 128 == 0 and N % 16 == 0
    if packed:
        return N % packed == 0 and K % 64 == 0
    return True


# the shape at which a format also runs 33 and 40 rows
MORE_AT = {"bf16": (4096, 4096), "fp8": (6144, 4096), "fp8_packed4": (6144, 4096), "fp8_packed16": (4096, 14336),
           "bf16_packed16": (4096, 4096), "mxfp4_packed": (4096, 14336)}
CASES = [(fmt, N, K, fusion) for fmt in FORMATS for N, K, fusion in SHAPES if allowed(fmt, N, K)]


def _ops():
    from spatialrgpt_amd import ops
    return ops


def randn(shape, seed, std):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, device=DEV, generator=g) * std).to(BF16)


@functools.lru_cache(maxsize=4)
def weights(fmt, N, K, swiglu):
    """the matrix of a case in the form its entry takes -> (kwargs of the entry, is_w4); made once per case and left unchanged"""
    ops = _ops()
    fp8, packed, w4 = FORMATS[fmt]
    R = 2 * N if swiglu else N
    w = randn((R, K), 7 * N + K, 0.02)
    if w4:
        codes, scales, _ = ops.quantize_mxfp4_rows(w)
        return dict(packed=ops.pack_mxfp4(codes, scales, swiglu=swiglu), n_rows=R), True
    if fp8:
        w8, sc, _ = ops.quantize_fp8_rows(w)
        if packed:
            return dict(w8=ops.pack_decode_weights(w8, packed), wscale=sc, packed_rows=packed, n_rows=R), False
        return dict(w8=w8, wscale=sc), False
    if packed:
        return dict(w=ops.pack_decode_weights(w, packed), packed_rows=packed, n_rows=R), False
    return dict(w=w), False


def product(wkw, is_w4, x, wide, **kw):
    ops = _ops()
    if is_w4:
        return ops.gemv_w4p(x, wkw["packed"], wkw["n_rows"], wide=wide, **kw)
    return ops.gemv_rowss(x, wide=wide, **wkw, **kw)


def guarded(rows, cols, dtype):
    """-> (buffer of NaN rows, its middle `rows` rows: a contiguous view)"""
    buf = torch.full((rows + 2 * GUARD, cols), float("nan"), device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + rows]


def guards_intact(buf, rows):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + rows:]).all())


def windows(R, chunk):
    """the reference's calls for a call of R rows cut into passes of `chunk`: [(first row of the call, rows of the call, rows taken)]"""
    out = []
    for b0 in range(0, R, chunk):
        n = min(chunk, R - b0)
        if n <= 16 and b0 == 0:
            out.append((0, n, range(0, n)))
        elif n <= 16:  # a tail: the last pass of the existing entry's call on the 16 rows in front of it and the tail (one row alone
            out.append((b0 - 16, 16 + n, range(16, 16 + n)))  # is not a call the entry takes)
        else:
            out.append((b0, 16, range(0, 16)))
            out.append((b0 + n - 16, 16, range(32 - n, 16)))  # rows b0 + 16 .. b0 + n - 1
    return out


def by_windows(R, chunk, call):
    """row r of the result of `call(first, rows)` (a tensor, or a tuple of tensors) on the window that owns r, stacked"""
    parts = None
    for first, n, take in windows(R, chunk):
        res = call(first, n)
        res = res if isinstance(res, tuple) else (res,)
        if parts is None:
            parts = [[] for _ in res]
        for p, t in zip(parts, res):
            p.append(t[take.start:take.stop])
    return tuple(torch.cat(p) for p in parts)


def pass_rows(fmt, R, N, K, norm, swiglu):
    fp8, packed, w4 = FORMATS[fmt]
    return _ops().gemv_wide_pass_rows(R, N, K, fp8=fp8, packed_rows=packed, w4=w4, norm=norm, swiglu=swiglu)


@pytest.mark.parametrize("fmt,N,K,fusion", CASES)
def test_wide_rows_have_the_bits_of_a_16_row_pass(fmt, N, K, fusion):
    ops = _ops()
    swiglu = fusion == "swiglu"
    wkw, is_w4 = weights(fmt, N, K, swiglu)
    norm = fusion in ("norm", "swiglu", "f32")
    gains = (1 + 0.1 * randn((K,), 11, 1.0).float()).to(BF16) if norm else None
    more = MORE_ROWS if (N, K) == MORE_AT[fmt] else ()
    for R in (*ROWS, *more):
        what = "%s N=%d K=%d %s R=%d" % (fmt, N, K, fusion, R)
        chunk = pass_rows(fmt, R, N, K, norm, swiglu)
        assert chunk == (16 if fmt in KEPT_AT_16 else 32), what + ": the route's rows per pass"
        x = randn((R, K), 1000 + R, 0.5)
        if fusion == "res":
            # o_proj / down_proj: the residual add in place (out == residual), publishing the rows' statistics
            h0 = randn((R, N), 2000 + R, 0.5)
            obuf, out = guarded(R, N, BF16)
            out.copy_(h0)
            tbuf, table = guarded(R, 512, F32)
            product(wkw, is_w4, x, True, residual=out, out=out, publish=True, table=table)
            want, want_t = by_windows(R, chunk, lambda a, n: product(wkw, is_w4, x[a:a + n], False, residual=h0[a:a + n], publish=True))
            assert guards_intact(obuf, R) and guards_intact(tbuf, R), what + ": written outside the rows"
            assert torch.equal(out, want), what + ": %d of %d outputs differ" % (int((out != want).sum()), out.numel())
            assert torch.equal(table, want_t), what + ": %d statistics slots differ" % int((table != want_t).sum())
            # a consumer fed with the tables (N = K here or not: the consumer's K is this product's N): a small norm product over them
            cw_kw, c_w4 = weights("bf16", 64, N, False)
            cg = (1 + 0.1 * randn((N,), 12, 1.0).float()).to(BF16)
            cons = product(cw_kw, c_w4, out, True, norm_w=cg, eps=EPS, rowss_in=table)
            c_chunk = pass_rows("bf16", R, 64, N, True, False)
            (cwant,) = by_windows(R, c_chunk, lambda a, n: product(cw_kw, c_w4, want[a:a + n], False, norm_w=cg, eps=EPS,
                                                                  rowss_in=want_t[a:a + n].contiguous()))
            assert torch.equal(cons, cwant), what + ": the consumer of the tables"
            continue
        kw = dict(norm_w=gains, eps=EPS) if norm else {}
        if swiglu:
            kw["swiglu"] = True
        if fusion == "f32":
            kw["out_f32"] = True
        obuf, out = guarded(R, N, F32 if fusion == "f32" else BF16)
        product(wkw, is_w4, x, True, out=out, **kw)
        (want,) = by_windows(R, chunk, lambda a, n: product(wkw, is_w4, x[a:a + n], False, **kw))
        assert guards_intact(obuf, R), what + ": written outside the rows"
        assert torch.equal(out, want), what + ": %d of %d outputs differ" % (int((out != want).sum()), out.numel())
        if norm:
            # the same with the statistics read from a producer's table (ss_in): x and its table from a publishing product
            p_kw, p_w4 = weights("bf16", K, 64, False)
            xin = randn((R, 64), 3000 + R, 0.5)
            h, t = product(p_kw, p_w4, xin, False, residual=x, publish=True)
            obuf, out = guarded(R, N, F32 if fusion == "f32" else BF16)
            product(wkw, is_w4, h, True, out=out, rowss_in=t, **kw)
            (want,) = by_windows(R, chunk, lambda a, n: product(wkw, is_w4, h[a:a + n], False, rowss_in=t[a:a + n].contiguous(), **kw))
            assert guards_intact(obuf, R), what + ": written outside the rows (ss_in)"
            assert torch.equal(out, want), what + " with ss_in: %d of %d outputs differ" % (int((out != want).sum()), out.numel())


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_16_rows_or_fewer_are_the_16_row_entry(fmt):
    N, K = 4096, 4096
    wkw, is_w4 = weights(fmt, N, K, False)
    for R in (1 if is_w4 else 2, 9, 16):
        x = randn((R, K), 4000 + R, 0.5)
        assert pass_rows(fmt, R, N, K, False, False) <= 16
        assert torch.equal(product(wkw, is_w4, x, True), product(wkw, is_w4, x, False)), "%s R=%d" % (fmt, R)
