"""The decode products (srgpt_gemv, srgpt_gemv_w8, srgpt_gemv_rowss; gemv.hip, gemv_w8.hip, skinny.hip) bit for bit on data for which
a correct kernel has ONE possible output, in the manner of tests/test_gpu_gemm_exact.py.

Plain products.  x holds integers in [-7, 7], W integers in [-8, 8] (exact in bf16 and, through ops.quantize_fp8_rows and its
power-of-two scales, in OCP e4m3), the residual integers in [-256, 256]; 56 K + 512 < 2^24, so every fp32 partial sum in every
order is exact.  Reference: float64 `x @ W.T`, then out = rnd(rnd(acc * wscale) + residual), rnd = round to nearest even to bf16;
`out_f32` stores that same bf16-valued number widened (include/srgpt.h); fp32 operands: no rounding at all.  The fp8 cases
multiply the scale of weight row n by 1, 1.25, 1.5 or 1.75 (n % 4) AFTER asserting that codes and power-of-two scales give the
integers back: acc is still an exact integer and `acc * wscale` ONE correctly rounded fp32 product, so the output is still unique,
and a scale applied behind the bf16 rounding now shows (with a power of two it cannot).

RMSNorm prologue (bf16 only: fp32 with a norm cannot be made exact and stays with the tolerance tests of test_gpu_kernels.py).
Every x row is a shuffle of randomly signed copies of the octets (7,7,4,3,2,1,0,0) and (6,6,5,5,2,1,1,0) -- square sum 128 each,
so the mean square is 16 -- times 2^(b % 4 - 1): the rows' statistics differ, the sum of squares is an exact fp32 value in any
order, mean(x^2) = 16 * 4^j exactly, 1 / rms lies within a few ulps of a power of two and rnd(x * r) absorbs that error: with
norm_w integers in [-4, 4] the normalised row is exactly x / rms * norm_w, in quarter units, |.| <= 7, and 4 * 56 K < 2^24 keeps
the sums exact.  _normed() asserts all of this for the case's own data, with r moved by -8, 0, +8 fp32 ulps, before the device call.

SwiGLU.  Integer x, up rows plain integers, gate rows integers times one power of two per case chosen so that max |gate| <= 32
(asserted): __expf stays far from its overflow, where the kernel and a float64 reference legitimately differ.  Reference:
rnd(rnd(silu64(rnd(gate))) * rnd(up)).  The kernels' x / (1 + __expf(-x)) is not correctly rounded, so an element is excluded
(it may take either neighbour) when the float64 silu lies within the relative band BAND of a bf16 rounding boundary.  BAND at
|x| <= 32: __expf(-x) = exp2(fl(-x * log2e)); the product's rounding and the constant's error move the argument by at most
32 log2e (2^-24 + 2^-26), i.e. the exponential by ln2 times that = 40 * 2^-24 relative; one ulp (2^-23) each for v_exp_f32, the add
1 + e and the divide (each propagates to the quotient with a factor <= 1): 46 * 2^-24 = 2.7e-6, times four = 184 * 2^-24 = 1.1e-5
(2^-16.5).  The excluded share is capped at 3 % per case, on the reference alone; every other element must be bit-equal.

Liveness, on the reference alone: every case must tell the documented roundings from wrong ones in at least 1 % of the elements
-- truncation, ties-away, no intermediate rounding before the residual add, the scale behind the rounding (where it is not 1), for
SwiGLU no rounding of silu and no rounding of the gate -- except the K = 8 cases, whose sums need no rounding: they pin the
mapping and the tail.

Surroundings.  x is followed by NaN rows (the MFMA kernel re-reads row B - 1 for rows past the batch), W by NaN rows (0x7F bytes
for fp8), wscale, norm_w and a packed array (copied out of ops.pack_decode_weights into a larger buffer) by NaN / 0x7F / 0xFF, the
residual sits in a larger NaN allocation, `out` is rows 1 ... B of a [B + 2, N] allocation filled with a sentinel that must
survive, a published table rows 1 ... B of a [B + 2, 512] one.  Every call runs twice and the second run's bits equal the first's.

Routes.  Every case names the route (spatialrgpt_amd/csrc/gemv_route.h) it exists for -- family, rows per weight pass and, per
pass, rows and NI / NW / PUB / PK / grid / cw (MFMA kernel) or B / NX / UB / NIT (VALU kernels) -- and asserts it through
tests/gemv_route_cli.cpp at the device's CU count: at 256 CUs another route is a failure, at any other CU count the case skips.

SRGPT_EXACT_LOG=<file> appends the liveness and excluded shares of every case (profiles/gemv_exact.txt was made from it)."""
import json
import math
import os

import pytest
import torch

from tests.util import FP8_NAN, SENTINEL, away, build_gemv_route_cli, check_guarded, exact_f32, guarded, ints, poisoned, rne, trunc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
LIVE_FLOOR = 0.01
BAND = 184 * 2.0 ** -24  # module docstring
EXCLUDED_CAP = 0.03
GATE_BOUND = 32.0
OCTETS = torch.tensor([[7, 7, 4, 3, 2, 1, 0, 0], [6, 6, 5, 5, 2, 1, 1, 0]], dtype=torch.float64)
FP8_SCALE_FACTORS = (1.0, 1.25, 1.5, 1.75)
ROWSS_STRIDE = 512
SLOT_RTOL = 2e-6  # test_gemv_rowss_handoff's bound for the row sum of the table


def _ops():
    from spatialrgpt_amd import _lib, ops
    return ops, _lib


@pytest.fixture(scope="module")
def route_cli(tmp_path_factory):
    return build_gemv_route_cli(tmp_path_factory.mktemp("gemv_route_exact"))


def _log(what, kind, value):
    path = os.environ.get("SRGPT_EXACT_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", ""), "what": what, "kind": kind, "share": value}) + "\n")


SKINNY_KEYS, VALU_KEYS = ("rows", "NI", "NW", "PUB", "PK", "grid", "cw"), ("rows", "B", "NX", "UB", "NIT")


def _assert_route(route_cli, wt, B, N, K, norm, swiglu, ss_in, packed, want):
    """`want` = (family, rows per weight pass, [per pass: (rows, NI, NW, PUB, PK, grid, cw) or (rows, B, NX, UB, NIT)]), recorded
    at 256 CUs; -> the CLI's answer"""
    cus = _ops()[1].load().srgpt_device_cus()
    if cus != 256:
        pytest.skip("the routes of these cases are recorded for 256 CUs, this device has %d" % cus)
    r = route_cli([(wt, B, N, K, int(norm), int(swiglu), int(ss_in), packed)], cus)[0]
    keys = SKINNY_KEYS if r["family"] == "skinny" else VALU_KEYS
    got = (r["family"], r["chunk"], [tuple(p[k] for k in keys) for p in r["passes"]])
    assert got == (want[0], want[1], [tuple(p) for p in want[2]]), \
        "%s rows=%d N=%d K=%d norm=%d swiglu=%d ss_in=%d packed=%d takes %s, the case exists for %s" % (wt, B, N, K, norm, swiglu, ss_in,
                                                                                                        packed, got, want)
    return r


# ------------------------------------------------------------------------------------------------ the CPU side
def _tally(tally, kind, differs):
    """count the elements of a case that a wrong rounding (or the SwiGLU band) tells from the reference"""
    t = tally.setdefault(kind, [0, 0])
    t[0] += int(differs.sum())
    t[1] += differs.numel()


def _assert_tally(what, tally):
    for kind, (n, total) in tally.items():
        _log(what, kind, n / total)
        if kind == "swiglu excluded":
            assert n <= EXCLUDED_CAP * total, "%s: %.2f %% of the elements lie within the band of a rounding boundary" % (what, 100 * n / total)
        else:
            assert n >= LIVE_FLOOR * total, "%s: '%s' differs from the reference in %.2f %% of the elements only" % (what, kind, 100 * n / total)


def _octet_rows(B, K, seed):
    """-> (rows [B, K] float64, their rms [B]): module docstring"""
    assert K % 8 == 0
    g = torch.Generator().manual_seed(seed)
    rows = []
    for b in range(B):
        r = OCTETS[torch.randint(0, 2, (K // 8,), generator=g)].reshape(-1)
        r = r[torch.randperm(K, generator=g)] * (torch.randint(0, 2, (K,), generator=g) * 2 - 1)
        rows.append(r * 2.0 ** (b % 4 - 1))
    return torch.stack(rows), 4 * 2.0 ** (torch.arange(B) % 4 - 1.0).double()


def _normed(x64, rms, nw64, eps, what):
    """the RMSNorm prologue's output for octet rows, exactly x / rms * norm_w: asserted for this data, for any order of the
    statistics' sum and any rsqrtf within 8 ulps"""
    K = x64.shape[1]
    sq = x64 * x64
    assert float(sq.sum(1).max()) * 4 < 2 ** 24 and torch.equal(sq * 4, (sq * 4).round()), what  # exact partial sums in any order
    ms = sq.sum(1) / K
    assert torch.equal(ms, rms * rms) and torch.equal(ms.float().double(), ms), what  # fl32(sum / K) is that number
    want = x64 / rms[:, None] * nw64
    assert torch.equal(want * 4, (want * 4).round()) and float(want.abs().max()) <= 7 and 4 * 56 * K < 2 ** 24, what
    r0 = torch.rsqrt(ms.float() + eps)
    for d in (-8, 0, 8):
        r = (r0.view(torch.int32) + d).view(F32)
        got = (nw64.float() * rne(x64.float() * r[:, None])).to(BF16)  # weight * h.to(dtype), as the kernels round
        assert torch.equal(got.double(), want), "%s: the normalised rows depend on 1 / rms at %+d ulps" % (what, d)
    return want


def _weights(w_i, pow2, fp8):
    """w_i: integer rows [R, K] (float64), pow2 [R]: a power of two per row (1 except for SwiGLU gate rows).  -> (the effective
    scale e [R] of row n: the kernel's sum over the integers times e is its product, operands for the device calls)"""
    ops, _ = _ops()
    w = (w_i * pow2[:, None]).to(BF16)
    assert torch.equal(w.double(), w_i * pow2[:, None])
    if not fp8:
        return pow2.clone(), dict(w=w)
    w8, wscale, deq = ops.quantize_fp8_rows(w)
    assert torch.equal(deq.double(), w_i * pow2[:, None])
    assert torch.equal(w8.view(torch.float8_e4m3fn).float().double() * wscale.double()[:, None], w_i * pow2[:, None])
    assert bool((torch.frexp(wscale)[0] == 0.5).all())  # powers of two
    m = torch.tensor(FP8_SCALE_FACTORS, dtype=torch.float64)[torch.arange(w_i.shape[0]) % 4]
    return pow2 * m, dict(w8=w8, wscale=(wscale.double() * m).float())


def _scaled(acc64, e):
    """fl32(acc * e): acc exact, ONE correctly rounded fp32 product (exact where e is a power of two)"""
    exact_f32(acc64)
    return (acc64 * e[None, :]).float()


def _plain_refs(prod, res, acc64, e, dtype, tally):
    """prod = fl32(acc * e) [B, N], res fp32 or None -> {"plain", "res"} fp32 references; bf16: the liveness of this data into `tally`"""
    if dtype == F32:
        return {"plain": prod, "res": exact_f32(prod.double() + res.double())}
    refs = {"plain": rne(prod)}
    _tally(tally, "plain, truncation", trunc(prod) != refs["plain"])
    _tally(tally, "plain, ties away", away(prod) != refs["plain"])
    if res is not None:
        refs["res"] = rne(rne(prod) + res)
        _tally(tally, "no intermediate rounding", rne((prod.double() + res.double()).float()) != refs["res"])
        _tally(tally, "residual, truncation", trunc(trunc(prod) + res) != refs["res"])
    if bool((torch.frexp(e)[0] != 0.5).any()):
        _tally(tally, "scale behind the rounding", rne((rne(acc64.float()).double() * e[None, :]).float()) != refs["plain"])
    return refs


def _silu64(g):
    return g / (1 + torch.exp(-g))


def _swiglu_refs(pg, pu, what, tally):
    """pg, pu = fl32(acc * e) of the gate and up rows -> (ref, alt) fp32: an element must equal ref, or alt where the float64 silu
    lies within BAND of a rounding boundary (module docstring; elsewhere alt == ref)"""
    g, u = rne(pg), rne(pu)
    assert float(g.abs().max()) <= GATE_BOUND, what
    s64 = _silu64(g.double())
    lo, hi = rne((s64 * (1 - BAND)).float()), rne((s64 * (1 + BAND)).float())
    _tally(tally, "swiglu excluded", lo != hi)
    s = rne(s64.float())
    assert bool(((s == lo) | (s == hi)).all())
    ref = rne(s * u)
    alt = torch.where(s == lo, rne(hi * u), rne(lo * u))
    _tally(tally, "swiglu, silu not rounded", rne((s64 * u.double()).float()) != ref)
    _tally(tally, "swiglu, gate not rounded", rne(rne(_silu64(pg.double()).float()) * u) != ref)
    _tally(tally, "swiglu, truncation", trunc(trunc(s64.float()) * u) != ref)
    return ref, alt


def _gate_pow2(acc_gate, fp8):
    """the power of two that brings the gate rows under GATE_BOUND (fp8: under the largest scale factor too)"""
    top = float(acc_gate.abs().max()) * (max(FP8_SCALE_FACTORS) if fp8 else 1.0)
    return 2.0 ** -max(0, math.ceil(math.log2(max(top, 1.0) / GATE_BOUND)))


# ------------------------------------------------------------------------------------------------ the device side
def _dev_weights(kw, packed, n_rows):
    """the operands of _weights on the device, poisoned behind; packed: through ops.pack_decode_weights into a poisoned buffer"""
    ops, _ = _ops()
    fp8 = "w8" in kw
    key = "w8" if fp8 else "w"
    out = dict(wscale=poisoned(kw["wscale"])) if fp8 else {}
    if not packed:
        out[key] = poisoned(kw[key], rows_after=5, poison=FP8_NAN if fp8 else float("nan"))
        return out
    pk = ops.pack_decode_weights(kw[key].to(DEV), packed)
    big = torch.full((pk.numel() + 4096,), FP8_NAN if fp8 else 0xFF, dtype=torch.uint8, device=DEV)  # 0xFFFF: a bf16 NaN
    big[:pk.numel()] = pk
    out.update({key: big[:pk.numel()], "packed_rows": packed, "n_rows": n_rows})
    return out


def _run_twice(call, B, N, odt, ref, alt, what):
    """call(out) into rows 1 ... B of a sentinel allocation, twice; -> the bits"""
    first = None
    for run in range(2):
        buf, view = guarded(B, N, N, odt, row0=1)
        call(view)
        got = check_guarded(buf, view, ref, what + (", second run" if run else ""), alt=alt)
        idt = SENTINEL[odt][0]
        assert first is None or torch.equal(got.view(idt), first.view(idt)), what + ": run-to-run difference"
        first = got
    return first


def _entry_call(entry, x_d, wkw, norm_w, eps, res, swiglu, out_f32, **extra):
    ops, _ = _ops()
    if entry == "gemv":
        return lambda out: ops.gemv(x_d, wkw["w"], norm_w, eps, res, swiglu, out=out, out_f32=out_f32)
    if entry == "gemv_w8":
        return lambda out: ops.gemv_w8(x_d, wkw["w8"], wkw["wscale"], norm_w, eps, res, swiglu, out=out, out_f32=out_f32)
    assert entry == "rowss"
    return lambda out: ops.gemv_rowss(x_d, norm_w=norm_w, eps=eps, residual=res, swiglu=swiglu, out=out, out_f32=out_f32, **wkw, **extra)


MIN_ELEMENTS = 128


def _product_case(route_cli, entry, wt, B, N, K, norm, swiglu, packed, route):
    """one product with everything of the module docstring: plain, residual and their fp32 forms, or SwiGLU.  A case of fewer than
    MIN_ELEMENTS outputs (N = 1: ONE element, which cannot be a tie and round up at once) runs as many data sets as give it that
    many, and its liveness and its excluded share are those of all of them together."""
    what = "%s %s B=%d N=%d K=%d%s%s%s" % (entry, wt, B, N, K, " norm" if norm else "", " swiglu" if swiglu else "",
                                            " packed %d" % packed if packed else "")
    assert 56 * K + 512 < 2 ** 24 and not (norm and wt == "f32")
    _assert_route(route_cli, wt, B, N, K, norm, swiglu, 0, packed, route)
    tally = {}
    for rep in range(-(-MIN_ELEMENTS // (B * N))):
        _product_once(entry, wt, B, N, K, norm, swiglu, packed, 1000 * B + 7 * N + K + 3 * norm + 5 * swiglu + 7919 * rep, tally, what)
    if K == 8 or wt == "f32":  # sums that need no rounding / no rounding at all: nothing to tell apart
        tally = {k: v for k, v in tally.items() if k == "swiglu excluded"}
    _assert_tally(what, tally)


def _product_once(entry, wt, B, N, K, norm, swiglu, packed, seed, tally, what, eps=1e-5):
    fp8, dtype = wt == "fp8", F32 if wt == "f32" else BF16
    if norm:
        x64, rms = _octet_rows(B, K, seed)
        nw64 = ints((K,), 4, seed + 1)
        xe = _normed(x64, rms, nw64, eps, what)
        norm_w = poisoned(nw64.to(BF16))
    else:
        x64 = xe = ints((B, K), 7, seed)
        norm_w = None
    w_i = ints(((2 if swiglu else 1) * N, K), 8, seed + 2)
    acc = xe @ w_i.T
    pow2 = torch.ones(w_i.shape[0], dtype=torch.float64)
    if swiglu:
        pow2[:N] = _gate_pow2(acc[:, :N], fp8)
    e, wkw = _weights(w_i, pow2, fp8)
    if dtype == F32:
        wkw = dict(w=w_i.float())
    prod = _scaled(acc, e)
    assert torch.equal(x64.to(dtype).double(), x64)
    x_d = poisoned(x64.to(dtype))
    wkw = _dev_weights(wkw, packed, w_i.shape[0])
    if swiglu:
        assert dtype == BF16  # (fp32 SwiGLU is not exact: with the tolerance tests)
        ref, alt = _swiglu_refs(prod[:, :N], prod[:, N:], what, tally)
        _run_twice(_entry_call(entry, x_d, wkw, norm_w, eps, None, True, False), B, N, BF16, ref.to(BF16).to(DEV), alt.to(BF16).to(DEV), what)
        return
    res_i = ints((B, N), 256, seed + 3)
    refs = _plain_refs(prod, res_i.float(), acc, e, dtype, tally)
    res_d = poisoned(res_i.to(dtype))
    for epi in ("plain", "res"):
        for out_f32 in (False, True) if dtype == BF16 else (False,):
            odt = F32 if out_f32 else dtype
            call = _entry_call(entry, x_d, wkw, norm_w, eps, res_d if epi == "res" else None, False, out_f32)
            _run_twice(call, B, N, odt, refs[epi].to(dtype).to(odt).to(DEV), None, "%s, %s%s" % (what, epi, " -> fp32" if out_f32 else ""))


# entry, weights (bf16 / f32 / fp8), B, N, K, norm, swiglu, packed granule, the route at 256 CUs, what the case pins
CASES = [
    ('gemv', 'bf16', 1, 37, 2560, 0, 0, 0, ('gemv_reg', 1, [(1, 1, 2, 8, 5)]),
     'gemv_reg_kernel NIT 5'),
    ('gemv', 'bf16', 1, 21, 2560, 0, 1, 0, ('gemv_reg', 1, [(1, 1, 2, 8, 5)]),
     'gemv_reg_kernel SwiGLU NIT 5'),
    ('gemv', 'bf16', 1, 37, 4096, 0, 0, 0, ('gemv_reg', 1, [(1, 1, 2, 8, 8)]),
     'gemv_reg_kernel NIT 8'),
    ('gemv', 'bf16', 1, 21, 4096, 0, 1, 0, ('gemv_reg', 1, [(1, 1, 2, 8, 8)]),
     'gemv_reg_kernel SwiGLU NIT 8'),
    ('gemv', 'bf16', 1, 37, 6912, 0, 0, 0, ('gemv_reg', 1, [(1, 1, 8, 8, 14)]),
     'gemv_reg_kernel NIT 14'),
    ('gemv', 'bf16', 1, 21, 6912, 0, 1, 0, ('gemv_reg', 1, [(1, 1, 8, 8, 14)]),
     'gemv_reg_kernel SwiGLU NIT 14'),
    ('gemv', 'bf16', 1, 37, 2056, 0, 0, 0, ('gemv_reg', 1, [(1, 1, 2, 8, 5)]),
     'gemv_reg_kernel NIT 5, the last iteration a partial chunk'),
    ('gemv', 'bf16', 1, 21, 2056, 0, 1, 0, ('gemv_reg', 1, [(1, 1, 2, 8, 5)]),
     'gemv_reg_kernel SwiGLU NIT 5, the last iteration a partial chunk'),
    ('gemv', 'bf16', 1, 37, 6664, 0, 0, 0, ('gemv_reg', 1, [(1, 1, 8, 8, 14)]),
     'gemv_reg_kernel NIT 14, the last iteration a partial chunk'),
    ('gemv', 'bf16', 1, 21, 6664, 0, 1, 0, ('gemv_reg', 1, [(1, 1, 8, 8, 14)]),
     'gemv_reg_kernel SwiGLU NIT 14, the last iteration a partial chunk'),
    ('gemv', 'bf16', 1, 8197, 2056, 0, 0, 0, ('gemv_reg', 1, [(1, 1, 2, 8, 5)]),
     'gemv_reg_kernel, a wave owns more units than its residual prefetch holds'),
    ('gemv', 'bf16', 1, 5, 8, 0, 0, 0, ('gemv', 1, [(1, 1, 2, 8, 1)]),
     'gemv_kernel one chunk (mapping and tail: no rounding)'),
    ('gemv', 'bf16', 1, 37, 264, 0, 0, 0, ('gemv', 1, [(1, 1, 2, 8, 1)]),
     'gemv_kernel NX 2, one partial iteration'),
    ('gemv', 'bf16', 1, 21, 264, 0, 1, 0, ('gemv', 1, [(1, 1, 2, 8, 1)]),
     'gemv_kernel SwiGLU'),
    ('gemv', 'bf16', 1, 37, 264, 1, 0, 0, ('gemv', 1, [(1, 1, 2, 8, 1)]),
     'gemv_kernel norm, small K'),
    ('gemv', 'bf16', 1, 37, 4096, 1, 0, 0, ('gemv', 1, [(1, 1, 2, 8, 8)]),
     'gemv_kernel norm, NX 2 at its limit'),
    ('gemv', 'bf16', 1, 37, 4104, 0, 0, 0, ('gemv', 1, [(1, 1, 8, 8, 9)]),
     'gemv_kernel NX 8'),
    ('gemv', 'bf16', 1, 21, 4104, 0, 1, 0, ('gemv', 1, [(1, 1, 8, 8, 9)]),
     'gemv_kernel SwiGLU NX 8'),
    ('gemv', 'bf16', 1, 37, 7168, 1, 0, 0, ('gemv', 1, [(1, 1, 8, 7, 14)]),
     'gemv_kernel norm, batches of 7 loads'),
    ('gemv', 'bf16', 1, 37, 10752, 0, 0, 0, ('gemv', 1, [(1, 1, 8, 7, 21)]),
     'gemv_kernel batches of 7 loads'),
    ('gemv', 'bf16', 1, 200, 16392, 0, 0, 0, ('gemv', 1, [(1, 1, 8, 8, 33)]),
     'gemv_kernel, the prologue loops past 2048 chunks'),
    ('gemv', 'bf16', 1, 200, 16392, 1, 0, 0, ('gemv', 1, [(1, 1, 8, 8, 33)]),
     'gemv_kernel norm, the prologue loops past 2048 chunks'),
    ('gemv', 'bf16', 1, 200, 24640, 0, 0, 0, ('gemv', 1, [(1, 1, 8, 7, 49)]),
     'gemv_kernel, the LDS limit is raised'),
    ('gemv', 'bf16', 1, 200, 35848, 0, 0, 0, ('gemv', 1, [(1, 1, 8, 8, 71)]),
     'gemv_kernel, one block per CU'),
    ('gemv', 'bf16', 1, 1, 264, 0, 0, 0, ('gemv', 1, [(1, 1, 2, 8, 1)]),
     'gemv_kernel N = 1'),
    ('gemv', 'bf16', 1, 3, 264, 0, 0, 0, ('gemv', 1, [(1, 1, 2, 8, 1)]),
     'gemv_kernel N = 3: fewer units than waves'),
    ('gemv', 'bf16', 1, 2051, 264, 0, 0, 0, ('gemv', 1, [(1, 1, 2, 8, 1)]),
     'gemv_kernel, waves take several units'),
    ('gemv', 'bf16', 1, 8197, 264, 0, 0, 0, ('gemv', 1, [(1, 1, 2, 8, 1)]),
     'gemv_kernel, a wave owns more units than its residual prefetch holds'),
    ('gemv', 'f32', 1, 37, 268, 0, 0, 0, ('gemv', 1, [(1, 1, 2, 8, 2)]),
     'gemv_kernel fp32, 1 row(s)'),
    ('gemv', 'f32', 2, 37, 268, 0, 0, 0, ('gemv', 2, [(2, 2, 2, 8, 2)]),
     'gemv_kernel fp32, 2 row(s)'),
    ('gemv', 'f32', 3, 37, 268, 0, 0, 0, ('gemv', 3, [(3, 3, 2, 8, 2)]),
     'gemv_kernel fp32, 3 row(s)'),
    ('gemv', 'f32', 4, 37, 268, 0, 0, 0, ('gemv', 4, [(4, 4, 2, 8, 2)]),
     'gemv_kernel fp32, 4 row(s)'),
    ('gemv', 'f32', 5, 9, 9608, 0, 0, 0, ('gemv', 3, [(3, 3, 8, 8, 38), (2, 2, 8, 8, 38)]),
     'gemv_kernel fp32, the LDS cap cuts the chunk to 3: passes 3 + 2'),
    ('gemv', 'f32', 9, 37, 36, 0, 0, 0, ('gemv', 4, [(4, 4, 2, 8, 1), (4, 4, 2, 8, 1), (1, 1, 2, 8, 1)]),
     'gemv_kernel fp32, passes 4 + 4 + 1'),
    ('gemv', 'f32', 4, 9, 2560, 0, 0, 0, ('gemv', 4, [(4, 4, 8, 8, 10)]),
     'gemv_kernel fp32, the looping prologue'),
    ('gemv_w8', 'fp8', 1, 37, 256, 0, 0, 0, ('gemv_w8', 1, [(1, 1, 2, 8, 0)]),
     'gemv_w8_kernel NX 2, odd N: the last unit half filled'),
    ('gemv_w8', 'fp8', 1, 38, 4112, 0, 0, 0, ('gemv_w8', 1, [(1, 1, 8, 8, 0)]),
     'gemv_w8_kernel NX 8'),
    ('gemv_w8', 'fp8', 1, 16391, 256, 0, 0, 0, ('gemv_w8', 1, [(1, 1, 2, 8, 0)]),
     'gemv_w8_kernel, a wave owns more units than its residual prefetch holds, odd N'),
    ('gemv_w8', 'fp8', 1, 37, 1024, 1, 0, 0, ('gemv_w8', 1, [(1, 1, 2, 8, 0)]),
     'gemv_w8_kernel norm'),
    ('gemv_w8', 'fp8', 1, 21, 1024, 0, 1, 0, ('gemv_w8', 1, [(1, 1, 2, 8, 0)]),
     'gemv_w8_kernel SwiGLU, odd N'),
    ('gemv_w8', 'fp8', 1, 6, 4112, 0, 1, 0, ('gemv_w8', 1, [(1, 1, 8, 8, 0)]),
     'gemv_w8_kernel SwiGLU NX 8'),
    ('gemv_w8', 'fp8', 1, 200, 16400, 0, 0, 0, ('gemv_w8', 1, [(1, 1, 8, 8, 0)]),
     'gemv_w8_kernel, the looping prologue: 2050 activation chunks'),
    ('gemv_w8', 'fp8', 1, 200, 16400, 1, 0, 0, ('gemv_w8', 1, [(1, 1, 8, 8, 0)]),
     'gemv_w8_kernel norm, the looping prologue'),
    ('gemv_w8', 'fp8', 1, 37, 264, 0, 0, 0, ('skinny', 16, [(1, 2, 4, 0, 0, 3, 16)]),
     'one fp8 row, K % 16 != 0: skinny_kernel with a batch of 1'),
    ('gemv_w8', 'fp8', 1, 37, 264, 1, 0, 0, ('skinny', 16, [(1, 2, 8, 0, 0, 3, 16)]),
     'one fp8 row, K % 16 != 0, norm'),
    ('gemv_w8', 'fp8', 1, 24, 264, 0, 1, 0, ('skinny', 16, [(1, 2, 4, 0, 0, 2, 16)]),
     'one fp8 row, K % 16 != 0, SwiGLU'),
    ('gemv', 'bf16', 2, 50, 264, 0, 0, 0, ('skinny', 16, [(2, 2, 4, 0, 0, 4, 16)]),
     'skinny_kernel 2 rows, NW 4'),
    ('gemv', 'bf16', 2, 50, 264, 1, 0, 0, ('skinny', 16, [(2, 2, 8, 0, 0, 4, 16)]),
     'skinny_kernel 2 rows, norm: NW 8'),
    ('gemv', 'bf16', 3, 50, 264, 0, 0, 0, ('skinny', 16, [(3, 2, 4, 0, 0, 4, 16)]),
     'skinny_kernel 3 rows, NW 4'),
    ('gemv', 'bf16', 3, 50, 264, 1, 0, 0, ('skinny', 16, [(3, 2, 8, 0, 0, 4, 16)]),
     'skinny_kernel 3 rows, norm: NW 8'),
    ('gemv', 'bf16', 4, 50, 264, 0, 0, 0, ('skinny', 16, [(4, 2, 4, 0, 0, 4, 16)]),
     'skinny_kernel 4 rows, NW 4'),
    ('gemv', 'bf16', 4, 50, 264, 1, 0, 0, ('skinny', 16, [(4, 2, 8, 0, 0, 4, 16)]),
     'skinny_kernel 4 rows, norm: NW 8'),
    ('gemv', 'bf16', 5, 50, 264, 0, 0, 0, ('skinny', 16, [(5, 4, 4, 0, 0, 4, 16)]),
     'skinny_kernel 5 rows, NW 4'),
    ('gemv', 'bf16', 5, 50, 264, 1, 0, 0, ('skinny', 16, [(5, 4, 8, 0, 0, 4, 16)]),
     'skinny_kernel 5 rows, norm: NW 8'),
    ('gemv', 'bf16', 8, 50, 264, 0, 0, 0, ('skinny', 16, [(8, 4, 4, 0, 0, 4, 16)]),
     'skinny_kernel 8 rows, NW 4'),
    ('gemv', 'bf16', 8, 50, 264, 1, 0, 0, ('skinny', 16, [(8, 4, 8, 0, 0, 4, 16)]),
     'skinny_kernel 8 rows, norm: NW 8'),
    ('gemv', 'bf16', 9, 50, 264, 0, 0, 0, ('skinny', 16, [(9, 8, 4, 0, 0, 4, 16)]),
     'skinny_kernel 9 rows, NW 4'),
    ('gemv', 'bf16', 9, 50, 264, 1, 0, 0, ('skinny', 16, [(9, 8, 8, 0, 0, 4, 16)]),
     'skinny_kernel 9 rows, norm: NW 8'),
    ('gemv', 'bf16', 16, 50, 264, 0, 0, 0, ('skinny', 16, [(16, 8, 4, 0, 0, 4, 16)]),
     'skinny_kernel 16 rows, NW 4'),
    ('gemv', 'bf16', 16, 50, 264, 1, 0, 0, ('skinny', 16, [(16, 8, 8, 0, 0, 4, 16)]),
     'skinny_kernel 16 rows, norm: NW 8'),
    ('gemv', 'bf16', 17, 50, 264, 0, 0, 0, ('skinny', 16, [(16, 8, 4, 0, 0, 4, 16), (1, 2, 4, 0, 0, 4, 16)]),
     'skinny_kernel 17 rows, NW 4'),
    ('gemv', 'bf16', 17, 50, 264, 1, 0, 0, ('skinny', 16, [(16, 8, 8, 0, 0, 4, 16), (1, 2, 8, 0, 0, 4, 16)]),
     'skinny_kernel 17 rows, norm: NW 8'),
    ('gemv', 'bf16', 33, 50, 264, 0, 0, 0, ('skinny', 16, [(16, 8, 4, 0, 0, 4, 16), (16, 8, 4, 0, 0, 4, 16), (1, 2, 4, 0, 0, 4, 16)]),
     'skinny_kernel 33 rows, NW 4'),
    ('gemv', 'bf16', 33, 50, 264, 1, 0, 0, ('skinny', 16, [(16, 8, 8, 0, 0, 4, 16), (16, 8, 8, 0, 0, 4, 16), (1, 2, 8, 0, 0, 4, 16)]),
     'skinny_kernel 33 rows, norm: NW 8'),
    ('gemv', 'bf16', 2, 24, 264, 0, 1, 0, ('skinny', 16, [(2, 2, 4, 0, 0, 2, 16)]),
     'skinny_kernel SwiGLU 2 rows, NW 4'),
    ('gemv', 'bf16', 2, 24, 264, 1, 1, 0, ('skinny', 16, [(2, 2, 8, 0, 0, 2, 16)]),
     'skinny_kernel SwiGLU 2 rows, norm: NW 8'),
    ('gemv', 'bf16', 5, 24, 264, 0, 1, 0, ('skinny', 16, [(5, 4, 4, 0, 0, 2, 16)]),
     'skinny_kernel SwiGLU 5 rows, NW 4'),
    ('gemv', 'bf16', 5, 24, 264, 1, 1, 0, ('skinny', 16, [(5, 4, 8, 0, 0, 2, 16)]),
     'skinny_kernel SwiGLU 5 rows, norm: NW 8'),
    ('gemv', 'bf16', 16, 24, 264, 0, 1, 0, ('skinny', 16, [(16, 8, 4, 0, 0, 2, 16)]),
     'skinny_kernel SwiGLU 16 rows, NW 4'),
    ('gemv', 'bf16', 16, 24, 264, 1, 1, 0, ('skinny', 16, [(16, 8, 8, 0, 0, 2, 16)]),
     'skinny_kernel SwiGLU 16 rows, norm: NW 8'),
    ('gemv', 'bf16', 5, 8200, 256, 1, 0, 0, ('skinny', 16, [(5, 4, 4, 0, 0, 483, 17)]),
     'skinny_kernel norm with more than 32 columns per CU: NW 4'),
    ('gemv', 'bf16', 3, 50, 8, 0, 0, 0, ('skinny', 16, [(3, 2, 4, 0, 0, 4, 16)]),
     'skinny_kernel K = 8 (mapping and tail: no rounding)'),
    ('gemv', 'bf16', 3, 50, 1024, 0, 0, 0, ('skinny', 16, [(3, 2, 4, 0, 0, 4, 16)]),
     'skinny_kernel K = 256 NW exactly'),
    ('gemv', 'bf16', 3, 50, 2048, 1, 0, 0, ('skinny', 16, [(3, 2, 8, 0, 0, 4, 16)]),
     'skinny_kernel K = 256 NW exactly, NW 8'),
    ('gemv', 'bf16', 3, 50, 1288, 0, 0, 0, ('skinny', 16, [(3, 2, 4, 0, 0, 4, 16)]),
     'skinny_kernel 6 slices over 4 waves, a tail of 8'),
    ('gemv', 'bf16', 3, 50, 1288, 1, 0, 0, ('skinny', 16, [(3, 2, 8, 0, 0, 4, 16)]),
     'skinny_kernel 6 slices over 8 waves, a tail of 8'),
    ('gemv', 'bf16', 5, 50, 4104, 0, 0, 0, ('skinny', 16, [(5, 4, 4, 0, 0, 4, 16)]),
     'skinny_kernel K = 4104'),
    ('gemv', 'bf16', 3, 13, 264, 0, 0, 0, ('skinny', 16, [(3, 2, 4, 0, 0, 1, 16)]),
     'skinny_kernel N < 16: one partial tile, one block'),
    ('gemv', 'bf16', 3, 20000, 264, 0, 0, 0, ('skinny', 16, [(3, 2, 4, 0, 0, 500, 40)]),
     'skinny_kernel 3 tiles per block, the last partial'),
    ('gemv', 'bf16', 2, 33000, 256, 0, 0, 0, ('skinny', 16, [(2, 2, 4, 0, 0, 508, 65)]),
     'skinny_kernel 5 tiles per block: a second pass'),
    ('gemv', 'bf16', 2, 16400, 256, 0, 1, 0, ('skinny', 16, [(2, 2, 4, 0, 0, 497, 33)]),
     'skinny_kernel SwiGLU 3 tiles per block: a second pass'),
    ('gemv_w8', 'fp8', 2, 50, 264, 0, 0, 0, ('skinny', 16, [(2, 2, 4, 0, 0, 4, 16)]),
     'skinny_kernel 2 rows, NW 4'),
    ('gemv_w8', 'fp8', 2, 50, 264, 1, 0, 0, ('skinny', 16, [(2, 2, 8, 0, 0, 4, 16)]),
     'skinny_kernel 2 rows, norm: NW 8'),
    ('gemv_w8', 'fp8', 3, 50, 264, 0, 0, 0, ('skinny', 16, [(3, 2, 4, 0, 0, 4, 16)]),
     'skinny_kernel 3 rows, NW 4'),
    ('gemv_w8', 'fp8', 3, 50, 264, 1, 0, 0, ('skinny', 16, [(3, 2, 8, 0, 0, 4, 16)]),
     'skinny_kernel 3 rows, norm: NW 8'),
    ('gemv_w8', 'fp8', 4, 50, 264, 0, 0, 0, ('skinny', 16, [(4, 2, 4, 0, 0, 4, 16)]),
     'skinny_kernel 4 rows, NW 4'),
    ('gemv_w8', 'fp8', 4, 50, 264, 1, 0, 0, ('skinny', 16, [(4, 2, 8, 0, 0, 4, 16)]),
     'skinny_kernel 4 rows, norm: NW 8'),
    ('gemv_w8', 'fp8', 5, 50, 264, 0, 0, 0, ('skinny', 16, [(5, 4, 4, 0, 0, 4, 16)]),
     'skinny_kernel 5 rows, NW 4'),
    ('gemv_w8', 'fp8', 5, 50, 264, 1, 0, 0, ('skinny', 16, [(5, 4, 8, 0, 0, 4, 16)]),
     'skinny_kernel 5 rows, norm: NW 8'),
    ('gemv_w8', 'fp8', 8, 50, 264, 0, 0, 0, ('skinny', 16, [(8, 4, 4, 0, 0, 4, 16)]),
     'skinny_kernel 8 rows, NW 4'),
    ('gemv_w8', 'fp8', 8, 50, 264, 1, 0, 0, ('skinny', 16, [(8, 4, 8, 0, 0, 4, 16)]),
     'skinny_kernel 8 rows, norm: NW 8'),
    ('gemv_w8', 'fp8', 9, 50, 264, 0, 0, 0, ('skinny', 16, [(9, 8, 4, 0, 0, 4, 16)]),
     'skinny_kernel 9 rows, NW 4'),
    ('gemv_w8', 'fp8', 9, 50, 264, 1, 0, 0, ('skinny', 16, [(9, 8, 8, 0, 0, 4, 16)]),
     'skinny_kernel 9 rows, norm: NW 8'),
    ('gemv_w8', 'fp8', 16, 50, 264, 0, 0, 0, ('skinny', 16, [(16, 8, 4, 0, 0, 4, 16)]),
     'skinny_kernel 16 rows, NW 4'),
    ('gemv_w8', 'fp8', 16, 50, 264, 1, 0, 0, ('skinny', 16, [(16, 8, 8, 0, 0, 4, 16)]),
     'skinny_kernel 16 rows, norm: NW 8'),
    ('gemv_w8', 'fp8', 17, 50, 264, 0, 0, 0, ('skinny', 16, [(16, 8, 4, 0, 0, 4, 16), (1, 2, 4, 0, 0, 4, 16)]),
     'skinny_kernel 17 rows, NW 4'),
    ('gemv_w8', 'fp8', 17, 50, 264, 1, 0, 0, ('skinny', 16, [(16, 8, 8, 0, 0, 4, 16), (1, 2, 8, 0, 0, 4, 16)]),
     'skinny_kernel 17 rows, norm: NW 8'),
    ('gemv_w8', 'fp8', 33, 50, 264, 0, 0, 0, ('skinny', 16, [(16, 8, 4, 0, 0, 4, 16), (16, 8, 4, 0, 0, 4, 16), (1, 2, 4, 0, 0, 4, 16)]),
     'skinny_kernel 33 rows, NW 4'),
    ('gemv_w8', 'fp8', 33, 50, 264, 1, 0, 0, ('skinny', 16, [(16, 8, 8, 0, 0, 4, 16), (16, 8, 8, 0, 0, 4, 16), (1, 2, 8, 0, 0, 4, 16)]),
     'skinny_kernel 33 rows, norm: NW 8'),
    ('gemv_w8', 'fp8', 2, 24, 264, 0, 1, 0, ('skinny', 16, [(2, 2, 4, 0, 0, 2, 16)]),
     'skinny_kernel SwiGLU 2 rows, NW 4'),
    ('gemv_w8', 'fp8', 2, 24, 264, 1, 1, 0, ('skinny', 16, [(2, 2, 8, 0, 0, 2, 16)]),
     'skinny_kernel SwiGLU 2 rows, norm: NW 8'),
    ('gemv_w8', 'fp8', 5, 24, 264, 0, 1, 0, ('skinny', 16, [(5, 4, 4, 0, 0, 2, 16)]),
     'skinny_kernel SwiGLU 5 rows, NW 4'),
    ('gemv_w8', 'fp8', 5, 24, 264, 1, 1, 0, ('skinny', 16, [(5, 4, 8, 0, 0, 2, 16)]),
     'skinny_kernel SwiGLU 5 rows, norm: NW 8'),
    ('gemv_w8', 'fp8', 16, 24, 264, 0, 1, 0, ('skinny', 16, [(16, 8, 4, 0, 0, 2, 16)]),
     'skinny_kernel SwiGLU 16 rows, NW 4'),
    ('gemv_w8', 'fp8', 16, 24, 264, 1, 1, 0, ('skinny', 16, [(16, 8, 8, 0, 0, 2, 16)]),
     'skinny_kernel SwiGLU 16 rows, norm: NW 8'),
    ('gemv_w8', 'fp8', 5, 8200, 256, 1, 0, 0, ('skinny', 16, [(5, 4, 4, 0, 0, 483, 17)]),
     'skinny_kernel norm with more than 32 columns per CU: NW 4'),
    ('gemv_w8', 'fp8', 3, 50, 8, 0, 0, 0, ('skinny', 16, [(3, 2, 4, 0, 0, 4, 16)]),
     'skinny_kernel K = 8 (mapping and tail: no rounding)'),
    ('gemv_w8', 'fp8', 3, 50, 1024, 0, 0, 0, ('skinny', 16, [(3, 2, 4, 0, 0, 4, 16)]),
     'skinny_kernel K = 256 NW exactly'),
    ('gemv_w8', 'fp8', 3, 50, 2048, 1, 0, 0, ('skinny', 16, [(3, 2, 8, 0, 0, 4, 16)]),
     'skinny_kernel K = 256 NW exactly, NW 8'),
    ('gemv_w8', 'fp8', 3, 50, 1288, 0, 0, 0, ('skinny', 16, [(3, 2, 4, 0, 0, 4, 16)]),
     'skinny_kernel 6 slices over 4 waves, a tail of 8'),
    ('gemv_w8', 'fp8', 3, 50, 1288, 1, 0, 0, ('skinny', 16, [(3, 2, 8, 0, 0, 4, 16)]),
     'skinny_kernel 6 slices over 8 waves, a tail of 8'),
    ('gemv_w8', 'fp8', 5, 50, 4104, 0, 0, 0, ('skinny', 16, [(5, 4, 4, 0, 0, 4, 16)]),
     'skinny_kernel K = 4104'),
    ('gemv_w8', 'fp8', 3, 13, 264, 0, 0, 0, ('skinny', 16, [(3, 2, 4, 0, 0, 1, 16)]),
     'skinny_kernel N < 16: one partial tile, one block'),
    ('gemv_w8', 'fp8', 3, 20000, 264, 0, 0, 0, ('skinny', 16, [(3, 2, 4, 0, 0, 500, 40)]),
     'skinny_kernel 3 tiles per block, the last partial'),
    ('gemv_w8', 'fp8', 2, 33000, 256, 0, 0, 0, ('skinny', 16, [(2, 2, 4, 0, 0, 508, 65)]),
     'skinny_kernel 5 tiles per block: a second pass'),
    ('gemv_w8', 'fp8', 2, 16400, 256, 0, 1, 0, ('skinny', 16, [(2, 2, 4, 0, 0, 497, 33)]),
     'skinny_kernel SwiGLU 3 tiles per block: a second pass'),
    ('gemv', 'bf16', 3, 11800, 264, 0, 0, 0, ('skinny', 16, [(3, 2, 4, 0, 0, 492, 24)]),
     'skinny_kernel 2 tiles per block, the last partial'),
    ('gemv', 'bf16', 3, 28400, 264, 0, 0, 0, ('skinny', 16, [(3, 2, 4, 0, 0, 508, 56)]),
     'skinny_kernel 4 tiles per block, the last partial'),
    ('rowss', 'bf16', 5, 176, 288, 0, 0, 4, ('skinny', 16, [(5, 4, 4, 0, 1, 11, 16)]),
     'skinny_kernel packed 4'),
    ('rowss', 'bf16', 5, 176, 288, 1, 0, 4, ('skinny', 16, [(5, 4, 8, 0, 1, 11, 16)]),
     'skinny_kernel packed 4, norm'),
    ('rowss', 'bf16', 5, 96, 288, 0, 1, 4, ('skinny', 16, [(5, 4, 4, 0, 1, 6, 16)]),
     'skinny_kernel packed 4, SwiGLU'),
    ('rowss', 'bf16', 5, 176, 288, 0, 0, 8, ('skinny', 16, [(5, 4, 4, 0, 1, 11, 16)]),
     'skinny_kernel packed 8'),
    ('rowss', 'bf16', 5, 176, 288, 1, 0, 8, ('skinny', 16, [(5, 4, 8, 0, 1, 11, 16)]),
     'skinny_kernel packed 8, norm'),
    ('rowss', 'bf16', 5, 96, 288, 0, 1, 8, ('skinny', 16, [(5, 4, 4, 0, 1, 6, 16)]),
     'skinny_kernel packed 8, SwiGLU'),
    ('rowss', 'bf16', 5, 176, 288, 0, 0, 16, ('skinny', 16, [(5, 4, 4, 0, 1, 11, 16)]),
     'skinny_kernel packed 16'),
    ('rowss', 'bf16', 5, 176, 288, 1, 0, 16, ('skinny', 16, [(5, 4, 8, 0, 1, 11, 16)]),
     'skinny_kernel packed 16, norm'),
    ('rowss', 'bf16', 5, 96, 288, 0, 1, 16, ('skinny', 16, [(5, 4, 4, 0, 1, 6, 16)]),
     'skinny_kernel packed 16, SwiGLU'),
    ('rowss', 'bf16', 16, 96, 288, 1, 1, 16, ('skinny', 16, [(16, 8, 8, 0, 1, 6, 16)]),
     'skinny_kernel packed 16, 16 rows, norm, SwiGLU'),
    ('rowss', 'fp8', 5, 176, 320, 0, 0, 4, ('skinny', 16, [(5, 4, 4, 0, 1, 11, 16)]),
     'skinny_kernel packed 4'),
    ('rowss', 'fp8', 5, 176, 320, 1, 0, 4, ('skinny', 16, [(5, 4, 8, 0, 1, 11, 16)]),
     'skinny_kernel packed 4, norm'),
    ('rowss', 'fp8', 5, 96, 320, 0, 1, 4, ('skinny', 16, [(5, 4, 4, 0, 1, 6, 16)]),
     'skinny_kernel packed 4, SwiGLU'),
    ('rowss', 'fp8', 5, 176, 320, 0, 0, 8, ('skinny', 16, [(5, 4, 4, 0, 1, 11, 16)]),
     'skinny_kernel packed 8'),
    ('rowss', 'fp8', 5, 176, 320, 1, 0, 8, ('skinny', 16, [(5, 4, 8, 0, 1, 11, 16)]),
     'skinny_kernel packed 8, norm'),
    ('rowss', 'fp8', 5, 96, 320, 0, 1, 8, ('skinny', 16, [(5, 4, 4, 0, 1, 6, 16)]),
     'skinny_kernel packed 8, SwiGLU'),
    ('rowss', 'fp8', 5, 176, 320, 0, 0, 16, ('skinny', 16, [(5, 4, 4, 0, 1, 11, 16)]),
     'skinny_kernel packed 16'),
    ('rowss', 'fp8', 5, 176, 320, 1, 0, 16, ('skinny', 16, [(5, 4, 8, 0, 1, 11, 16)]),
     'skinny_kernel packed 16, norm'),
    ('rowss', 'fp8', 5, 96, 320, 0, 1, 16, ('skinny', 16, [(5, 4, 4, 0, 1, 6, 16)]),
     'skinny_kernel packed 16, SwiGLU'),
    ('rowss', 'fp8', 16, 96, 320, 1, 1, 16, ('skinny', 16, [(16, 8, 8, 0, 1, 6, 16)]),
     'skinny_kernel packed 16, 16 rows, norm, SwiGLU'),
]


@pytest.mark.parametrize("entry,wt,B,N,K,norm,swiglu,packed,route,what", CASES,
                         ids=["%s-%s-%dx%dx%d%s%s%s" % (c[0], c[1], c[2], c[3], c[4], "-norm" * c[5], "-swiglu" * c[6], "-pk%d" % c[7] if c[7] else "")
                              for c in CASES])
def test_decode_product_exact(route_cli, entry, wt, B, N, K, norm, swiglu, packed, route, what):
    _product_case(route_cli, entry, wt, B, N, K, norm, swiglu, packed, route)


# ------------------------------------------------------------------------------------------------ the statistics hand-off
def _guarded_table(B):
    buf, view = guarded(B, ROWSS_STRIDE, ROWSS_STRIDE, F32, row0=1)
    return buf, view


def _check_table_guard(buf, view, what):
    view.fill_(torch.tensor([SENTINEL[F32][1]], dtype=torch.int32).view(F32).item())
    assert bool((buf.view(torch.int32) == SENTINEL[F32][1]).all()), what + ": written outside the table"


def _slot_sums(h64, passes):
    """the table a producer with these weight passes publishes for the output rows h64 [B, N]: (float64 [B, 512], grid per row)"""
    want = torch.zeros((h64.shape[0], ROWSS_STRIDE), dtype=torch.float64)
    grids, b0 = [], 0
    for p in passes:
        for j in range(p["grid"]):
            want[b0:b0 + p["rows"], j] = h64[b0:b0 + p["rows"], j * p["cw"]:(j + 1) * p["cw"]].pow(2).sum(1)
        grids += [p["grid"]] * p["rows"]
        b0 += p["rows"]
    assert b0 == h64.shape[0]
    return want, grids


PRODUCER_CASES = [
    # weights, B, N, K, the route at 256 CUs
    ('bf16', 5, 1000, 264, ('skinny', 16, [(5, 4, 4, 0, 0, 63, 16)])),
    ('fp8', 8, 1000, 264, ('skinny', 16, [(8, 4, 4, 0, 0, 63, 16)])),
    ('bf16', 17, 1000, 264, ('skinny', 16, [(16, 8, 4, 0, 0, 63, 16), (1, 2, 4, 0, 0, 63, 16)])),
    ('fp8', 33, 600, 264, ('skinny', 16, [(16, 8, 4, 0, 0, 38, 16), (16, 8, 4, 0, 0, 38, 16), (1, 2, 4, 0, 0, 38, 16)])),
    ('bf16', 3, 20000, 64, ('skinny', 16, [(3, 2, 4, 0, 0, 500, 40)])),
    ('fp8', 2, 50, 8, ('skinny', 16, [(2, 2, 4, 0, 0, 4, 16)])),
]


@pytest.mark.parametrize("wt,B,N,K,route", PRODUCER_CASES, ids=["%s-%dx%dx%d" % c[:4] for c in PRODUCER_CASES])
def test_rowss_producer_table_slot_by_slot(route_cli, wt, B, N, K, route):
    """dense integer data through the publishing product: `out` is the reference bit for bit, slot j of row b is the sum of squares
    of the columns [j cw, (j + 1) cw) of that row's reference (the tolerance test_gemv_rowss_handoff gives the row sum), every slot
    from `grid` on is exactly 0, and nothing around out or the table is written"""
    ops, _ = _ops()
    what = "rowss producer %s B=%d N=%d K=%d" % (wt, B, N, K)
    fp8 = wt == "fp8"
    r = _assert_route(route_cli, wt, B, N, K, 0, 0, 0, 0, route)
    assert r["rowss_supported"] == 1
    seed = 77 * B + N + K
    x64, w_i, res_i = ints((B, K), 7, seed), ints((N, K), 8, seed + 1), ints((B, N), 256, seed + 2)
    acc = x64 @ w_i.T
    e, wkw = _weights(w_i, torch.ones(N, dtype=torch.float64), fp8)
    tally = {}
    ref = _plain_refs(_scaled(acc, e), res_i.float(), acc, e, BF16, tally)["res"]
    if K != 8:
        _assert_tally(what, tally)
    want, grids = _slot_sums(ref.double(), r["passes"])
    x_d, res_d, wkw = poisoned(x64.to(BF16)), poisoned(res_i.to(BF16)), _dev_weights(wkw, 0, N)
    first = None
    for run in range(2):
        tbuf, table = _guarded_table(B)
        call = _entry_call("rowss", x_d, wkw, None, 0.0, res_d, False, False, publish=True, table=table)
        obuf, out = guarded(B, N, N, BF16, row0=1)
        got_out, got_table = call(out)
        assert got_table.data_ptr() == table.data_ptr()
        bits = check_guarded(obuf, out, ref.to(BF16).to(DEV), what).view(torch.int16)
        t = table.cpu()
        for b in range(B):
            assert bool((t[b, grids[b]:] == 0).all()), "%s: row %d, slots past the grid (%d)" % (what, b, grids[b])
        bad = (t.double() - want).abs() > SLOT_RTOL * want
        if bool(bad.any()):
            b, j = (int(i) for i in bad.nonzero()[0])
            pytest.fail("%s: %d slots differ, the first at (row, slot) = (%d, %d): %r, expected %r" % (what, int(bad.sum()), b, j, float(t[b, j]),
                                                                                                       float(want[b, j])))
        _check_table_guard(tbuf, table, what)
        if first is not None:
            assert torch.equal(first[0], bits) and torch.equal(first[1].view(torch.int32), t.view(torch.int32)), what + ": run-to-run difference"
        first = (bits, t)


CHAIN_CASES = [
    # weights, B, consumer N2 (its SwiGLU form: N2 / 2 outputs), packed granule of the consumer, the routes at 256 CUs of the producer
    # and of the consumer reading the table: plain / out_f32, SwiGLU
    ('bf16', 3, 192, 0, ('skinny', 16, [(3, 2, 4, 0, 0, 32, 16)]),
     ('skinny', 16, [(3, 2, 8, 1, 0, 12, 16)]),
     ('skinny', 16, [(3, 2, 8, 1, 0, 6, 16)])),
    ('fp8', 3, 192, 4, ('skinny', 16, [(3, 2, 4, 0, 0, 32, 16)]),
     ('skinny', 16, [(3, 2, 8, 1, 1, 12, 16)]),
     ('skinny', 16, [(3, 2, 8, 1, 1, 6, 16)])),
    ('bf16', 5, 192, 8, ('skinny', 16, [(5, 4, 4, 0, 0, 32, 16)]),
     ('skinny', 16, [(5, 4, 8, 1, 1, 12, 16)]),
     ('skinny', 16, [(5, 4, 8, 1, 1, 6, 16)])),
    ('fp8', 8, 192, 0, ('skinny', 16, [(8, 4, 4, 0, 0, 32, 16)]),
     ('skinny', 16, [(8, 4, 8, 1, 0, 12, 16)]),
     ('skinny', 16, [(8, 4, 8, 1, 0, 6, 16)])),
    ('bf16', 16, 192, 16, ('skinny', 16, [(16, 8, 4, 0, 0, 32, 16)]),
     ('skinny', 16, [(16, 8, 8, 1, 1, 12, 16)]),
     ('skinny', 16, [(16, 8, 8, 1, 1, 6, 16)])),
    ('fp8', 16, 192, 8, ('skinny', 16, [(16, 8, 4, 0, 0, 32, 16)]),
     ('skinny', 16, [(16, 8, 8, 1, 1, 12, 16)]),
     ('skinny', 16, [(16, 8, 8, 1, 1, 6, 16)])),
    ('bf16', 17, 192, 4, ('skinny', 16, [(16, 8, 4, 0, 0, 32, 16), (1, 2, 4, 0, 0, 32, 16)]),
     ('skinny', 16, [(16, 8, 8, 1, 1, 12, 16), (1, 2, 8, 1, 1, 12, 16)]),
     ('skinny', 16, [(16, 8, 8, 1, 1, 6, 16), (1, 2, 8, 1, 1, 6, 16)])),
    ('fp8', 17, 192, 16, ('skinny', 16, [(16, 8, 4, 0, 0, 32, 16), (1, 2, 4, 0, 0, 32, 16)]),
     ('skinny', 16, [(16, 8, 8, 1, 1, 12, 16), (1, 2, 8, 1, 1, 12, 16)]),
     ('skinny', 16, [(16, 8, 8, 1, 1, 6, 16), (1, 2, 8, 1, 1, 6, 16)])),
    ('bf16', 33, 192, 0, ('skinny', 16, [(16, 8, 4, 0, 0, 32, 16), (16, 8, 4, 0, 0, 32, 16), (1, 2, 4, 0, 0, 32, 16)]),
     ('skinny', 16, [(16, 8, 8, 1, 0, 12, 16), (16, 8, 8, 1, 0, 12, 16), (1, 2, 8, 1, 0, 12, 16)]),
     ('skinny', 16, [(16, 8, 8, 1, 0, 6, 16), (16, 8, 8, 1, 0, 6, 16), (1, 2, 8, 1, 0, 6, 16)])),
    ('fp8', 33, 192, 4, ('skinny', 16, [(16, 8, 4, 0, 0, 32, 16), (16, 8, 4, 0, 0, 32, 16), (1, 2, 4, 0, 0, 32, 16)]),
     ('skinny', 16, [(16, 8, 8, 1, 1, 12, 16), (16, 8, 8, 1, 1, 12, 16), (1, 2, 8, 1, 1, 12, 16)]),
     ('skinny', 16, [(16, 8, 8, 1, 1, 6, 16), (16, 8, 8, 1, 1, 6, 16), (1, 2, 8, 1, 1, 6, 16)])),
    ('bf16', 5, 8224, 0, ('skinny', 16, [(5, 4, 4, 0, 0, 32, 16)]),
     ('skinny', 16, [(5, 4, 4, 1, 0, 484, 17)]),
     ('skinny', 16, [(5, 4, 8, 1, 0, 242, 17)])),
    ('fp8', 5, 8224, 16, ('skinny', 16, [(5, 4, 4, 0, 0, 32, 16)]),
     ('skinny', 16, [(5, 4, 4, 1, 1, 257, 32)]),
     ('skinny', 16, [(5, 4, 8, 1, 1, 129, 32)])),
]
CHAIN_N1, CHAIN_K = 512, 64


@pytest.mark.parametrize("wt,B,N2,packed,route_p,route_c,route_s", CHAIN_CASES, ids=["%s-B%d-N%d-pk%d" % c[:4] for c in CHAIN_CASES])
def test_rowss_chain_exact_statistics(route_cli, wt, B, N2, packed, route_p, route_c, route_s):
    """producer -> consumer with exact statistics.  The producer's W has four entries of [-2, 2] per row at K = 64 (|acc| <= 56: no
    rounding) and its residual is h - acc for scaled octet rows h (bf16-exact, asserted), so out == h and every table slot is an exact
    integer multiple of 1 / 4: compared with torch.equal.  The consumer (RMSNorm, then plain, out_f32 and SwiGLU) must return the
    ONE reference from all three sources of the statistics: the published table, its own reduction, and plain srgpt_gemv /
    srgpt_gemv_w8 (row-major weights) -- equality where test_gemv_rowss_handoff allows one bf16 ulp.  17 and 33 rows: every weight
    pass publishes and reads its own rows of the table."""
    ops, _ = _ops()
    what = "rowss chain %s B=%d N2=%d packed=%d" % (wt, B, N2, packed)
    fp8, N1, K, eps = wt == "fp8", CHAIN_N1, CHAIN_K, 1e-6
    rp = _assert_route(route_cli, wt, B, N1, K, 0, 0, 0, 0, route_p)
    _assert_route(route_cli, wt, B, N2, N1, 1, 0, 1, packed, route_c)
    _assert_route(route_cli, wt, B, N2 // 2, N1, 1, 1, 1, packed, route_s)
    seed = 31 * B + N2 + packed
    g = torch.Generator().manual_seed(seed)
    h, rms = _octet_rows(B, N1, seed + 1)
    x64 = ints((B, K), 7, seed + 2)
    w1 = torch.zeros((N1, K), dtype=torch.float64)
    cols = torch.rand((N1, K), generator=g).argsort(1)[:, :4]
    w1.scatter_(1, cols, torch.randint(-2, 3, (N1, 4), generator=g).double())
    acc1 = x64 @ w1.T
    assert float(acc1.abs().max()) <= 56
    res1 = h - acc1
    assert torch.equal(res1.to(BF16).double(), res1) and torch.equal(h.to(BF16).double(), h), what
    # the producer: fp8 scales stay powers of two here (acc must come back unrounded)
    if fp8:
        w8, wscale, deq = ops.quantize_fp8_rows(w1.to(BF16))
        assert torch.equal(deq.double(), w1)
        kw1 = dict(w8=w8, wscale=wscale)
    else:
        kw1 = dict(w=w1.to(BF16))
    want, grids = _slot_sums(h, rp["passes"])
    assert torch.equal(want * 4, (want * 4).round()) and float(want.sum(1).max()) * 4 < 2 ** 24  # exact in fp32 in any order
    x_d, res_d, kw1 = poisoned(x64.to(BF16)), poisoned(res1.to(BF16)), _dev_weights(kw1, 0, N1)
    tbuf, table = _guarded_table(B)
    obuf, hbuf = guarded(B, N1, N1, BF16, row0=1)
    h_d = poisoned(h.to(BF16))
    _entry_call("rowss", x_d, kw1, None, 0.0, res_d, False, False, publish=True, table=table)(hbuf)
    assert torch.equal(table.cpu().double(), want), what + ": the published table"
    check_guarded(obuf, hbuf, h_d, what + ": the producer's rows")
    table_d = table.clone()
    _check_table_guard(tbuf, table, what)
    # the consumer
    nw64 = ints((N1,), 4, seed + 3)
    xe = _normed(h, rms, nw64, eps, what)
    w2 = ints((N2, N1), 8, seed + 4)
    acc2 = xe @ w2.T
    pow2 = torch.ones(N2, dtype=torch.float64)
    pow2[:N2 // 2] = _gate_pow2(acc2[:, :N2 // 2], fp8)
    e, kw2 = _weights(w2, pow2, fp8)
    prod = _scaled(acc2, e)
    tally = {}
    ref = _plain_refs(prod, None, acc2, e, BF16, tally)["plain"]
    sref, salt = _swiglu_refs(prod[:, :N2 // 2], prod[:, N2 // 2:], what, tally)
    _assert_tally(what, tally)
    norm_w = poisoned(nw64.to(BF16))
    kw2_rm = _dev_weights(kw2, 0, N2)
    kw2_pk = _dev_weights(kw2, packed, N2) if packed else kw2_rm
    sources = [("published table", "rowss", kw2_pk, dict(rowss_in=table_d)), ("own statistics", "rowss", kw2_pk, {}),
               ("plain entry", "gemv_w8" if fp8 else "gemv", kw2_rm, {})]
    for src, entry, kw, extra in sources:
        for form, swiglu, out_f32, n, r, a in (("plain", False, False, N2, ref, None), ("out_f32", False, True, N2, ref, None),
                                               ("swiglu", True, False, N2 // 2, sref, salt)):
            odt = F32 if out_f32 else BF16
            call = _entry_call(entry, h_d, kw, norm_w, eps, None, swiglu, out_f32, **extra)
            _run_twice(call, B, n, odt, r.to(BF16).to(odt).to(DEV), None if a is None else a.to(BF16).to(DEV), "%s, %s, %s" % (what, src, form))
