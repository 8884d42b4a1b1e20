"""Data for which region pooling (csrc/region.hip) and the vision tower's row kernels (csrc/norm.hip; avgpool, s2d, im2col and
vit_assemble_cls of region.hip) have ONE possible output, and their float64 references.  No GPU here: tests/test_host_region_exact.py
asserts every precondition stated below for every case and shows that the data tells wrong kernels from the right one;
tests/test_gpu_vision_exact.py runs the kernels on it.

Region pooling.  Features are integers in [-8, 8].  A processor-size mask holds integers 0 .. 3 whose sum is exactly 2^k (filled at
random, then single entries moved until the sum is met); its side is fw, 2 fw or fw / 2, so the wrapper passes rscale = 1, 2 or 0.5
exactly and the bilinear taps weigh {0, 1}, {1/2, 1/2} or {1/4, 3/4} per axis.  The resampled values v are then multiples of 1/16 up
to 3 -- exact in bf16 -- and their sum is S = 2^k (fw / side)^2, because every source pixel's total influence is 1, 1/4 or 4 at these
ratios (the clamped borders included); k is chosen so that S is a power of two <= 2^14.  Then den = rnd(rnd(S) + 1e-8) = S, the
normalised weights v / den are exact in bf16 under any division that is exact on exact quotients, every product weight * feature
is a multiple of 2^-4 / S, and because the weight numerators of a mask add up to 16 S units and |feature| <= 8 no sum of any subset
exceeds 128 S <= 2^21 units: every fp32 partial sum in every order, every slab split and every MFMA accumulation is exact.  A correct
kernel returns the float64 W @ F, rounded ONCE to bf16 for bf16 features, that number itself for fp32 features.  v comes from
torch.nn.functional.interpolate(..., mode="bilinear") on the CPU, which is what the oracle's mask_pooling calls.  One mask of every
case is all zeros: its row is exactly 0.0 (0 / 1e-8 = 0), never NaN; a case of ONE mask has a second mask set that is that zero mask.

The cases are the smallest at which each code path of region.hip exists; the thresholds are restated here (RP_*, MFMA_*) and
Case.geometry() derives, from fw alone, which side of each a case lies on.

LayerNorm.  Rows are m + s * v with v a shuffle of the octets of tests/test_gpu_gemv_exact.py (square sum 128 each) in which every
octet comes together with its negation -- and, where cols / 8 is odd, one octet signed so that it sums to zero: (7, -7, 4, -3, -2, 1,
0, 0) or (6, -6, 5, -5, 2, -1, -1, 0) -- so the mean is exactly m and the variance exactly 16 s^2; s in {1/2, 1, 2}, m in {0, +-4,
+-8}, gains multiples of 1/2 with |g| <= 2, biases ODD multiples of 1/16 (an exactly cancelling p * g + b would keep the error of
rsqrtf; p * g is a multiple of 1/8 and an odd sixteenth cannot cancel it).  (x - mean) * rstd * g + b is then v / 4 * g + b, an odd
multiple of 1/16 below 12: a bf16 value.  The rows with m != 0 rely on sum / cols being an IEEE division: the library is built
without any fast-math flag."""
import math

import torch
import torch.nn.functional as F

from tests.test_gpu_gemv_exact import OCTETS
from tests.util import BF16, F32, ints

# ---- restated from csrc/region.hip
RP_POS = 1024        # positions per block of the resample launch = per mask-sum slab
RP_ROWS = 300        # feature rows per block of the VALU pooling kernel
RP_FB = 16           # partials its last arriver keeps in flight
RP_CW_F32 = 32       # fp32 channels per block of the VALU kernel
RP_MAXM = 16         # masks per launch
MFMA_FB = 24         # partials the MFMA kernel's last arriver keeps in flight
MFMA_PSUM = 16       # mask-sum slabs the MFMA kernel takes per batch
MFMA_CW = 64         # channels per block of the MFMA kernel
VALU_PSUM = 32       # mask-sum slabs the VALU kernel takes per batch
S_MAX = 2 ** 14


def mfma_chunks(L):  # region_mfma_chunks
    return 4 if L >= 8192 else (2 if L >= 2048 else 1)


class Case:
    def __init__(self, dtype, fw, C, M, sides, what, want):
        self.dtype, self.fw, self.C, self.M, self.sides, self.what, self.want = dtype, fw, C, M, tuple(sides), what, want
        self.L = fw * fw
        self.id = "%s-fw%d-C%d-M%d" % ("bf16" if dtype == BF16 else "f32", fw, C, M)
        self.seed = 7 * fw + 1000 * M + C

    def geometry(self):
        """from fw (and the dtype, which selects the kernel) alone: the kernel's row slabs, what its last slab holds, the mask-sum
        slabs and the rounds of each loop that has a threshold"""
        L = self.L
        n_psum = -(-L // RP_POS)
        if self.dtype == BF16:
            ch = mfma_chunks(L)
            rows = 128 * ch
            return dict(kernel="mfma", ch=ch, rows=rows, full=L // rows, tail=L % rows, nslab=-(-L // rows), n_psum=n_psum,
                        psum_batches=-(-n_psum // MFMA_PSUM), fb_rounds=-(-(-(-L // rows)) // MFMA_FB))
        nslab = -(-L // RP_ROWS)
        return dict(kernel="valu", mm=8 if self.M <= 8 else 16, rows=RP_ROWS, full=L // RP_ROWS,
                    tail=L % RP_ROWS, nslab=nslab, n_psum=n_psum, psum_batches=-(-n_psum // VALU_PSUM), fb_rounds=-(-nslab // RP_FB))

    def slab_rows(self):
        return self.geometry()["rows"]


# dtype, fw, C, M, mask sides, the path the case exists for, what geometry() must say
CASES = [
    Case(BF16, 16, 8, 1, (16,), "CH = 1, two full row slabs, one channel chunk (all lanes clamped to chunk 0)",
         dict(ch=1, full=2, tail=0, psum_batches=1, fb_rounds=1)),
    Case(BF16, 27, 72, 7, (27, 54), "CH = 1, 5 slabs + a tail of 89 rows; second channel slab 7/8 clamped",
         dict(ch=1, full=5, tail=89, psum_batches=1, fb_rounds=1)),
    Case(BF16, 46, 200, 16, (46, 92, 23), "CH = 2, 8 slabs + 68 rows", dict(ch=2, full=8, tail=68, psum_batches=1, fb_rounds=1)),
    Case(BF16, 80, 64, 9, (80,), "CH = 2, 25 row slabs: more than FB = 24, the last arriver's second round",
         dict(ch=2, full=25, tail=0, psum_batches=1, fb_rounds=2)),
    Case(BF16, 92, 136, 8, (92, 46), "CH = 4, 16 slabs + 272 rows", dict(ch=4, full=16, tail=272, psum_batches=1, fb_rounds=1)),
    Case(BF16, 130, 72, 17, (260, 65), "17 mask-sum slabs (the i0 = 16 loop) and 34 row slabs; M = 17 goes through the wrapper as 16 + 1",
         dict(ch=4, full=33, tail=4, nslab=34, n_psum=17, psum_batches=2, fb_rounds=2)),
    Case(F32, 16, 4, 1, (16,), "one partial row slab, one 4-channel chunk", dict(mm=8, full=0, tail=256, psum_batches=1, fb_rounds=1)),
    Case(F32, 27, 36, 8, (27, 54), "2 slabs + 129 rows; C = 32 + 4; MM = 8", dict(mm=8, full=2, tail=129, psum_batches=1, fb_rounds=1)),
    Case(F32, 27, 36, 9, (27, 54), "2 slabs + 129 rows; C = 32 + 4; MM = 16", dict(mm=16, full=2, tail=129, psum_batches=1, fb_rounds=1)),
    Case(F32, 46, 36, 5, (46, 92, 23), "every mask type at a second size: 7 slabs + 16 rows, three mask-sum slabs",
         dict(mm=8, full=7, tail=16, n_psum=3, psum_batches=1, fb_rounds=1)),
    Case(F32, 70, 32, 16, (70, 35), "17 row slabs: more than RP_FB = 16", dict(mm=16, full=16, tail=100, nslab=17, psum_batches=1, fb_rounds=2)),
    Case(F32, 182, 4, 2, (182, 91), "33 mask-sum slabs: the second 32-batch of the prologue",
         dict(mm=8, n_psum=33, psum_batches=2, nslab=111)),
]
CASE_IDS = [c.id for c in CASES]
MASK_TYPES = ("bf16", "f32", "u8")


# ------------------------------------------------------------------------------------------------ region pooling: the data
def features(case):
    """[L, C] float64 integers in [-8, 8]"""
    return ints((case.L, case.C), 8, case.seed)


def mask_k(fw, side):
    """the largest k with 2^k <= 1.5 side^2 (the mean of a random 0 .. 3 fill) and S = 2^k (fw / side)^2 <= 2^14"""
    k = int(math.floor(math.log2(1.5 * side * side)))
    while 2 ** k * fw * fw > S_MAX * side * side:
        k -= 1
    return k


def _mask(side, total, g):
    P = torch.randint(0, 4, (side * side,), generator=g)
    d = total - int(P.sum())
    while d != 0:  # move single entries until the sum is met
        sign = 1 if d > 0 else -1
        cand = (P < 3 if d > 0 else P > 0).nonzero()[:, 0]
        n = min(abs(d), cand.numel())
        P[cand[torch.randperm(cand.numel(), generator=g)[:n]]] += sign
        d -= sign * n
    return P.reshape(side, side)


def mask_sets(case, side):
    """-> [(masks [M, side, side] float64 with integer entries 0 .. 3, the index of the all-zero mask)]; M = 1: the second set is the
    zero mask"""
    g = torch.Generator().manual_seed(case.seed * 31 + side)
    total = 2 ** mask_k(case.fw, side)
    P = torch.stack([_mask(side, total, g) for _ in range(case.M)]).double()
    if case.M == 1:
        return [(P, None), (torch.zeros_like(P), 0)]
    zero = case.M // 2
    P[zero] = 0
    return [(P, zero)]


def resampled(P, fw):
    """the processor-size masks on the feature grid, as the oracle's mask_pooling resamples them -> [M, fw * fw] float64"""
    side = P.shape[-1]
    sf = (fw * fw / (side * side)) ** 0.5
    v = F.interpolate(P.float()[None], scale_factor=sf, mode="bilinear")[0]
    assert v.shape[-2:] == (fw, fw), (v.shape, fw)
    return v.double().flatten(1)


def weights(v, dtype):
    """-> (W = v / den [M, L] float64, den [M]) with the kernel's denominator: rnd(rnd(sum) + 1e-8) in the feature dtype"""
    s = v.sum(1)
    den = (s.to(dtype).float() + torch.tensor(1e-8, dtype=F32)).to(dtype).double()
    return v / den[:, None], den


def pooled(W, feat, dtype):
    """float64 W @ F, rounded once to the feature dtype -> fp32-valued tensor of that dtype"""
    return (W @ feat).float().to(dtype)


def reference(case, P, feat=None):
    feat = features(case) if feat is None else feat
    W = weights(resampled(P, case.fw), case.dtype)[0]
    out = pooled(W, feat, case.dtype)
    assert case.dtype != F32 or torch.equal(out.double(), W @ feat)  # fp32 features: no rounding at all
    return out


def raw_u8(P):
    """the raw uint8 mask of twice the side whose cv2-nearest resize is P: raw[2y, 2x] = P[y, x], 255 wherever the tables do not point"""
    M, side, _ = P.shape
    raw = torch.full((M, 2 * side, 2 * side), 255, dtype=torch.uint8)
    raw[:, ::2, ::2] = P.to(torch.uint8)
    return raw


def own_tables(side, seed):
    """nearest-neighbour tables of the test's own into raw_u8's mask: rows reversed, columns permuted -> (ys, xs int32, the
    processor-size mask they make of P as a function)"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.arange(side - 1, -1, -1)
    cols = torch.randperm(side, generator=g)
    return (2 * rows).to(torch.int32), (2 * cols).to(torch.int32), lambda P: P[:, rows][:, :, cols]


# ------------------------------------------------------------------------------------------------ region pooling: wrong kernels
def _pair_perm(L, chunk, partner):
    """the permutation of 0 .. L - 1 that swaps p with partner(p) inside every whole `chunk`"""
    idx = torch.arange(L)
    whole = (L // chunk) * chunk
    idx[:whole] = partner(idx[:whole])
    return idx


def mutants(case, P, feat):
    """{name: the output of a kernel that makes this mistake (in the feature dtype), or None where the case has nothing to show it}"""
    dtype, fw, L = case.dtype, case.fw, case.L
    v = resampled(P, fw)
    W, den = weights(v, dtype)
    rows = case.slab_rows()
    last0 = ((L - 1) // rows) * rows  # the last slab, partial where L is no multiple
    out = {}
    out["positions p, p + 1 of a chunk swapped"] = pooled(W[:, _pair_perm(L, 32, lambda p: p ^ 1)], feat, dtype)
    out["positions p, p + 4 swapped (a transposing read's block)"] = pooled(W[:, _pair_perm(L, 32, lambda p: p ^ 4)], feat, dtype)
    Wd = W.clone()
    Wd[:, last0:] = 0
    out["last row slab dropped"] = pooled(Wd, feat, dtype)
    Wt = W.clone()
    Wt[:, last0:] *= 2
    out["last row slab counted twice"] = pooled(Wt, feat, dtype)
    if case.C >= 16:
        c = torch.arange(case.C)
        whole = (case.C // 16) * 16
        c[:whole] = c[:whole] ^ 8
        out["channels c, c + 8 swapped"] = pooled(W, feat[:, c], dtype)
    else:
        out["channels c, c + 8 swapped"] = None
    out["masks m, m + 1 exchanged"] = pooled(W.roll(-1, 0), feat, dtype) if case.M > 1 else None  # every row takes its neighbour's
    Ws = torch.zeros_like(W)
    Ws[:, 1:] = W[:, :-1]
    out["weight of position p applied to p + 1"] = pooled(Ws, feat, dtype)
    side = P.shape[-1]
    Pt = P[:, :, torch.clamp(torch.arange(side) + 1, max=side - 1)]
    out["a bilinear tap off by one source pixel"] = pooled(weights(resampled(Pt, fw), dtype)[0], feat, dtype)
    s32 = v.sum(1).float()
    den_alt = (s32 + torch.tensor(1e-8, dtype=F32)).double()
    nz = den > 1e-6
    out["den not rounded to the feature dtype"] = None if torch.equal(den_alt[nz], den[nz]) else pooled(v / den_alt[:, None], feat, dtype)
    return out


def box_masks(M, S, seed=30):
    """the rectangular 0 / 1 masks of tests/test_gpu_kernels.py::test_region_pool_true_shape_vs_oracle"""
    g = torch.Generator().manual_seed(seed)
    masks = torch.zeros((M, S, S))
    for m in range(M):
        y0, x0 = int(torch.randint(0, S // 2, (1,), generator=g)), int(torch.randint(0, S // 2, (1,), generator=g))
        h, w = int(torch.randint(S // 8, S // 2, (1,), generator=g)), int(torch.randint(S // 8, S // 2, (1,), generator=g))
        masks[m, y0:y0 + h, x0:x0 + w] = 1
    return masks.double()


# ------------------------------------------------------------------------------------------------ LayerNorm
ZERO_SUM_SIGNS = torch.tensor([[1, -1, 1, -1, -1, 1, 1, 1], [1, -1, 1, -1, 1, -1, -1, 1]], dtype=torch.float64)
LN_S, LN_M = (0.5, 1.0, 2.0), (0.0, 4.0, -4.0, 8.0, -8.0)
LN_COLS = (8, 64, 1152, 2056, 4608)
LN_ROWS = (1, 5)


def ln_rows(rows, cols, seed):
    """-> (x [rows, cols], v, m [rows], s [rows]) float64 with x = m + s v: module docstring"""
    assert cols % 8 == 0
    g = torch.Generator().manual_seed(seed)
    xs, vs = [], []
    for r in range(rows):
        o = OCTETS[torch.randint(0, 2, (cols // 16,), generator=g)]
        parts = [o.reshape(-1), -o.reshape(-1)]
        if cols % 16:
            which = int(torch.randint(0, 2, (1,), generator=g))
            parts.append(OCTETS[which] * ZERO_SUM_SIGNS[which])
        v = torch.cat(parts)[torch.randperm(cols, generator=g)]
        vs.append(v)
        xs.append(LN_M[(r + seed) % 5] + LN_S[(r + seed) % 3] * v)
    m = torch.tensor([LN_M[(r + seed) % 5] for r in range(rows)], dtype=torch.float64)
    s = torch.tensor([LN_S[(r + seed) % 3] for r in range(rows)], dtype=torch.float64)
    return torch.stack(xs), torch.stack(vs), m, s


def ln_params(cols, seed, bias_bound=8):
    """gains: multiples of 1/2, |g| <= 2; biases: odd multiples of 1/16, |b| < bias_bound"""
    g = ints((cols,), 4, seed + 1) / 2
    gen = torch.Generator().manual_seed(seed + 2)
    b = (2 * torch.randint(-8 * bias_bound, 8 * bias_bound, (cols,), generator=gen) + 1).double() / 16
    return g, b


def ln_expected(v, g, b):
    """(x - mean) / sqrt(var) * g + b for the rows of ln_rows: v / 4 * g + b"""
    return v / 4 * g + b


def gelu64(y):
    return 0.5 * y * (1 + torch.erf(y * (0.5 ** 0.5)))


def bf16_ulp(x):
    """the spacing of bf16 at |x| (normal numbers)"""
    return torch.exp2(torch.floor(torch.log2(x.abs().double())) - 7)


GELU_BIAS_BOUND = 2
GELU_SLACK = 2.0 ** -20  # times |y|: erff's absolute error of a few fp32 ulps of 1 in front of the factor 0.5 y, ~16 times over
EXCLUDED_CAP = 0.03


def gelu_limit(y, ref):
    """the bound of the LayerNorm + GELU(erf) comparison: one bf16 ulp of the reference plus |y| 2^-20"""
    return bf16_ulp(ref) + y.abs() * GELU_SLACK


# ------------------------------------------------------------------------------------------------ avgpool and the data movers
AVGPOOL_SHAPES = ((108, 27), (96, 27), (27, 27), (24, 7))  # uniform 4 x 4; adaptive windows of 4 and 5 that overlap; identity; 24 -> 7


def avgpool_windows(in_w, out_w):
    return [((o * in_w) // out_w, -(-((o + 1) * in_w) // out_w)) for o in range(out_w)]


def avgpool_reference(x64, n_img, in_w, out_w, dtype):
    """x64 [n, in_w * in_w, C] integers -> rnd(fl32(s * fl32(1 / n))) [n, out_w * out_w, C]: the window sum is exact and every further
    step ONE IEEE operation"""
    C = x64.shape[-1]
    x = x64.reshape(n_img, in_w, in_w, C)
    win = avgpool_windows(in_w, out_w)
    out = torch.empty((n_img, out_w, out_w, C), dtype=F32)
    for oy, (y0, y1) in enumerate(win):
        for ox, (x0, x1) in enumerate(win):
            s = x[:, y0:y1, x0:x1].sum((1, 2))
            assert float(s.abs().max()) < 2 ** 24
            inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float((y1 - y0) * (x1 - x0)), dtype=F32)
            out[:, oy, ox] = s.float() * inv
    return out.reshape(n_img, out_w * out_w, C).to(dtype)


def s2d_reference(x, g):
    """DownSampleBlock on [n, g * g, C]: out token bc * hb + br = [x(2br, 2bc) | x(2br, 2bc + 1) | x(2br + 1, 2bc) | x(2br + 1, 2bc + 1)],
    zero outside the grid"""
    n, _, C = x.shape
    hb = (g + 1) // 2
    pad = torch.zeros((n, 2 * hb, 2 * hb, C), dtype=x.dtype)
    pad[:, :g, :g] = x.reshape(n, g, g, C)
    q = pad.reshape(n, hb, 2, hb, 2, C)  # [n, br, dr, bc, dc, C]
    return q.permute(0, 3, 1, 2, 4, 5).reshape(n, hb * hb, 4 * C)


def im2col_reference(img, p, kp):
    """[n, 3, S, S] -> rows (img, py, px) of the pixels ordered (c, ky, kx), zero pad to kp"""
    n, _, S, _ = img.shape
    gw = S // p
    col = img.reshape(n, 3, gw, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(n * gw * gw, 3 * p * p)
    out = torch.zeros((n * gw * gw, kp), dtype=img.dtype)
    out[:, :3 * p * p] = col
    return out
