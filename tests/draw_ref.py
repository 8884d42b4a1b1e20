"""The sampled token, restated on the host: Philox4x32-10, the draw address, the inverse-CDF walk and the Gumbel-max key of
csrc/pick.h and csrc/sample.hip in numpy and torch on the CPU -- no GPU, no import of the library.  tests/test_host_draw_ref.py
proves the restatement (Random123's known answers, the address rules, the mutants below); tests/test_gpu_draw_exact.py holds every
entry point of both device samplers to it, token for token.

THE RULE
  address   Philox counter words (ctr_lo, ctr_hi, seq, w), key (seed_lo, seed_hi).  w = the vocabulary index for a Gumbel key,
            0xFFFFFFFF for the inverse-CDF uniform.  (ctr, seq) = (counter, b) for rows that are sequences; (counter + t, 0), a 64-bit
            sum, for rows that are steps; (counter + max(steps[b], 0) - m + t, b), m = min_b max(steps[b], 0), for sequences x steps.
  scores    fp32(logit) / fp32(T), one correctly rounded fp32 division.
  kept set  HF's warpers on the float64 image of those scores: top-k keeps every tie at the k-th score, top-p sorts ascending (the
            lower index first among equal scores), removes while the cumulative softmax is <= fp32(1 - top_p), never the largest.
  inverse CDF (srgpt_sample, top_k 1 .. 64)   the kept list ranked by (score desc, index desc); x = word 0 of the Philox output,
            u = (x >> 8) * 2^-24 in [0, 1); the token is the first rank r with u * Z < c_r, c_r = sum_{j <= r} exp(s_j - s_0),
            Z = c_{n2 - 1}; if no rank satisfies it, the last one.
  Gumbel-max (srgpt_sample with top_k = 0; srgpt_sample_full over its kept set)   n = x >> 8, u = min(fp32(fp32(n) + 0.5) * 2^-24,
            1 - 2^-24) formed in fp32 exactly as the kernel forms it (n + 0.5 is no fp32 number for n >= 2^23 and rounds half to
            even; the minimum keeps n = 2^24 - 1, which rounds to 2^24, inside (0, 1)); key = score - log(-log(u)); the token is
            the first maximum over the kept entries; an entry of score -inf never wins.

AMBIGUITY is judged by this reference alone, in float64, from the fp32 arithmetic of the kernel's lines.  eps = 2^-24 (half an ulp,
the rounding of one fp32 operation), ulp(x) = 2^(floor(log2 |x|) - 23).

  __expf    The ROCm math headers installed with the toolchain state no error bound for __expf; they define it as
            exp2(fl(log2e_f * x)) on the hardware exp2.  So it is derived: the product rounds (eps relative) and log2e_f itself is
            off by < eps / 2 relative, an absolute error of 1.5 eps |x| log2(e) in the exponent, i.e. 1.5 eps |x| relative in the
            result; the hardware exp2 adds one ulp, 2 eps relative.  A term t = exp(x) therefore carries  t * (2 + 1.5 |x|) * eps.
            E_exp = sum_j t_j (2 + 1.5 |x_j|) eps / Z  is computed per case from the kept scores (<= 2.6 eps for any list).
  d_cdf     (the walk `target < c`, sample_select_kernel)   relative to Z: the n2 sequential fp32 additions of Z2, the same
            additions again in c, and the product u * Z2 -- each partial sum is <= Z, so (n2 + 2) eps bounds the additions that
            matter twice over -- plus E_exp.   d_cdf = 8 * ((n2 + 2) eps + E_exp);   64 kept entries: 8 * 68.6 eps ~ 2^-14.9.
  d_cut     (the top-p cut `c <= top_p_rm` of the same kernel, over the nk entries before the cut)   Z (nk additions), then per
            entry one division and one addition: (2 nk + 2) eps, and E_exp for Z and for c each.
            d_cut = 8 * ((2 nk + 2) eps + 2 E_exp).   The full sampler sums 2^45 fixed-point masses of expf (taken at one ulp:
            the toolchain installs no error table for it either) in integers: no summation error, each mass off by 2 eps relative and 2^-46 absolute, in Z and in the partial
            sum alike:   d_cut_full = 8 * (4 eps + V 2^-45 / Z_fixed) with Z_fixed >= 1, so <= 8 * (4 eps + V 2^-45).
  d_g       (two Gumbel keys)   a = -logf(u) is taken as off by one ulp, 2 eps relative, which moves log(a) by 2 eps absolute; the
            outer logf is off by one ulp of g = log(a); the subtraction rounds to the key: one ulp of the key.
            d_g = 8 * (2 eps + ulp(g) + ulp(key)), at the larger magnitudes of the two best entries.  |g| < 32 and |key| < 32:
            8 * (2^-23 + 2^-19 + 2^-19) ~ 2^-15.  The factor 8 also covers that TWO keys err.
  exact     A kept list of n2 exactly equal scores with n2 a power of two and no top-p filter has no error at all: every term is
            exp2(0) = 1, every sum a small integer, u * n2 exact.  Such a case is never ambiguous, and it is the one place where
            `<` and `<=` in the walk part: u * Z lands ON a c_r.

A case is ambiguous when min_r |u Z - c_r| / Z < d_cdf (r < n2 - 1: the last rank is the fall-through either way), or a float64
top-p cumulative lies within d_cut of fp32(1 - top_p), or the two best keys are closer than d_g.  Then `ok` holds every admissible
token (both neighbours of the contested boundary; with a contested cut, the draws over the list one entry shorter and longer).

MUTANTS: wrong references, one line each, switched on by name (`mut`); the host test shows that each draws another token than
the rule in at least one non-ambiguous case that can see it.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
EPS = 2.0 ** -24
U_MAX = np.float32(1.0 - 2.0 ** -24)  # 0x1.fffffep-1f: the largest fp32 below 1
KEPT_MAX = 256                        # csrc/sample.hip SMP_LIST: capacity of the top-k-64 sampler's kept list

MUTANTS = {
    "word_y": "output word y for x",
    "seq_dropped": "counter word 2 is 0, not the sequence",
    "icdf_word_0": "the inverse-CDF uniform read at index word 0 for 0xFFFFFFFF",
    "ctr_hi_dropped": "counter word 1 is 0, not the counter's high word",
    "seed_hi_dropped": "key word 1 is 0, not the seed's high word",
    "nine_rounds": "nine Philox rounds",
    "gumbel_no_half": "Gumbel u without + 0.5",
    "walk_le": "<= for < in the walk",
    "ties_ascending": "tie groups ranked index ascending",
    "walk_before_top_p": "the walk over the list before the top-p cut",
    "steps_t_in_seq": "rows-are-steps puts t into the sequence word",
    "u_one": "the Gumbel u not kept below 1",
}


# ------------------------------------------------------------------------------------------------ Philox and the address
def philox4x32_10(c0, c1, c2, c3, k0, k1, rounds=10):
    """Philox4x32 on uint64 arrays holding 32-bit words (they broadcast) -> the four output words"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3, k0, k1))
    m = np.uint64(M32)
    for _ in range(rounds):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2  # < 2^64: exact
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return c0, c1, c2, c3


def addr_seqs(counter, b):
    """row b of a launch whose rows are the sequences of one step"""
    return counter & M64, b


def addr_steps(counter, t, mut=frozenset()):
    """row t of a launch whose rows are successive steps of one sequence"""
    if "steps_t_in_seq" in mut:
        return counter & M64, t
    return (counter + t) & M64, 0


def addr_seq_steps(counter, steps, T, b, t):
    """row b * T + t of a launch over len(steps) sequences x T steps (csrc/draw_addr.h)"""
    filled = [max(int(s), 0) for s in steps]
    return (counter + filled[b] - min(filled) + t) & M64, b


def draw_word(seed, ctr, seq, w, mut=frozenset()):
    """word 0 of the Philox output at the address (seed, ctr, seq, w); w may be an array of vocabulary indices"""
    c1 = 0 if "ctr_hi_dropped" in mut else ctr >> 32
    k1 = 0 if "seed_hi_dropped" in mut else (seed >> 32) & M32
    c2 = 0 if "seq_dropped" in mut else seq & M32
    out = philox4x32_10(ctr & M32, c1, c2, w, seed & M32, k1, rounds=9 if "nine_rounds" in mut else 10)
    return out[1] if "word_y" in mut else out[0]


def icdf_n(seed, ctr, seq, mut=frozenset()):
    """the 24 bits of the inverse-CDF uniform: u = n * 2^-24"""
    return int(draw_word(seed, ctr, seq, 0 if "icdf_word_0" in mut else M32, mut)) >> 8


def gumbel_n(seed, ctr, seq, idx, mut=frozenset()):
    """the 24 bits behind the Gumbel uniform of every vocabulary index in idx"""
    return draw_word(seed, ctr, seq, np.asarray(idx, dtype=np.uint64), mut) >> np.uint64(8)


def gumbel_u(n, mut=frozenset()):
    """fp32, exactly as pick_gumbel_key forms it"""
    n = np.asarray(n).astype(np.float32)  # < 2^24: exact
    u = (n if "gumbel_no_half" in mut else n + np.float32(0.5)) * np.float32(2.0 ** -24)
    return u if "u_one" in mut else np.minimum(u, U_MAX)


# ------------------------------------------------------------------------------------------------ scores and kept sets
def scores_of(row, temperature):
    return np.asarray(row, dtype=np.float32) / np.float32(temperature)


def warp_stable(scores, top_k, top_p):
    """generation.warp_logits (temperature already applied) with a STABLE ascending sort (CPU torch.sort's order among ties: lower
    index first), and the oracle's cumulative probability of every entry (nan where top-p is off).
    -> (kept bool [B, V], cp [B, V])"""
    V = scores.shape[-1]
    if top_k is not None and top_k != 0:
        k = min(max(int(top_k), 1), V)
        kth = torch.topk(scores, k, dim=-1).values[..., -1, None]
        scores = scores.masked_fill(scores < kth, float("-inf"))
    cp_at = torch.full_like(scores, float("nan"))
    if top_p is not None and top_p < 1.0:
        sl, si = torch.sort(scores, descending=False, stable=True, dim=-1)
        cp = sl.softmax(dim=-1).cumsum(dim=-1)
        rm = cp <= (1 - top_p)
        rm[..., -1:] = False
        scores = scores.masked_fill(rm.scatter(-1, si, rm), float("-inf"))
        cp_at = cp_at.scatter(-1, si, cp)
    return scores > float("-inf"), cp_at


def _ulp(x):
    x = abs(float(x))
    return 2.0 ** -149 if x < 2.0 ** -126 else 2.0 ** (int(np.floor(np.log2(x))) - 23)


def _p_on(top_p):
    return top_p is not None and top_p < 1.0


def _cut(top_p):
    return float(np.float32(1.0 - float(top_p)))  # srgpt_sampling::top_p_rm


def _kept64(s, top_k, top_p):
    """the warpers on the float64 image of fp32 scores s [V] -> (kept bool [V], cumulative [V] or nan)"""
    kept, cp = warp_stable(torch.from_numpy(s.astype(np.float64))[None], top_k, top_p)
    return kept[0].numpy(), cp[0].numpy()


# ------------------------------------------------------------------------------------------------ the two draws
def ref_sample(row, setting, seed, ctr, seq, mut=frozenset()):
    """srgpt_sample's token for one row at the address (seed, ctr, seq) -> a namespace: tok, ok (the admissible tokens), ambiguous,
    margin and its bound d, u, kept (the kept list, best first; None in Gumbel mode)"""
    temperature, top_k, top_p = setting
    s = scores_of(row, temperature)
    if not top_k:
        assert not _p_on(top_p), "srgpt_sample serves no top-p filter without top-k"
        return _gumbel(s, np.ones(s.size, dtype=bool), seed, ctr, seq, mut)
    assert 1 <= top_k <= 64
    assert int(np.isfinite(s).sum()) >= min(top_k, s.size), "a k-th score of -inf keeps unbounded ties: not a case for this reference"
    idx = np.nonzero(_kept64(s, top_k, None)[0])[0]
    nk = idx.size
    assert nk <= KEPT_MAX, "more ties at the k-th score than the device list holds: not a case for this reference"
    order = np.lexsort((idx if "ties_ascending" in mut else -idx, -s[idx].astype(np.float64)))
    rank = idx[order]  # best first
    x = s[rank].astype(np.float64) - float(s[rank[0]])
    t = np.exp(x)
    e_exp = lambda n: float((t[:n] * (2 + 1.5 * np.abs(np.where(np.isfinite(x[:n]), x[:n], 0.0)))).sum() * EPS / t[:n].sum())
    n2, cut_amb, cut_margin, d_cut = nk, False, np.inf, 0.0
    if _p_on(top_p):
        asc = np.cumsum(t[::-1]) / t.sum()  # ascending cumulative softmax: entry j of it is rank nk - 1 - j
        gone = asc[:-1] <= _cut(top_p)      # never the largest
        n2 = nk - int(gone.sum())
        assert not gone.any() or bool(gone[:int(gone.sum())].all())
        d_cut = 8 * ((2 * nk + 2) * EPS + 2 * e_exp(nk))
        cut_margin = float(np.abs(asc[:-1] - _cut(top_p)).min()) if nk > 1 else np.inf
        cut_amb = cut_margin < d_cut
        if not cut_amb and not mut:  # TopPLogitsWarper itself is the authority on the kept set
            assert sorted(rank[:n2].tolist()) == np.nonzero(_kept64(s, top_k, top_p)[0])[0].tolist()
    n = icdf_n(seed, ctr, seq, mut)
    u = n * 2.0 ** -24

    def walk(m):
        c = np.cumsum(t[:m])
        z = c[-1]
        hit = np.nonzero(u * z <= c if "walk_le" in mut else u * z < c)[0]
        pick = int(hit[0]) if hit.size else m - 1
        exact = not _p_on(top_p) and m & (m - 1) == 0 and bool((x[:m] == 0).all())
        d = 0.0 if exact else 8 * ((m + 2) * EPS + e_exp(m))
        gap = np.abs(u * z - c[:-1]) / z
        near = np.nonzero(gap < d)[0]
        return pick, {pick} | {int(r) for r in near} | {int(r) + 1 for r in near}, float(gap.min()) if gap.size else np.inf, d

    pick, ranks, margin, d = walk(nk if "walk_before_top_p" in mut else n2)
    if cut_amb:
        for m in (n2 - 1, n2 + 1):
            if 1 <= m <= nk:
                ranks |= walk(m)[1]
    return SimpleNamespace(tok=int(rank[pick]), ok={int(rank[r]) for r in ranks}, ambiguous=cut_amb or len(ranks) > 1,
                           cut_ambiguous=cut_amb, margin=min(margin, cut_margin), d=d, d_cut=d_cut, u=u, n=n, kept=rank[:n2].tolist(),
                           rank=pick, kind="icdf")


def _gumbel(s, kept, seed, ctr, seq, mut, also=(), **more):
    """first maximum of score - log(-log(u)) over the kept entries; `also`: other kept masks a contested top-p cut admits"""
    V = s.size
    u32 = gumbel_u(gumbel_n(seed, ctr, seq, np.arange(V), mut), mut)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = -np.log(-np.log(u32.astype(np.float64)))
        key = s.astype(np.float64) + g
    live = s > -np.inf
    toks, margin, d = [], np.inf, 0.0
    for mask in (kept,) + tuple(also):
        k = np.where(mask & live & ~np.isnan(key), key, -np.inf)
        best = int(np.argmax(k))
        toks.append(best)
        if mask is kept:
            rest = k.copy()
            rest[best] = -np.inf
            second = int(np.argmax(rest))
            margin = float(k[best] - rest[second]) if np.isfinite(rest[second]) else np.inf
            gm = max(abs(g[best]), abs(g[second])) if np.isfinite(g[best]) else 32.0
            km = max(abs(k[best]), abs(rest[second]) if np.isfinite(rest[second]) else 0.0) if np.isfinite(k[best]) else 32.0
            d = 8 * (2 * EPS + _ulp(gm) + _ulp(km))
            if margin < d:
                toks += [int(i) for i in np.nonzero(k >= k[best] - d)[0]]
    return SimpleNamespace(tok=toks[0], ok=set(toks), ambiguous=len(set(toks)) > 1 or bool(more.get("cut_ambiguous")), margin=margin, d=d,
                           u=float(u32[toks[0]]), n=None, kind="gumbel", kept=kept, **more)


def ref_sample_full(row, setting, seed, ctr, seq, mut=frozenset()):
    """srgpt_sample_full's token and kept mask for one row at the address (seed, ctr, seq)"""
    temperature, top_k, top_p = setting
    s = scores_of(row, temperature)
    kept, cp = _kept64(s, top_k, top_p)
    also, cut_amb, d_cut, cut_margin = (), False, 0.0, np.inf
    if _p_on(top_p):
        d_cut = 8 * (4 * EPS + s.size * 2.0 ** -45)
        before, _ = _kept64(s, top_k, None)
        last = np.lexsort((np.arange(s.size), s))[-1]  # the largest entry (highest index among equals): never removed
        band = before & (np.abs(cp - _cut(top_p)) < d_cut)
        band[last] = False
        cut_margin = float(np.abs(cp - _cut(top_p))[before & (np.arange(s.size) != last)].min()) if before.sum() > 1 else np.inf
        cut_amb = bool(band.any())
        if cut_amb:
            also = (kept & ~band, kept | band)
    return _gumbel(s, kept, seed, ctr, seq, mut, also=also, cut_ambiguous=cut_amb, d_cut=d_cut, cut_margin=cut_margin)


def ref_draw(which, row, setting, seed, ctr, seq, mut=frozenset()):
    return (ref_sample if which == "sample" else ref_sample_full)(row, setting, seed, ctr, seq, mut)


# ------------------------------------------------------------------------------------------------ the cases both test files run
VOCABS = (1, 70, 129, 1000, 32002, 128258, 262144)  # fewer entries than slices, ragged last slices, the vocabulary limit
SEEDS = (1, 2 ** 32 + 7, 2 ** 64 - 1)
COUNTERS = (0, 5, 2 ** 32 - 2, 2 ** 32 + 41)        # six calls from 2^32 - 2 cross the carry into the high word
SETTINGS = {"sample": ((1.0, 0, None), (0.2, 50, None), (0.7, 50, 0.9), (1.3, 64, 0.95), (1.0, 1, None), (5.0, 64, None), (0.05, 8, None)),
            "sample_full": ((1.0, 0, None), (0.7, 0, 0.9), (0.7, 1000, None), (1.3, 64, 0.95), (1.0, 0, 0.0))}
ROW_PLAIN, ROW_TIES, ROW_NEG_INF, ROW_ONE_FINITE = range(4)
HEAD = 40

# addresses found with the Philox above (re-checked by the host test): seed 1, sequence 0
EDGE_GUMBEL = ((15, 102788), (86, 50897), (261, 79736))     # (counter, vocabulary index): n = 0xFFFFFF, the u that rounded to 1
EDGE_ICDF_LAST, EDGE_ICDF_ZERO = 4307477616, 4310220570     # counters: n = 0xFFFFFF (the largest u), n = 0
EDGE_WALK_EXACT = ((4295135531, 26), (4295400006, 1), (4297630933, 33))  # (counter, j): n = j * 2^18, so u * 64 = j exactly
EDGE_V = 128258
EDGE_BELOW = 30.0   # the hit entry sits this far below the row maximum: its honest key loses by ~ 10 or more


def _hash(V, salt):
    x = np.arange(4 * V, dtype=np.uint32)
    with np.errstate(over="ignore"):
        x = (x + np.uint32(0x9E3779B9 + salt)) * np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(13)
    return x.reshape(4, V)


def head_indices(V):
    """the vocabulary indices of the planted head, lowest value first, spread over the slices"""
    H = min(HEAD, V // 2)
    return [(7 + j * (V // H)) % V for j in range(H)] if H else []


@functools.lru_cache(maxsize=None)
def case_logits(V):
    """fp32 [4, V] from an integer hash of the index (as tests/pick_kat.py::hashed_logits): a bulk in [-8, 8) under a head of up to
    40 entries at 9 + j / 4 + jitter, so that the kept mass sits on few entries, as a language model's does, and a top-p cut falls
    between well separated cumulatives.  Row 1 plants exactly equal scores at ranks 1 .. 4 and 7 .. 8, row 2 sets an eighth of
    the bulk to -inf, row 3 is -inf but for one entry."""
    h = _hash(V, V)
    lg = (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -20) - np.float32(8.0)
    idx = head_indices(V)
    H = len(idx)
    for r in range(3):
        for j, i in enumerate(idx):
            lg[r, i] = np.float32(9.0 + 0.25 * j) + np.float32((int(h[r, i]) & 0xFF) / 2048.0)
    if H >= 10:
        for group in ((H - 2, H - 3, H - 4, H - 5), (H - 8, H - 9)):
            lg[ROW_TIES, [idx[j] for j in group]] = np.float32(9.0 + 0.25 * group[-1])
    if V >= 70:
        gone = (h[ROW_NEG_INF] & np.uint32(7)) == 0
        gone[idx] = False
        lg[ROW_NEG_INF, gone] = -np.inf
    one = (V * 5) // 7
    lg[ROW_ONE_FINITE] = np.where(np.arange(V) == one, lg[ROW_ONE_FINITE], np.float32(-np.inf))
    lg.setflags(write=False)
    return lg


def chains():
    """the thinned product of shapes, addresses and settings: every V with every setting once, B, seed and start counter rotating
    through their values; six consecutive calls at the small vocabularies and wherever the calls cross the counter's carry, two
    elsewhere; then the one-finite-entry row through every path that can take it.
    -> dicts: which, setting, V, rows (the rows of case_logits(V) the B sequences read), seed, counter, calls"""
    n = 0
    for which, settings in SETTINGS.items():
        for setting in settings:
            for V in VOCABS:
                B, seed, counter = (1, 3)[n % 2], SEEDS[n % 3], COUNTERS[(n // 2) % 4]
                rows = (ROW_PLAIN, ROW_TIES, ROW_NEG_INF) if B == 3 else ((n // 2) % 3,)
                yield dict(which=which, setting=setting, V=V, rows=rows, seed=seed, counter=counter,
                           calls=6 if V <= 1000 or counter == 2 ** 32 - 2 else 2)
                n += 1
    for V in (70, 32002):
        for which, setting in (("sample", (1.0, 0, None)), ("sample", (1.0, 1, None)), ("sample_full", (1.0, 0, None)),
                               ("sample_full", (0.7, 0, 0.9)), ("sample_full", (0.7, 1000, None))):
            yield dict(which=which, setting=setting, V=V, rows=(ROW_ONE_FINITE,), seed=SEEDS[n % 3], counter=COUNTERS[n % 4], calls=2)
            n += 1


def chain_id(c):
    t, k, p = c["setting"]
    return f"{c['which']}-T{t}-k{k}-p{p}-V{c['V']}-B{len(c['rows'])}-s{c['seed'] % 1000}-c{c['counter']}"


def edge_gumbel_row(hit):
    """row 0 of the V = 128258 logits with the hit entry planted 30 below the row maximum"""
    row = case_logits(EDGE_V)[ROW_PLAIN].copy()
    assert hit not in head_indices(EDGE_V)
    row[hit] = row.max() - np.float32(EDGE_BELOW)
    return row


def walk_exact_row(V=1000):
    """64 exactly equal scores above everything else: under top_k = 64 the walk is exact integer arithmetic"""
    row = case_logits(V)[ROW_PLAIN].copy()
    row[3 + 15 * np.arange(64)] = np.float32(24.0)
    return row


@functools.lru_cache(maxsize=None)
def ref_chain_row(which, setting, V, row, seed, ctr, seq):
    """the reference of one row of a chain call, computed once for both test files' use within a process"""
    return ref_draw(which, case_logits(V)[row], setting, seed, ctr, seq)


NO_HALF_V, NO_HALF_CTR = 262144, 7


@functools.lru_cache(maxsize=None)
def no_half_row():
    """-> (row, a, b): -inf but for two entries.  At (seed 1, counter 7, sequence 0) entry a holds the largest odd n >= 2^23 of the
    vocabulary, which n + 0.5 rounds UP to n + 1, and entry b the largest even n, which stays.  b's logit puts its key midway
    between a's key with and without the + 0.5: the rule draws a, a u without + 0.5 draws b, either by some 250 d_g."""
    n = gumbel_n(1, NO_HALF_CTR, 0, np.arange(NO_HALF_V)).astype(np.int64)
    odd = (n & 1 == 1) & (n >= 2 ** 23) & (n < 0xFFFFFF)
    a, b = int(np.argmax(np.where(odd, n, 0))), int(np.argmax(np.where(n & 1 == 0, n, 0)))
    g = lambda m, mut=frozenset(): -np.log(-np.log(float(gumbel_u(m, mut))))
    row = np.full(NO_HALF_V, -np.inf, dtype=np.float32)
    row[a], row[b] = 0.0, np.float32((g(n[a]) + g(n[a], {"gumbel_no_half"})) / 2 - g(n[b]))
    row.setflags(write=False)
    return row, a, b


MODE_V = 32002
MODE_SETTINGS = (("sample", (1.0, 0, None)), ("sample", (0.7, 50, 0.9)), ("sample_full", (0.7, 0, 0.9)), ("sample_full", (0.7, 1000, None)))
STEPS_ROWS, STEPS_SEED, STEPS_COUNTERS = (0, 1, 2, 0), 2 ** 32 + 7, (5, 2 ** 32 - 2)          # T = 4 rows that are steps
SEQ_ROWS, SEQ_T, SEQ_SEED, SEQ_COUNTER, SEQ_STEPS = (0, 1, 2, 2, 0, 1), 3, 2 ** 64 - 1, 2 ** 32 - 2, ((5, 2), (-3, 2))
WALK_EDGE_SETTINGS = ((5.0, 64, None), (0.7, 50, 0.9))


def mode_rows(mut=frozenset()):
    """every row of the two other row modes -> (group, which, setting, logits row, seed, ctr, seq, t)"""
    lg = case_logits(MODE_V)
    for which, setting in MODE_SETTINGS:
        for counter in STEPS_COUNTERS:
            for t, row in enumerate(STEPS_ROWS):
                yield ("steps", which, setting, lg[row], STEPS_SEED) + addr_steps(counter, t, mut) + (t,)
        for steps in SEQ_STEPS:
            for r, row in enumerate(SEQ_ROWS):
                yield ("seq_steps", which, setting, lg[row], SEQ_SEED) + addr_seq_steps(SEQ_COUNTER, steps, SEQ_T, r // SEQ_T, r % SEQ_T) + (r % SEQ_T,)


def edge_rows():
    """the planted edge draws, all at seed 1, sequence 0 -> (name, which, setting, logits row, ctr)"""
    for setting in WALK_EDGE_SETTINGS:
        for name, ctr in (("walk_zero", EDGE_ICDF_ZERO), ("walk_last", EDGE_ICDF_LAST)):
            yield name, "sample", setting, case_logits(1000)[ROW_PLAIN], ctr
    for ctr, _ in EDGE_WALK_EXACT:
        yield "walk_exact", "sample", (1.0, 64, None), walk_exact_row(), ctr
    for ctr, hit in EDGE_GUMBEL:
        for which, setting in (("sample", (1.0, 0, None)), ("sample_full", (1.0, 0, None)), ("sample_full", (1.0, 64, None))):
            yield "gumbel_ones", which, setting, edge_gumbel_row(hit), ctr
    for which in ("sample", "sample_full"):
        yield "no_half", which, (1.0, 0, None), no_half_row()[0], NO_HALF_CTR
