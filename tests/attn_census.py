"""The attention census: inputs on which every softmax weight is exactly 1 or underflows to nothing, and whose V rows spell the index
of their key, so that an output row times the number of keys it should have seen is a table of integer counts -- which keys were
summed, and how often.  One key too many, too few or twice moves a count of at most ~10 by 1, where on random data it moves the
output by 1 / n of its range.  Shared by tests/test_host_attn_census.py (the float64 reference against mutant references, no GPU) and
tests/test_gpu_attention_census.py (every attention entry point against the reference).

Data, the same for every entry point:
  V[b, j, hk, :]  a two-part one-hot code of j, rotated by hk + b: with Hd = D // 2, channel (j % Hd + hk + b) % Hd of the first half
                  and channel Hd + (j // Hd + hk + b) % Hd of the second are 1, everything else 0 (at most Hd * Hd keys);
  K[b, j, hk, :]  a * e[j % D];
  q               0 ("uniform": the plain mean over the visible keys), a * e[r] with r the residue of the row's FIRST INVISIBLE key
                  ("lit_next": the mean over the visible keys of that residue class, unless the mask lets the lure through) or of
                  its LAST VISIBLE key ("lit_last": dropping that key loses the dominant term);
  a               the smallest power of two with a * a * scale >= 64 nats: a lit logit beats an unlit one by e^64 at least.
The decode entries (identity RoPE tables) get a lure in every cache row at or behind the row's position: K = a * e[r], V = 7 in
channel D - 1, which no code uses there.

The reference is the float64 masked softmax of include/srgpt.h's rule: key s is visible to query t of row b iff s <= q_pos0[b] + t
(where the call is causal) and s < min(kv_len[b], Tk); a query without a visible key yields zeros."""
import functools
import math
from dataclasses import dataclass
from typing import Optional

import torch

BF16, F32 = torch.bfloat16, torch.float32
FAMILIES = ("uniform", "lit_next", "lit_last")
# the weights are 1 up to 1e-5 (flash.hip's fma residue), sums of 0 / 1 values and of weights are integers below 2^24: what is left
# is the normalisation in fp32 and the store -- two ulps of the output type
REL = {BF16: 2.0 ** -7, F32: 2.0 ** -20}
ZERO = 2.0 ** -60  # where the reference is 0 (in float64: an unlit weight, below e^-64)
LURE = 7.0
MARGIN = 8.0       # a mutant has to move an element by this many tolerances: the smallest designed effect is 1 in ~10 against 1 in 128

MUTANTS = {
    1: "every row sees its first invisible key",
    2: "every row loses its last visible key",
    3: "every row loses key 0",
    4: "each key at a multiple of 64 is dropped",
    5: "each key at a multiple of 64 is counted twice",
    6: "kv_len is ignored",
    7: "kv_len[0] is used for all rows",
    8: "q_pos0[0] / pos[0] is used for all rows",
    9: "query head h reads kv head h % Hkv",
    10: "batch row b reads row 0's K / V",
}


def amplitude(D, scale=None):
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    a = 1.0
    while a * a * scale < 64.0:
        a *= 2.0
    return a


@functools.lru_cache(maxsize=None)
def v_codes(B, n, Hkv, D):
    """[B, n, Hkv, D] fp32: the code of key j in row b, kv head hk (shared between the problems: never written to)"""
    Hd = D // 2
    assert n <= Hd * Hd, (n, D)
    j = torch.arange(n)
    v = torch.zeros((B, n, Hkv, D), dtype=F32)
    for b in range(B):
        for hk in range(Hkv):
            v[b, j, hk, (j % Hd + hk + b) % Hd] = 1.0
            v[b, j, hk, Hd + (j // Hd + hk + b) % Hd] = 1.0
    return v


@functools.lru_cache(maxsize=None)
def k_dirs(n, D, a):
    """[n, D] fp32: a * e[j % D] (shared, never written to)"""
    k = torch.zeros((n, D), dtype=F32)
    j = torch.arange(n)
    k[j, j % D] = a
    return k


def visible(q_pos0, kv_len, Tk, B, Tq, S):
    """include/srgpt.h's rule -> bool [B, Tq, S]; q_pos0 None = not causal, kv_len None = Tk"""
    s = torch.arange(S)
    m = torch.empty((B, Tq, S), dtype=torch.bool)
    for b in range(B):
        n = Tk if kv_len is None else min(int(kv_len[b]), Tk)
        row = (s < n)[None, :].expand(Tq, S)
        if q_pos0 is not None:
            row = row & (s[None, :] <= int(q_pos0[b]) + torch.arange(Tq)[:, None])
        m[b] = row
    return m


@dataclass
class Problem:
    """one launch: q [B, Tq, Hq, D], k / v [B, S, Hkv, D] (fp32 holding values every dtype has; S: the key rows there are, or for a
    decode entry those any row can reach), the rule's arguments, and -- decode entries -- the launch's raw inputs"""
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    q_pos0: Optional[list]
    kv_len: Optional[list]
    Tk: int
    scale: float
    what: str = ""
    qkv: Optional[torch.Tensor] = None       # decode: [B, T, (Hq + 2 Hkv) D]
    kc0: Optional[torch.Tensor] = None       # decode: the head of the caches before the launch, [B, Hkv, S, D] (decode_problem)
    vc0: Optional[torch.Tensor] = None
    lure_res: Optional[torch.Tensor] = None  # decode: [B, T], the residues the lures behind the head cycle through


def multiplicity(p, mutant=None):
    """how often query (b, t) counts key s -> double [B, Tq, S] (the rule: 0 / 1)"""
    B, Tq, S = p.q.shape[0], p.q.shape[1], p.k.shape[1]
    q_pos0, kv_len = p.q_pos0, p.kv_len
    if mutant == 6 and kv_len is not None:
        kv_len = None
    if mutant == 7 and kv_len is not None:
        kv_len = [kv_len[0]] * B
    if mutant == 8 and q_pos0 is not None:
        q_pos0 = [q_pos0[0]] * B
    m = visible(q_pos0, kv_len, p.Tk, B, Tq, S).double()
    n = m.sum(-1).long()  # the visible keys are a prefix
    if mutant == 1:
        m.scatter_add_(2, n.clamp(max=S - 1)[..., None], (n < S).double()[..., None])
    if mutant == 2:
        m.scatter_(2, (n - 1).clamp(min=0)[..., None], torch.zeros((B, Tq, 1), dtype=torch.float64))
    if mutant == 3:
        m[..., 0] = 0
    if mutant == 4:
        m[..., ::64] = 0
    if mutant == 5:
        m[..., ::64] *= 2
    return m


def reference(p, mutant=None, census=False):
    """float64 softmax(scale * q k^T + mask) v by the header's rule -> out [B, Tq, Hq, D]; with census: (out, n_lit [B, Tq, Hq],
    counts [B, Tq, Hq, D]) -- the number of keys that carry the row's maximal logit and the sum of their V rows.  `mutant`: one of
    MUTANTS, a reference that is wrong in that way."""
    B, Tq, Hq, D = p.q.shape
    Hkv = p.k.shape[2]
    G = Hq // Hkv
    m = multiplicity(p, mutant)
    used = int(m.amax((0, 1)).nonzero().max()) + 1 if bool(m.any()) else 1  # no key behind the last one anybody counts
    m = m[..., :used]
    hmap = torch.tensor([h % Hkv if mutant == 9 else h // G for h in range(Hq)])
    kk, vv = p.k[:, :used].double()[:, :, hmap], p.v[:, :used].double()[:, :, hmap]  # [B, used, Hq, D]
    if mutant == 10:
        kk, vv = kk[:1].expand(B, -1, -1, -1), vv[:1].expand(B, -1, -1, -1)
    m = m[:, None]                                                                   # [B, 1, Tq, used]
    logit = (torch.einsum("bthd,bshd->bhts", p.q.double(), kk) * p.scale).masked_fill(m == 0, float("-inf"))
    mx = logit.amax(-1, keepdim=True)
    some = torch.isfinite(mx)  # a query without a visible key: zeros
    w = torch.where(some, m * torch.exp(logit - torch.where(some, mx, torch.zeros_like(mx))), torch.zeros_like(logit))
    den = w.sum(-1, keepdim=True)
    out = torch.einsum("bhts,bshd->bthd", w / torch.where(some, den, torch.ones_like(den)), vv)
    if census:
        lit = torch.where(some & (logit == mx), m.expand_as(logit), torch.zeros_like(logit))
        n_lit, counts = lit.sum(-1).transpose(1, 2), torch.einsum("bhts,bshd->bthd", lit, vv)
        return out, n_lit, counts
    return out


def applies(p, mutant):
    """whether the mutant changes, for any query, WHICH keys the softmax weighs (a sole key counted twice normalises away; a mapping
    mutant needs a second kv head / batch row to go wrong with)"""
    B, Hq, Hkv = p.q.shape[0], p.q.shape[2], p.k.shape[2]
    if mutant == 9:
        return Hkv > 1 and Hq // Hkv > 1
    if mutant == 10:
        return B > 1
    a, b = multiplicity(p), multiplicity(p, mutant)
    norm = lambda m: m / m.sum(-1, keepdim=True).clamp(min=1)  # noqa: E731
    return not torch.equal(norm(a), norm(b))


def tolerance(ref, dtype):
    return torch.where(ref.abs() < ZERO, torch.full_like(ref, ZERO), REL[dtype] * ref.abs())


def margin(p, mutant, dtype, ref=None):
    """max over the elements of |mutant reference - reference| / tolerance"""
    ref = reference(p) if ref is None else ref
    return float(((reference(p, mutant) - ref).abs() / tolerance(ref, dtype)).max())


# ------------------------------------------------------------------------------------------------ the data
def _queries(n_vis, family, Hq, D, a):
    """n_vis [B, Tq]: the visible keys of a row are 0 .. n_vis - 1, so n_vis is its first invisible key"""
    B, Tq = n_vis.shape
    q = torch.zeros((B, Tq, Hq, D), dtype=F32)
    if family != "uniform":
        r = (n_vis if family == "lit_next" else (n_vis - 1).clamp(min=0)) % D
        q.scatter_(3, r[:, :, None, None].expand(B, Tq, Hq, 1), a)
    return q


def prefill_problem(family, B, Tq, Tk, Hq, Hkv, D, q_pos0, kv_len, what=""):
    """srgpt_attention (causal: q_pos0 = [Tk - Tq] * B, else None) and srgpt_attention_append over Tk key rows"""
    assert family in FAMILIES
    a = amplitude(D)
    n_vis = visible(q_pos0, kv_len, Tk, B, Tq, Tk).sum(-1)
    k = k_dirs(Tk, D, a)[None, :, None, :].expand(B, Tk, Hkv, D).contiguous()
    return Problem(_queries(n_vis, family, Hq, D, a), k, v_codes(B, Tk, Hkv, D), q_pos0, kv_len, Tk, 1.0 / math.sqrt(D),
                   f"{family} {what}")


def decode_problem(family, pos, T, Hq, Hkv, D, max_pos, what=""):
    """srgpt_decode_attention (T = 1) / srgpt_decode_attention_multi: row b has pos[b] tokens cached and appends T.  The caches
    before the launch hold the codes in rows [0, pos[b]) and a lure in every row from pos[b] on (those the launch appends included:
    it has to overwrite them).  Only the HEAD of the caches, rows [0, S) with S one past the last row any launch row appends, is
    kept here -- kc0 / vc0 before the launch, Problem.k / .v as the launch must leave it; everything behind is lures, which
    decode_caches() spells out."""
    assert family in FAMILIES
    B, Hd, a = len(pos), D // 2, amplitude(D)
    assert D % 2 == 0 and min(pos) >= 0 and max(pos) + T <= max_pos
    assert (max(pos) + T - 1) // Hd + (Hkv - 1) + (B - 1) < Hd - 1, "channel D - 1 belongs to the lures"
    S = min(max_pos, max(pos) + T + 1)
    n_vis = torch.tensor(pos)[:, None] + torch.arange(T)[None, :] + 1  # [B, T]
    q = _queries(n_vis, family, Hq, D, a)
    res = (n_vis - 1 if family == "lit_last" else n_vis) % D  # the lit residue of (b, t); uniform: that of lit_next
    nat_k, nat_v = k_dirs(S, D, a), v_codes(B, S, Hkv, D)
    kc0 = torch.zeros((B, Hkv, S, D), dtype=F32)
    vc0 = torch.zeros((B, Hkv, S, D), dtype=F32)
    vc0[..., D - 1] = LURE
    s = torch.arange(S)
    for b, pb in enumerate(pos):
        kc0[b, :, s, res[b][(s - pb) % T]] = a
        kc0[b, :, :pb] = nat_k[:pb]
        vc0[b, :, :pb] = nat_v[b, :pb].transpose(0, 1)
    kc, vc = kc0.clone(), vc0.clone()
    new_k = torch.empty((B, T, Hkv, D), dtype=F32)
    new_v = torch.empty((B, T, Hkv, D), dtype=F32)
    for b, pb in enumerate(pos):
        new_k[b] = nat_k[pb:pb + T, None, :]
        new_v[b] = nat_v[b, pb:pb + T]
        kc[b, :, pb:pb + T] = new_k[b].transpose(0, 1)
        vc[b, :, pb:pb + T] = new_v[b].transpose(0, 1)
    qkv = torch.cat([q.reshape(B, T, -1), new_k.reshape(B, T, -1), new_v.reshape(B, T, -1)], -1)
    return Problem(q, kc.transpose(1, 2), vc.transpose(1, 2), list(pos), None, max_pos, 1.0 / math.sqrt(D),
                   f"{family} pos {list(pos)} T {T} {what}", qkv, kc0, vc0, res)


def decode_caches(p, dtype, device):
    """the whole caches of a decode problem on the device, [B, Hkv, max_pos, D]: (k, v) before the launch and (k, v) as the launch
    must leave them -- the head from the problem, lures from there to the cache's end"""
    B, Hkv, S, D = p.kc0.shape
    max_pos, T, a = p.Tk, p.q.shape[1], amplitude(D)
    kc = torch.zeros((B, Hkv, max_pos, D), dtype=dtype, device=device)
    vc = torch.zeros((B, Hkv, max_pos, D), dtype=dtype, device=device)
    vc[..., D - 1] = LURE
    if max_pos > S:
        s = torch.arange(S, max_pos, device=device)
        for b, pb in enumerate(p.q_pos0):
            kc[b, :, s, p.lure_res[b].to(device)[(s - pb) % T]] = a
    k_want, v_want = kc.clone(), vc.clone()
    kc[:, :, :S], vc[:, :, :S] = p.kc0.to(device=device, dtype=dtype), p.vc0.to(device=device, dtype=dtype)
    k_want[:, :, :S] = p.k.transpose(1, 2).to(device=device, dtype=dtype)
    v_want[:, :, :S] = p.v.transpose(1, 2).to(device=device, dtype=dtype)
    return kc, vc, k_want, v_want


# ------------------------------------------------------------------------------------------------ the census
def _describe(diff, b, hk, D, vis_row, lures):
    """diff [D]: counted minus expected, of one (row, query, head) -> which keys that spells"""
    Hd, rot = D // 2, hk + b
    parts = []
    if lures and diff[D - 1] != 0:
        parts.append(f"channel {D - 1} off by {float(diff[D - 1]):g}: a lure at or behind the row's position was read")
        diff = diff.clone()
        diff[D - 1] = 0
    lo = {(c - rot) % Hd: int(diff[c]) for c in range(Hd) if diff[c] != 0}
    hi = {(c - Hd - rot) % Hd: int(diff[c]) for c in range(Hd, 2 * Hd) if diff[c] != 0}
    keys = [(h * Hd + l, dl) for l, dl in lo.items() for h, dh in hi.items() if (dl > 0) == (dh > 0)]
    if keys and len(keys) <= 8:
        for j, d in keys:
            if d < 0:
                parts.append(f"key {j} missing")
            elif j < len(vis_row) and bool(vis_row[j]):
                parts.append(f"key {j} counted twice")
            else:
                parts.append(f"key {j} extra (not visible to this query)")
        if len(lo) * len(hi) > 1:
            parts.append("(candidates: the two halves of the code do not pair up uniquely)")
    elif lo or hi:
        parts.append(f"keys with j % {Hd} in {lo} and j // {Hd} in {hi} (residue: counted minus expected)")
    return "; ".join(parts)


def census_error(got, p, dtype):
    """None if `got` [B, Tq, Hq, D] is the census of Problem p, else the message: the closeness that failed and, decoded, the first
    query whose integer counts are off with the keys that are missing, counted twice or extra"""
    ref, n_lit, counts = reference(p, census=True)
    got = got.detach().double().cpu().reshape(ref.shape)
    msgs = []
    if not bool(torch.isfinite(got).all()):
        return f"{p.what}: {int((~torch.isfinite(got)).sum())} elements are not finite"
    excess = (got - ref).abs() / tolerance(ref, dtype)
    if float(excess.max()) > 1.0:
        i = [int(x) for x in (excess == excess.max()).nonzero()[0]]
        msgs.append(f"|got - ref| = {float(excess.max()):.3g} x the tolerance at (row, query, head, channel) = {tuple(i)}: "
                    f"got {float(got[tuple(i)])!r}, ref {float(ref[tuple(i)])!r}")
    cnt = (got * n_lit[..., None]).round()
    bad = (cnt != counts).any(-1)
    if bool(bad.any()):
        b, t, h = (int(x) for x in bad.nonzero()[0])
        Hq, Hkv, D = ref.shape[2], p.k.shape[2], ref.shape[3]
        vis = multiplicity(p)[b, t] > 0
        # a key too many or too few also changes what the row was divided by: the count nearest the expected one at which the row
        # is a table of integers
        n0 = int(n_lit[b, t, h])
        fits = [n for n in sorted(range(max(1, n0 - 12), n0 + 13), key=lambda n: abs(n - n0))
                if float((got[b, t, h] * n - (got[b, t, h] * n).round()).abs().max()) < 0.2]
        n1 = fits[0] if fits else n0
        msgs.append(f"census of row {b}, query {t}, head {h} (kv head {h // (Hq // Hkv)}; {int(vis.sum())} keys visible, {n0} lit, "
                    f"the output reads as a sum over {n1}): "
                    + _describe((got[b, t, h] * n1).round() - counts[b, t, h], b, h // (Hq // Hkv), D, vis, p.kc0 is not None)
                    + f"; {int(bad.sum())} of {bad.numel()} (row, query, head) censuses are off")
    return f"{p.what}: " + " | ".join(msgs) if msgs else None


# ------------------------------------------------------------------------------------------------ the cases
# Each names the kernel it expects from csrc/attn_route.h ("route"); the GPU test asserts it through the route CLIs.
@dataclass
class Case:
    id: str
    entry: str                 # attention / append / decode / multi
    dtype: torch.dtype
    Hq: int
    Hkv: int
    D: int
    route: tuple               # (family, instance ...)
    B: int = 0
    Tq: int = 0
    Tk: int = 0
    causal: bool = True
    kv_len: Optional[list] = None
    q_pos0: Optional[list] = None
    max_pos: int = 0
    T: int = 1
    launches: tuple = ()       # decode / multi: the pos list of every launch
    inapplicable: tuple = ()   # mutants of 1 .. 5 no data of this shape can show, with the reason in the id's comment

    def problems(self, family):
        """the launches of this case for one query family"""
        if self.entry in ("attention", "append"):
            q_pos0 = self.q_pos0 if self.entry == "append" else [self.Tk - self.Tq] * self.B if self.causal else None
            return [prefill_problem(family, self.B, self.Tq, self.Tk, self.Hq, self.Hkv, self.D, q_pos0, self.kv_len, self.id)]
        return [decode_problem(family, pos, self.T, self.Hq, self.Hkv, self.D, self.max_pos, self.id) for pos in self.launches]


def _cases():
    c = []
    dt = {BF16: "bf16", F32: "f32"}
    # srgpt_attention, flash
    for Tq, Tk in ((1, 1), (64, 64), (65, 65), (130, 130), (17, 147), (65, 130)):
        for lens in (None, [Tk, 63]):
            # Tk = 1: there is no key behind the only one (1), and a sole key counted twice is the same mean (5)
            c.append(Case(f"flash128-causal-{Tq}x{Tk}-{'len' if lens else 'nolen'}", "attention", BF16, 4, 2, 128, ("flash", 128), B=2, Tq=Tq,
                          Tk=Tk, kv_len=lens, inapplicable=(1, 5) if Tk == 1 else ()))
    for Tk in (64, 65, 129):
        c.append(Case(f"flash128-full-{Tk}", "attention", BF16, 4, 2, 128, ("flash", 128), B=2, Tq=Tk, Tk=Tk, causal=False, kv_len=[Tk, 1]))
    for Tk in (64, 65, 200):
        # Tk <= 65: kv_len[1] = 65 clamps to Tk, every key is visible and there is no first invisible one (1)
        c.append(Case(f"flash96-full-{Tk}", "attention", BF16, 2, 2, 72, ("flash", 96), B=2, Tq=Tk, Tk=Tk, causal=False, kv_len=[Tk, 65],
                      inapplicable=(1,) if Tk <= 65 else ()))
    for causal in (True, False):
        c.append(Case(f"flash64-{'causal' if causal else 'full'}-130", "attention", BF16, 4, 2, 64, ("flash", 64), B=2, Tq=130, Tk=130,
                      causal=causal, kv_len=None if causal else [130, 67]))
    c.append(Case("flash96-causal-65", "attention", BF16, 2, 2, 72, ("flash", 96), B=2, Tq=65, Tk=65, kv_len=[65, 64]))
    c.append(Case("flash32-causal-130", "attention", BF16, 4, 2, 32, ("flash", 32), B=2, Tq=130, Tk=130))
    c.append(Case("flash32-full-130", "attention", BF16, 4, 2, 32, ("flash", 32), B=2, Tq=130, Tk=130, causal=False, kv_len=[130, 65]))
    # srgpt_attention, one wave per row
    c.append(Case("onewave-f32-d16-64", "attention", F32, 4, 2, 16, ("one_wave",), B=2, Tq=64, Tk=64, kv_len=[64, 33]))
    c.append(Case("onewave-f32-d128-65x130", "attention", F32, 4, 2, 128, ("one_wave",), B=2, Tq=65, Tk=130, kv_len=[130, 100]))
    c.append(Case("onewave-bf16-d20-100", "attention", BF16, 4, 2, 20, ("one_wave",), B=2, Tq=100, Tk=100, kv_len=[100, 41]))
    # srgpt_attention_append
    for name, dtype, D, route in (("flash128", BF16, 128, ("flash", 128)), ("onewave-f32-d64", F32, 64, ("one_wave",))):
        c.append(Case(f"append-{name}-65", "append", dtype, 4, 2, D, route, B=3, Tq=65, Tk=195, q_pos0=[0, 63, 130], kv_len=[65, 128, 195]))
        c.append(Case(f"append-{name}-65-cut", "append", dtype, 4, 2, D, route, B=3, Tq=65, Tk=195, q_pos0=[0, 63, 130],
                      kv_len=[65, 100, 195]))
        c.append(Case(f"append-{name}-1", "append", dtype, 4, 2, D, route, B=3, Tq=1, Tk=128, q_pos0=[0, 64, 127], kv_len=[1, 65, 128]))
    # srgpt_decode_attention, MFMA: Hkv = 2, B = 4
    for G in (1, 2, 4, 8):
        c.append(Case(f"decode-mfma-G{G}-384", "decode", BF16, 2 * G, 2, 128, ("decode_mfma", G, 6, 64), max_pos=384,
                      launches=([0, 1, 62, 63], [64, 65, 127, 128], [129, 191, 192, 320])))
        c.append(Case(f"decode-mfma-G{G}-8192", "decode", BF16, 2 * G, 2, 128, ("decode_mfma", G, 64, 128), max_pos=8192,
                      launches=([127, 128, 129, 255], [256, 257, 127, 129])))
    # srgpt_decode_attention, VALU: the chunks follow the sequence length, so the sweep moves their edges over every small position
    # one sequence: 16 splits of ceil((pos + 1) / 16) keys -- both sides of every position at which the chunk grows, not each one
    sweep1 = tuple([p] for p in (0, 1, 2, 14, 15, 16, 17, 30, 31, 32, 33, 40, 255, 256, 257, 511))
    sweep2 = tuple([p, 40 - p] for p in range(21)) + ([255, 256], [257, 511])
    for name, dtype, Hq, Hkv in (("f32-G1", F32, 2, 2), ("f32-G4", F32, 8, 2), ("bf16-G2", BF16, 4, 2)):
        G = Hq // Hkv
        c.append(Case(f"decode-valu-{name}-B1", "decode", dtype, Hq, Hkv, 64, ("decode_valu", G, 16), max_pos=512, launches=sweep1))
        c.append(Case(f"decode-valu-{name}-B2", "decode", dtype, Hq, Hkv, 64, ("decode_valu", G, 8), max_pos=512, launches=sweep2))
    # srgpt_decode_attention_multi: the T new rows straddle a 64-key range; row t's lure is row t + 1's own key
    for G, T in ((4, 2), (4, 4), (1, 16), (8, 2), (2, 8), (1, 2), (2, 2)):  # the last two: the instances of 2 and 4 columns
        nc = next(n for n in (2, 4, 8, 16) if n >= G * T)
        c.append(Case(f"multi-mfma-G{G}-T{T}", "multi", BF16, 2 * G, 2, 128, ("multi_mfma", G, nc, 6, 64), max_pos=384, T=T,
                      launches=([0, 62, 63, 64],)))
    c.append(Case("multi-composed-f32-d64-T3", "multi", F32, 4, 2, 64, ("composed",), max_pos=128, T=3, launches=([0, 63],)))
    assert len({x.id for x in c}) == len(c)
    return c


CASES = _cases()
