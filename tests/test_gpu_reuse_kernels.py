"""The two kernels of prefix reuse (csrc/reuse.hip) against host loops, exact ints: srgpt_rows_match (leading byte-equal rows, any
alignment, any row width, a result that needs no initial value and touches one int) and srgpt_splice_match (leading rows of a splice
table that name the sources of the old row sequence: the old table, then the generated ids)."""
import pytest
import torch

from spatialrgpt_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD0, GUARD1, GARBAGE = 0x5A5A5A5A, -0x12345678, 0x7BADF00D


def _host_rows_match(a, b, rows):
    """a, b: CPU uint8 [rows, row_bytes]"""
    n = 0
    while n < rows and torch.equal(a[n], b[n]):
        n += 1
    return n


class _Pair:
    """two device byte buffers at chosen offsets from a 16-byte boundary, and the guarded output int"""

    def __init__(self, rows, row_bytes, off_a, off_b):
        self.rows, self.row_bytes, n = rows, row_bytes, max(rows, 1) * row_bytes
        self.store_a = torch.zeros((n + 64,), dtype=torch.uint8, device=DEV)
        self.store_b = torch.zeros((n + 64,), dtype=torch.uint8, device=DEV)
        assert self.store_a.data_ptr() % 16 == 0 and self.store_b.data_ptr() % 16 == 0
        self.a = self.store_a[off_a:off_a + n].view(max(rows, 1), row_bytes)
        self.b = self.store_b[off_b:off_b + n].view(max(rows, 1), row_bytes)
        assert self.a.data_ptr() % 16 == off_a and self.b.data_ptr() % 16 == off_b
        self.out = torch.tensor([GUARD0, GARBAGE, GUARD1], dtype=torch.int32, device=DEV)

    def run(self, a_cpu, b_cpu):
        self.a.copy_(a_cpu)
        self.b.copy_(b_cpu)
        self.out.copy_(torch.tensor([GUARD0, GARBAGE, GUARD1], dtype=torch.int32))  # garbage, not zero, in the result's place
        ops.rows_match(self.a, self.b, self.rows, self.out[1:2])
        g0, got, g1 = self.out.cpu().tolist()
        assert (g0, g1) == (GUARD0, GUARD1), "an int next to out[0] was written"
        return got


def _diff_cases(rows, rb):
    """(what, [flat byte positions that differ]) for a [rows, rb] buffer"""
    n = rows * rb
    cases = [("equal", []), ("first byte of the buffer", [0]), ("last byte of the buffer", [n - 1])]
    for r in sorted({0, rows - 1}):
        cases.append((f"row {r}, its middle", [r * rb + rb // 2]))
        for back in sorted({0, min(rb, 15) - 1}):  # inside the last, unaligned, 1 .. 15 bytes of the row only
            cases.append((f"row {r}, {back} bytes before its end", [(r + 1) * rb - 1 - back]))
    if rows >= 2:
        cases.append(("two differing rows: the first wins", [(rows - 1) * rb + rb // 3, (rows - 2) * rb + rb - 1]))
        cases.append(("first byte of the second row", [rb]))
    return cases


@pytest.mark.parametrize("row_bytes", [1, 15, 16, 17, 4096 + 3])
def test_rows_match_against_the_host_loop(row_bytes):
    g = torch.Generator().manual_seed(row_bytes)
    for rows in (0, 1, 3):
        base = torch.randint(0, 256, (max(rows, 1), row_bytes), dtype=torch.uint8, generator=g)
        for off_a in (0, 2, 6):
            for off_b in (0, 2, 6):
                p = _Pair(rows, row_bytes, off_a, off_b)
                if rows == 0:
                    assert p.run(base, base) == 0 and p.run(base, base ^ 255) == 0
                    continue
                for what, where in _diff_cases(rows, row_bytes):
                    other = base.clone()
                    for pos in where:
                        other.view(-1)[pos] ^= 0x40
                    want = _host_rows_match(base, other, rows)
                    assert want == (min(where) // row_bytes if where else rows)
                    got = p.run(base, other)
                    assert got == want, (what, rows, row_bytes, off_a, off_b, got, want)
                    assert p.run(other, base) == want, (what, "operands swapped")


@pytest.mark.parametrize("off_a,off_b", [(0, 0), (2, 6), (0, 2), (0, 1), (6, 0)])
def test_rows_match_over_many_blocks(off_a, off_b):
    """a media-sized compare: every unit width the alignments select (16, 4, 2, 1, 2 bytes) over more than one block"""
    rows, rb = 2, 300007
    g = torch.Generator().manual_seed(5)
    base = torch.randint(0, 256, (rows, rb), dtype=torch.uint8, generator=g)
    p = _Pair(rows, rb, off_a, off_b)
    for where in ([], [0], [rows * rb - 1], [rb - 1], [rb], [rb + 123457], [123457, rb + 5], [rb // 2, rb // 2 + 1, rb + 1]):
        other = base.clone()
        for pos in where:
            other.view(-1)[pos] ^= 1
        want = _host_rows_match(base, other, rows)
        assert p.run(base, other) == want, (where, off_a, off_b)


def test_rows_match_is_bytewise_on_floats():
    """-0.0 differs from 0.0, equal NaN bytes are equal; torch slices of a float tensor go in as they are"""
    x = torch.tensor([[0.0, 1.5, float("nan")], [2.0, -0.0, 3.0], [4.0, 5.0, 6.0]], device=DEV)
    y = x.clone()
    out = torch.full((1,), GARBAGE, dtype=torch.int32, device=DEV)
    assert int(ops.rows_match(x, y, 3, out)[0]) == 3  # NaN == NaN by bytes
    y[1, 1] = 0.0
    assert bool((x[1] == y[1]).all()) and int(ops.rows_match(x, y, 3, out)[0]) == 1  # equal as floats, not as bytes
    big = torch.arange(40, dtype=torch.bfloat16, device=DEV).reshape(8, 5)
    assert int(ops.rows_match(big[1:4], big.clone()[1:4], 3, out)[0]) == 3  # a slice 10 bytes past the allocation's boundary
    assert int(ops.rows_match(big[1:4], big[2:5], 3, out)[0]) == 0
    with pytest.raises(ValueError):
        ops.rows_match(big[1:4], big[2:4], 3, out)


# ------------------------------------------------------------------------------------------------ srgpt_splice_match
def _host_splice_match(desc_new, len_new, desc_old, n_old, gen, n_gen, nrc):
    n = 0
    for r in range(min(len_new, n_old + n_gen)):
        key = int(desc_new[r][0])
        old = int(desc_old[r][0]) if r < n_old else int(gen[r - n_old]) << 2
        kind, src = key & 3, key >> 2
        if key != old or (kind in (2, 3) and src >= nrc):
            break
        n += 1
    return n


def _run_splice_match(desc_new, len_new, desc_old, n_old, gen, n_gen, nrc):
    pad = torch.zeros((1, 2), dtype=torch.int32)
    dn = torch.cat([desc_new.reshape(-1, 2).to(torch.int32), pad]).to(DEV)  # never an empty tensor: the pointers must not be NULL
    do = torch.cat([desc_old.reshape(-1, 2).to(torch.int32), pad]).to(DEV)
    ge = torch.cat([gen.reshape(-1).to(torch.int64), torch.zeros((1,), dtype=torch.int64)]).to(DEV)
    out = torch.tensor([GUARD0, GARBAGE, GUARD1], dtype=torch.int32, device=DEV)
    ops.splice_match(dn, len_new, do, n_old, ge, n_gen, nrc, out[1:2])
    g0, got, g1 = out.cpu().tolist()
    assert (g0, g1) == (GUARD0, GUARD1)
    want = _host_splice_match(desc_new.reshape(-1, 2).tolist(), len_new, desc_old.reshape(-1, 2).tolist(), n_old, gen.tolist(), n_gen, nrc)
    assert got == want, (got, want, len_new, n_old, n_gen, nrc)
    return got


def _table(n, seed, regions=4):
    """a prompt's rows as the plan leaves them: text ids, a run of image rows, <mask> / <depth> pairs in order; the second int of a
    row (the prompt position) is set to something else in every copy"""
    g = torch.Generator().manual_seed(seed)
    keys = (torch.randint(0, 1000, (n,), generator=g) << 2)
    img0 = min(3, n)
    img1 = min(img0 + 196, n)
    keys[img0:img1] = 1 | (torch.arange(img1 - img0) << 2)
    for k in range(regions):
        r = img1 + 2 + 3 * k
        if r + 1 < n:
            keys[r] = 2 | (k << 2)
            keys[r + 1] = 3 | (k << 2)
    return keys.to(torch.int32)


def _desc(keys, second):
    return torch.stack([keys, torch.full_like(keys, second) + torch.arange(keys.numel(), dtype=torch.int32)], 1)


@pytest.mark.parametrize("len_new", [0, 1, 1023, 1024, 1025, 2049])
def test_splice_match_first_mismatch_at_the_edges_of_the_strided_loop(len_new):
    keys = _table(len_new, seed=len_new)
    for at in sorted({0, 1023, 1024, len_new - 1, None} - {-1}, key=lambda v: (v is None, v)):
        if at is not None and at >= len_new:
            continue
        old = keys.clone()
        if at is not None:
            old[at] += 4  # the same kind, the next source
        # the whole old sequence in desc_old; the second ints differ everywhere and are ignored
        got = _run_splice_match(_desc(keys, 7), len_new, _desc(old, -9000), len_new, torch.zeros(0, dtype=torch.int64), 0, 4)
        assert got == (len_new if at is None else at)
    # the old sequence shorter / longer than the new prompt
    if len_new > 1:
        assert _run_splice_match(_desc(keys, 7), len_new, _desc(keys[:len_new - 1], 0), len_new - 1, torch.zeros(0, dtype=torch.int64), 0, 4) == len_new - 1
    longer = torch.cat([keys, torch.tensor([8, 12], dtype=torch.int32)])
    assert _run_splice_match(_desc(keys, 7), len_new, _desc(longer, 0), len_new + 2, torch.zeros(0, dtype=torch.int64), 0, 4) == len_new


def test_splice_match_across_the_boundary_between_the_old_table_and_the_generated_ids():
    n_old, n_gen = 1020, 9
    keys = _table(n_old + n_gen + 6, seed=3)
    gen = (keys[n_old:n_old + n_gen] >> 2).to(torch.int64)  # text rows: kind 0, src = the id
    assert bool(((keys[n_old:] & 3) == 0).all())
    new, old = _desc(keys, 1), _desc(keys[:n_old], -5)
    assert _run_splice_match(new, keys.numel(), old, n_old, gen, n_gen, 4) == n_old + n_gen  # a match across it, to the end of OLD
    assert _run_splice_match(new, n_old + 4, old, n_old, gen, n_gen, 4) == n_old + 4          # ... to the end of NEW
    g2 = gen.clone()
    g2[0] += 1
    assert _run_splice_match(new, keys.numel(), old, n_old, g2, n_gen, 4) == n_old            # the first generated row differs
    g2 = gen.clone()
    g2[n_gen - 1] += 1
    assert _run_splice_match(new, keys.numel(), old, n_old, g2, n_gen, 4) == n_old + n_gen - 1
    for kind in (1, 2, 3):  # a new row of another kind whose src IS the generated id: a generated row is a text row
        k2 = keys.clone()
        k2[n_old + 2] = kind | (int(gen[2]) << 2)
        assert _run_splice_match(_desc(k2, 1), keys.numel(), old, n_old, gen, n_gen, 1 << 20) == n_old + 2
    assert _run_splice_match(new, keys.numel(), old, n_old, gen, 0, 4) == n_old               # n_gen_old = 0
    assert _run_splice_match(new, keys.numel(), old, 0, (keys >> 2).to(torch.int64), 3, 4) == 3   # n_old_rows = 0: ids only
    assert _run_splice_match(new, keys.numel(), old, 0, gen, 0, 4) == 0                       # nothing old at all
    big = torch.tensor([1 << 40], dtype=torch.int64)  # an id beyond the descriptor's bits equals no key (its low bits are key 0's)
    assert _run_splice_match(_desc(torch.zeros(1, dtype=torch.int32), 0), 1, old, 0, big, 1, 4) == 0


def test_splice_match_region_rows_beyond_the_common_regions_do_not_match():
    keys = _table(260, seed=11, regions=4)
    new, old = _desc(keys, 0), _desc(keys, 100)
    first = {k: int(((keys & 3) == 2).logical_and((keys >> 2) == k).nonzero()[0]) for k in range(4)}
    assert _run_splice_match(new, 260, old, 260, torch.zeros(0, dtype=torch.int64), 0, 4) == 260  # src = n_regions_common - 1 matches
    for nrc in (3, 2, 1, 0):
        assert _run_splice_match(new, 260, old, 260, torch.zeros(0, dtype=torch.int64), 0, nrc) == first[nrc]  # src = n_regions_common
    # a <depth> row alone beyond the common regions (its <mask> row is text here)
    k2 = keys.clone()
    k2[first[2]] = 77 << 2
    assert _run_splice_match(_desc(k2, 0), 260, _desc(k2, 5), 260, torch.zeros(0, dtype=torch.int64), 0, 2) == first[2] + 1
