"""CPU: the host restatement of the draw (tests/draw_ref.py) proved on its own -- Random123's known answers for Philox4x32-10, the
address rules against each other, the planted edge addresses, the share of cases the reference can judge without ambiguity, and
every mutant of the rule caught by a case the GPU file runs."""
import collections
import functools

import numpy as np
import pytest

from tests import draw_ref as R


def test_philox_known_answers():
    kat = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((R.M32,) * 4, (R.M32,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
    for ctr, key, want in kat:
        assert " ".join("%08x" % int(w) for w in R.philox4x32_10(*ctr, *key)) == want
    # arrays broadcast: the three vectors in one call
    cols = [np.array(c, dtype=np.uint64) for c in zip(*[c + k for c, k, _ in kat])]
    out = np.stack(R.philox4x32_10(*cols), axis=1)
    assert [" ".join("%08x" % int(w) for w in row) for row in out] == [w for _, _, w in kat]


def test_the_third_address_rule_contains_the_first_two():
    for counter in (0, 5, 2 ** 32 - 2, 2 ** 64 - 2):
        for s in (-4, 0, 3, 70000):   # B = 1: rows that are steps, whatever the count
            for t in range(4):
                assert R.addr_seq_steps(counter, [s], 4, 0, t) == R.addr_steps(counter, t)
        for steps in ([3, 3, 3], [0, -2, 0]):   # T = 1 and equal counts: rows that are sequences
            for b in range(3):
                assert R.addr_seq_steps(counter, steps, 1, b, 0) == R.addr_seqs(counter, b)
    assert R.addr_steps(2 ** 32 - 1, 1) == (2 ** 32, 0) and R.addr_steps(2 ** 64 - 1, 1) == (0, 0)   # the carry, and the wrap
    assert R.addr_seq_steps(10, [5, 2], 3, 0, 2) == (15, 0) and R.addr_seq_steps(10, [-3, 2], 3, 1, 1) == (13, 1)


def test_the_edge_addresses():
    for ctr, hit in R.EDGE_GUMBEL:
        n = R.gumbel_n(1, ctr, 0, hit)
        assert int(n) == 0xFFFFFF
        assert float(R.gumbel_u(n, {"u_one"})) == 1.0            # (n + 0.5) rounds to 2^24 in fp32 ...
        assert float(R.gumbel_u(n)) == 1.0 - 2.0 ** -24          # ... and the rule keeps u below 1
    assert R.icdf_n(1, R.EDGE_ICDF_LAST, 0) == 0xFFFFFF and R.icdf_n(1, R.EDGE_ICDF_ZERO, 0) == 0
    assert min(R.EDGE_ICDF_LAST, R.EDGE_ICDF_ZERO) >= 2 ** 32   # the counter's high word is live
    for ctr, j in R.EDGE_WALK_EXACT:
        assert R.icdf_n(1, ctr, 0) == j << 18 and ctr >= 2 ** 32
    n = np.arange(2 ** 24, dtype=np.uint64)                      # every one of the 2^24 uniforms lies inside (0, 1)
    u = R.gumbel_u(n)
    assert u.dtype == np.float32 and float(u.min()) == 2.0 ** -25 and float(u.max()) == 1.0 - 2.0 ** -24
    assert int((R.gumbel_u(n, {"u_one"}) != u).sum()) == 1      # the clamp changes one value of u and no other


@functools.lru_cache(maxsize=None)
def _cases():
    """every row the GPU file draws -> (group, name, which, setting, logits row, seed, ctr, seq, t, reference)"""
    out = []
    for c in R.chains():
        for i in range(c["calls"]):
            for b, row in enumerate(c["rows"]):
                ctr, seq = R.addr_seqs((c["counter"] + i) & R.M64, b)
                ref = R.ref_chain_row(c["which"], c["setting"], c["V"], row, c["seed"], ctr, seq)
                out.append(((c["which"], c["setting"]), "chain-row%d" % row, c["which"], c["setting"], R.case_logits(c["V"])[row], c["seed"],
                            ctr, seq, 0, ref))
    for mode, which, setting, row, seed, ctr, seq, t in R.mode_rows():
        out.append(((which, setting), mode, which, setting, row, seed, ctr, seq, t, R.ref_draw(which, row, setting, seed, ctr, seq)))
    for name, which, setting, row, ctr in R.edge_rows():
        out.append(("edge", name, which, setting, row, 1, ctr, 0, 0, R.ref_draw(which, row, setting, 1, ctr, 0)))
    return out


def test_the_reference_judges_nearly_every_case():
    total, clear = collections.Counter(), collections.Counter()
    for group, *_, ref in _cases():
        total[group] += 1
        clear[group] += not ref.ambiguous
    assert set(total) == {(w, s) for w, ss in R.SETTINGS.items() for s in ss} | {"edge"}
    for V in R.VOCABS:
        assert {(c["which"], c["setting"]) for c in R.chains() if c["V"] == V} == set(total) - {"edge"}   # every V under every setting
    for group in total:
        share = clear[group] / total[group]
        print(group, total[group], "rows, non-ambiguous share %.4f" % share)
        assert share >= (1.0 if group == "edge" else 0.98), (group, share)


def test_the_planted_edges_draw_what_they_are_planted_for():
    seen = collections.Counter()
    for group, name, which, setting, row, seed, ctr, seq, t, ref in _cases():
        if group != "edge":
            continue
        seen[name] += 1
        if name == "walk_zero":
            assert ref.n == 0 and ref.rank == 0
        elif name == "walk_last":
            assert ref.n == 0xFFFFFF and ref.rank == len(ref.kept) - 1 > 0
        elif name == "walk_exact":
            assert ref.d == 0.0 and len(ref.kept) == 64 and ref.rank == ref.n >> 18
        elif name == "gumbel_ones":
            hit = dict(R.EDGE_GUMBEL)[ctr]
            assert ref.tok != hit and float(row[hit]) == float(row.max()) - R.EDGE_BELOW
            assert bool(ref.kept[hit]) == (setting[1] == 0)     # kept with everything kept, outside the top 64
        elif name == "no_half":
            assert ref.tok == R.no_half_row()[1] and ref.margin > 100 * ref.d
    assert seen == {"walk_zero": 2, "walk_last": 2, "walk_exact": 3, "gumbel_ones": 9, "no_half": 2}


# which cases can see a mutant at all
SEES = {
    "word_y": lambda c: True,
    "seq_dropped": lambda c: c["seq"] != 0,
    "icdf_word_0": lambda c: c["ref"].kind == "icdf",
    "ctr_hi_dropped": lambda c: c["ctr"] >= 2 ** 32,
    "seed_hi_dropped": lambda c: c["seed"] >= 2 ** 32,
    "nine_rounds": lambda c: True,
    "gumbel_no_half": lambda c: c["name"] == "no_half",
    "walk_le": lambda c: c["name"] == "walk_exact",
    "ties_ascending": lambda c: c["ref"].kind == "icdf" and c["name"] in ("chain-row%d" % R.ROW_TIES, "steps", "seq_steps"),
    "walk_before_top_p": lambda c: c["ref"].kind == "icdf" and c["setting"][2] is not None,
    "steps_t_in_seq": lambda c: c["name"] == "steps" and c["t"] > 0,
    "u_one": lambda c: c["name"] == "gumbel_ones" and c["setting"][1] == 0,
}


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_every_mutant_is_caught(mutant):
    """a wrong reference draws, in at least one non-ambiguous case that can see it, a token the rule does not draw"""
    assert set(SEES) == set(R.MUTANTS) and len(R.MUTANTS) >= 10
    mut = frozenset({mutant})
    saw = caught = 0
    for group, name, which, setting, row, seed, ctr, seq, t, ref in _cases():
        c = dict(name=name, setting=setting, seed=seed, ctr=ctr, seq=seq, t=t, ref=ref)
        if ref.ambiguous or not SEES[mutant](c):
            continue
        saw += 1
        if mutant == "steps_t_in_seq":
            ctr, seq = R.addr_steps(ctr - t, t, mut)   # the launch's counter is the row's less t
        caught += R.ref_draw(which, row, setting, seed, ctr, seq, mut).tok not in ref.ok
        if caught >= 3 or saw >= 60:
            break
    print(f"{mutant} ({R.MUTANTS[mutant]}): caught in {caught} of the first {saw} cases that can see it")
    assert caught >= 1, (mutant, saw)
    if mutant in ("u_one", "walk_le", "gumbel_no_half", "steps_t_in_seq"):
        assert caught == min(saw, 3), (mutant, caught, saw)   # planted for it: every one of them catches it
