"""CPU: the census data of tests/attn_census.py can tell a wrong key selection from the right one.  For every case of
tests/test_gpu_attention_census.py the float64 reference is compared with MUTANT references -- the rule of include/srgpt.h broken in
one of ten ways (attn_census.MUTANTS) -- and every mutant that changes which keys a launch weighs has to move at least one element,
in at least one of the three query families, by 8 times the tolerance the GPU test allows.  A case whose data cannot tell a mutant
apart fails here, and the data is fixed, not the mutant list; every case keeps mutants 1 to 5 except where no data of its shape could
show one (Case.inapplicable, with the reason beside it).  The census decoder is run on the mutants too: it has to name the keys."""
import math
import os

import pytest
import torch

from tests import attn_census as ac

CASE_IDS = [c.id for c in ac.CASES]


@pytest.mark.parametrize("case", ac.CASES, ids=CASE_IDS)
def test_every_applicable_mutant_is_told_apart(case):
    fams = {f: case.problems(f) for f in ac.FAMILIES}
    n_launch = len(fams["uniform"])
    applied, smallest = set(), {}
    for i in range(n_launch):
        refs = {f: ac.reference(fams[f][i]) for f in ac.FAMILIES}
        for mu in ac.MUTANTS:
            if not ac.applies(fams["uniform"][i], mu):
                continue  # skipped by name: the report below lists what applied
            applied.add(mu)
            mg = max(ac.margin(fams[f][i], mu, case.dtype, refs[f]) for f in ac.FAMILIES)
            assert mg >= ac.MARGIN, f"{case.id}, launch {i} ({fams['uniform'][i].what}): mutant {mu} ({ac.MUTANTS[mu]}) moves no element " \
                                    f"by more than {mg:.3g} tolerances"
            smallest[mu] = min(mg, smallest.get(mu, math.inf))
    assert {1, 2, 3, 4, 5} - applied == set(case.inapplicable), (case.id, sorted(applied), case.inapplicable)
    # mutants 6 .. 10 where the case has what they need
    if case.id.endswith("-cut") or case.entry == "attention" and case.kv_len is not None and min(case.kv_len) < case.Tk:
        assert 6 in applied, case.id
        if len(set(min(n, case.Tk) for n in case.kv_len)) > 1:
            assert 7 in applied, case.id
    if case.entry != "attention" and any(len(set(pos)) > 1 for pos in (case.launches or [case.q_pos0])):
        assert 8 in applied, case.id
    if case.Hkv > 1 and case.Hq > case.Hkv:
        assert 9 in applied, case.id
    if case.B > 1 or any(len(pos) > 1 for pos in case.launches):
        assert 10 in applied, case.id
    log = os.environ.get("SRGPT_CENSUS_MARGINS")  # the table of profiles/attention_census.txt
    if log:
        with open(log, "a") as f:
            f.write("%-34s %s\n" % (case.id, "  ".join("%d:%.3g" % (mu, smallest[mu]) for mu in sorted(smallest))))


def test_the_amplitude_is_exact_in_bf16_and_64_nats_clear():
    for D, a in ((128, 32), (72, 32), (64, 32), (32, 32), (20, 32), (16, 16)):
        assert ac.amplitude(D) == a and a * a / math.sqrt(D) >= 64 and (a / 2) ** 2 / math.sqrt(D) < 64
        assert float(torch.tensor(float(a)).to(torch.bfloat16)) == a
    assert math.exp(-64.0) < 2.0 ** -90


def test_codes_are_unique_and_differ_by_head_and_row():
    for D, n in ((128, 4096), (72, 200), (64, 1024), (32, 256), (20, 100), (16, 64)):
        v = ac.v_codes(2, n, 2, D)
        assert bool((v.sum(-1) == 2).all()) and set(v.unique().tolist()) == {0.0, 1.0}
        for b in range(2):
            for hk in range(2):
                assert len({tuple(r.nonzero().flatten().tolist()) for r in v[b, :, hk]}) == n
        assert not torch.equal(v[0, :, 0], v[0, :, 1]) and not torch.equal(v[0, :, 0], v[1, :, 0])
        # rows 0 and 1 at one kv head apart, and kv heads 0 and 1 one row apart, do coincide by construction: hk + b is the rotation


def test_every_stored_value_is_exact_in_the_case_dtype():
    for case in ac.CASES:
        p = case.problems("lit_next")[0]
        for t in (p.q, p.k, p.v) + ((p.qkv, p.kc0, p.vc0) if p.qkv is not None else ()):
            assert torch.equal(t.to(case.dtype).float(), t), case.id


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("lens", [None, [37, 5, 0]])
def test_reference_is_the_ragged_tests_formula_on_random_data(causal, lens):
    """attn_census.reference against `_attn_ref64` of tests/test_gpu_attention_ragged.py: the same operation"""
    from tests.test_gpu_attention_ragged import _attn_ref64
    B, Tq, Tk, Hq, Hkv, D = 3, 29, 37, 4, 2, 24
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(s, generator=g) for s in ((B, Tq, Hq, D), (B, Tk, Hkv, D), (B, Tk, Hkv, D)))
    p = ac.Problem(q, k, v, [Tk - Tq] * B if causal else None, lens, Tk, 1.0 / math.sqrt(D))
    want, vis = _attn_ref64(q, k, v, causal, lens)
    got = ac.reference(p)
    assert float((got - want).abs().max()) < 1e-13
    assert torch.equal(ac.multiplicity(p).any(-1), vis)


@pytest.mark.parametrize("case_id,mutant,words", [
    ("flash128-causal-65x130-nolen", 1, "extra"),
    ("flash128-causal-65x130-nolen", 2, "missing"),
    ("flash128-full-129", 5, "counted twice"),
    ("decode-mfma-G4-384", 1, "a lure"),
    ("decode-valu-f32-G4-B2", 4, "key 0 missing"),
    ("multi-mfma-G4-T4", 1, "extra"),
])
def test_the_decoder_names_the_keys(case_id, mutant, words):
    """a mutant reference handed to the census check as if a kernel had returned it"""
    case = next(c for c in ac.CASES if c.id == case_id)
    p = case.problems("uniform")[-1]
    assert ac.census_error(ac.reference(p).to(case.dtype), p, case.dtype) is None
    msg = ac.census_error(ac.reference(p, mutant).to(case.dtype), p, case.dtype)
    assert msg is not None and words in msg and "census of row" in msg, msg
