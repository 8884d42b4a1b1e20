"""CPU: generation.StopJudge, the one stop rule behind the engine's decode loops (plain and lookup steps), against a serial
reference written here in HF's order -- after each whole column: EOS ids, "all rows finished?", then the stopping criteria.

The ids are seeded random matrices over a vocabulary of 8, so EOS ids and the criteria's trigger ids occur often.  They are
delivered the two ways the engine delivers them: one column per feed (plain steps), and 1 .. 5 new ids per row and feed, rows
apart from each other (lookup steps).  What a row has NOT emitted yet is poisoned with the id the criteria fire on, so a judge
that looks at a column before its slowest row reached it stops early.  Every case compares n_keep, rows(n_keep) and the exact
sequence of (criterion index, ids.shape) calls."""
import random

import pytest
import torch

from spatialrgpt_amd.generation import StopJudge

VOCAB, TRIG, TRIG2 = 8, 5, 2
EOS = {"none": None, "int": 3, "two": [3, 6], "empty": []}
SEEDS = range(6)


class _Rec:
    """a criterion that logs its calls; `fn(new column [B]) -> bool | bool tensor [B]` sees only the LAST column, as a criterion
    with state does (the demo's KeywordsStoppingCriteria): a column skipped or handed over twice changes its verdict"""

    def __init__(self, index, fn, log):
        self.index, self.fn, self.log = index, fn, log

    def __call__(self, ids, scores):
        assert scores is None
        self.log.append((self.index, tuple(ids.shape)))
        return self.fn(ids[:, -1])


def _criteria(kind, B, log):
    if kind == "none":
        return None
    if kind == "any":  # fires when TRIG first appears in any row
        return [_Rec(0, lambda col: bool((col == TRIG).any()), log)]
    if kind == "tensor":  # a [B] bool tensor: the rows that have shown TRIG so far
        hit = torch.zeros((B,), dtype=torch.bool)

        def rows(col):
            hit.logical_or_(col == TRIG)
            return hit.clone()
        return [_Rec(0, rows, log)]
    if kind == "two":  # the first fires on TRIG: the second (which fires on TRIG2) must not be called for that column
        return [_Rec(0, lambda col: bool((col == TRIG).any()), log), _Rec(1, lambda col: bool((col == TRIG2).any()), log)]
    raise ValueError(kind)


def _truthy(r):
    return bool(r.all()) if isinstance(r, torch.Tensor) else bool(r)


def _reference(ids, eos, kind, max_new):
    """the serial loop: column by column, EOS -> all rows finished? -> criteria"""
    B, log = ids.shape[0], []
    eos = ([eos] if isinstance(eos, int) else list(eos)) if eos is not None else []
    crits = _criteria(kind, B, log) or []
    first, n_keep = [None] * B, max_new
    for c in range(max_new):
        for b in range(B):
            if first[b] is None and int(ids[b, c]) in eos:
                first[b] = c + 1
        if eos and all(f is not None for f in first):
            n_keep = c + 1
            break
        if any(_truthy(crit(ids[:, :c + 1], None)) for crit in crits):  # any() stops at the first that fires
            n_keep = c + 1
            break
    return n_keep, [n_keep if f is None else min(f, n_keep) for f in first], log


def _deliver(ids, have):
    """the buffer the loop reads after the device emitted have[b] ids of row b: the rest is poison"""
    buf = torch.full_like(ids, TRIG)
    for b, n in enumerate(have):
        buf[b, :n] = ids[b, :n]
    return buf


def _run(ids, eos, kind, max_new, style, rng):
    B, log = ids.shape[0], []
    judge = StopJudge(B, eos, _criteria(kind, B, log), max_new)
    have = [1] * B
    for t in range(max_new + 1):
        if style == "plain":
            have = [t + 1] * B
        elif t:
            have = [min(n + rng.randint(1, 5), max_new) for n in have]
        n_keep = judge.feed(_deliver(ids, have), have)
        if n_keep is not None:
            return n_keep, judge.rows(n_keep), log
    raise AssertionError("the judge did not end a request whose rows all hold max_new_tokens ids")


def _ids(B, cols, seed, exclude=()):
    g = torch.Generator().manual_seed(1000 * B + 10 * cols + seed)
    pool = torch.tensor([v for v in range(VOCAB) if v not in exclude])
    return pool[torch.randint(0, len(pool), (B, cols), generator=g)]


@pytest.mark.parametrize("style", ["plain", "lookup"])
@pytest.mark.parametrize("kind", ["none", "any", "tensor", "two"])
@pytest.mark.parametrize("eos", list(EOS))
@pytest.mark.parametrize("B", [1, 2, 4])
def test_judge_matches_the_serial_loop(B, eos, kind, style):
    for seed in SEEDS:
        max_new = 12 + 2 * seed + (seed % 2)  # 12 .. 23 columns
        ids = _ids(B, max_new, seed)
        rng = random.Random(seed)
        assert _run(ids, EOS[eos], kind, max_new, style, rng) == _reference(ids, EOS[eos], kind, max_new), (seed, ids)


@pytest.mark.parametrize("style", ["plain", "lookup"])
@pytest.mark.parametrize("B", [1, 2, 4])
def test_a_request_nothing_stops_runs_to_max_new_tokens(B, style):
    max_new = 17
    ids = _ids(B, max_new, 0, exclude=(3, 6, TRIG, TRIG2))  # neither an EOS id nor a trigger occurs
    for eos, kind in (("none", "none"), ("two", "two"), ("int", "tensor")):
        got = _run(ids, EOS[eos], kind, max_new, style, random.Random(B))
        assert got == _reference(ids, EOS[eos], kind, max_new)
        assert got[0] == max_new and got[1] == [max_new] * B
        assert [c[1] for c in got[2] if c[0] == 0] == ([] if kind == "none" else [(B, c + 1) for c in range(max_new)])


@pytest.mark.parametrize("style", ["plain", "lookup"])
@pytest.mark.parametrize("kind", ["none", "two"])
def test_a_second_eos_behind_a_rows_first_changes_nothing(kind, style):
    ids = torch.tensor([[0, 1, 3, 1, 6, 0, 3, 1, 0, 1, 0, 1],
                        [1, 0, 1, 0, 1, 0, 1, 6, 3, 0, 1, 0]])
    for seed in SEEDS:
        got = _run(ids, [3, 6], kind, 12, style, random.Random(seed))
        assert got == _reference(ids, [3, 6], kind, 12)
        assert got[0] == 8 and got[1] == [3, 8]
        # the closing column's EOS is judged before its criteria: seven columns were handed over, not eight
        assert got[2] == ([] if kind == "none" else [(i, (2, c + 1)) for c in range(7) for i in (0, 1)])


def test_eos_forms_and_can_stop():
    for given, want in ((None, None), (3, [3]), ([3, 6], [3, 6]), ((6, 3), [6, 3]), ({3}, [3]), ([], None), ((), None)):
        judge = StopJudge(2, given, None, 4)
        assert judge.eos == want and judge.can_stop == (want is not None)
    assert not StopJudge(1, None, [], 4).can_stop
    assert StopJudge(1, None, [lambda ids, scores: False], 4).can_stop
