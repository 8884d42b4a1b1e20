"""CPU: the decision of prefix reuse, `plan_reuse(matched_rows, live_len, len_new, cap, max_new, state_max_new) -> (mode, L)` -- a
pure function (spatialrgpt_amd/reuse.py), driven over the table of cases the feature's description sets."""
import pytest

from spatialrgpt_amd.reuse import plan_reuse

# the last request left live_len = 215 cached rows (a 210-row prompt + 6 kept ids, the last one pending); cache of 400 positions
CASES = [
    # matched_rows, live_len, len_new, cap, max_new, state_max_new -> mode, L
    ("matched above live_len: the pending id's row is not cached", (216, 215, 223, 400, 8, 128), ("append", 215)),
    ("matched equal to live_len", (215, 215, 223, 400, 8, 128), ("append", 215)),
    ("matched below live_len: an id changed inside the cached rows", (204, 215, 223, 400, 8, 128), ("append", 204)),
    ("matched == len_new, the repeated request: one row is appended", (210, 215, 210, 400, 8, 128), ("append", 209)),
    ("matched == len_new == live_len + 1", (216, 215, 216, 400, 8, 128), ("append", 215)),
    ("nothing matched", (0, 215, 223, 400, 8, 128), ("fresh", 0)),
    ("a one-row prompt: len_new - 1 == 0", (1, 215, 1, 400, 8, 128), ("fresh", 0)),
    ("an empty retained state", (5, 0, 223, 400, 8, 128), ("fresh", 0)),
    ("capacity short by one position", (215, 215, 223, 230, 8, 128), ("fresh", 215)),
    ("capacity that fits exactly", (215, 215, 223, 231, 8, 128), ("append", 215)),
    ("max_new above the state's", (215, 215, 223, 400, 129, 128), ("fresh", 215)),
    ("max_new equal to the state's", (215, 215, 223, 400, 128, 128), ("append", 215)),
]


@pytest.mark.parametrize("what,args,want", CASES, ids=[c[0] for c in CASES])
def test_plan_reuse(what, args, want):
    assert plan_reuse(*args) == want, what


def test_plan_reuse_always_appends_a_row_and_never_overruns():
    for matched in range(0, 12):
        for live in range(0, 12):
            for len_new in range(1, 12):
                mode, L = plan_reuse(matched, live, len_new, 16, 4, 4)
                assert 0 <= L <= min(matched, live, len_new - 1)
                assert (mode == "append") == (L > 0 and len_new + 4 <= 16)
