"""The Philox address of a row of a sampler launch over B sequences x T steps, and the counter rule that goes with it
(spatialrgpt_amd/csrc/draw_addr.h), on the CPU through tests/draw_addr_cli.cpp -- the header compiled alone, no HIP.  The plain sampled
batched loop draws generated id i of sequence b at (c0 + i, b); the batched sampled lookup step has one counter for sequences that
have emitted different numbers of ids, and these tests show that the rule gives every row exactly that address."""
import random
import subprocess

import pytest

from tests.util import _build_route_cli


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    exe = _build_route_cli(tmp_path_factory.mktemp("draw_addr"), "draw_addr_cli")

    def ask(lines):
        out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out

    return ask


def addr_line(counter, T, steps):
    return f"addr {counter} {len(steps)} {T} " + " ".join(map(str, steps))


def parse_addr(line):
    m, *rows = line.split(" | ")
    return int(m), [tuple(map(int, r.split())) for r in rows]


def test_random_walks_read_the_plain_loops_addresses(cli):
    """B rows emit 1 .. T ids per step and freeze at max_new: id i of row b was addressed at (c0 + i, b), counter == c0 + m throughout"""
    rng = random.Random(20240611)
    lines, checks = [], []
    for walk in range(200):
        B, T, max_new = rng.randint(1, 8), rng.randint(1, 6), rng.randint(2, 40)
        c0 = rng.choice([0, 7, 2 ** 32 - 3, 2 ** 40 + 5, rng.getrandbits(60)])
        steps = [1] * B  # behind the first pick: every row has emitted one id and the counter is c0 + 1
        while min(steps) < max_new:
            m = min(steps)
            emit = [0 if s >= max_new else min(rng.randint(1, T), max_new - s) for s in steps]
            after = [s + e for s, e in zip(steps, emit)]
            lines.append(addr_line(c0 + m, T, steps))
            checks.append(("addr", c0, T, list(steps), emit))
            lines.append(f"adv {B} " + " ".join(map(str, steps)) + " " + " ".join(map(str, after)))
            checks.append(("adv", min(after) - m))
            steps = after
        # every row frozen: the counter stays
        lines.append(f"adv {B} " + " ".join(map(str, steps)) + " " + " ".join(map(str, steps)))
        checks.append(("adv", 0))
    seen_apart = False
    for line, chk in zip(cli(lines), checks):
        if chk[0] == "adv":
            assert int(line) == chk[1]  # by induction the counter is c0 + m before every step
            continue
        _, c0, T, steps, emit = chk
        m, rows = parse_addr(line)
        assert m == min(steps)
        seen_apart = seen_apart or len(set(steps)) > 1
        for b, s in enumerate(steps):
            for t in range(emit[b]):  # the rows whose draws become ids s + t of row b
                assert rows[b * T + t] == ((c0 + s + t) % 2 ** 64, b), (c0, steps, b, t)
    assert seen_apart  # the walks did let rows run apart


def test_one_sequence_is_the_rows_are_steps_address(cli):
    """B = 1: (counter + t, 0) whatever the count, and the advance is the ids emitted"""
    lines = [addr_line(c, T, [s]) for c in (0, 5, 2 ** 32 - 1, 2 ** 63) for T in (1, 2, 4, 16) for s in (0, 1, 9, 1000)]
    want = [[((c + t) % 2 ** 64, 0) for t in range(T)] for c in (0, 5, 2 ** 32 - 1, 2 ** 63) for T in (1, 2, 4, 16) for s in (0, 1, 9, 1000)]
    assert [parse_addr(ln)[1] for ln in cli(lines)] == want
    assert cli(["adv 1 3 7", "adv 1 1 2", "adv 1 40 40"]) == ["4", "1", "0"]


def test_one_step_and_equal_counts_is_the_sequences_address(cli):
    """T = 1 and equal steps[]: (counter, b), and a step in which every row emits one id advances the counter by one"""
    lines = [addr_line(c, 1, [s] * B) for c in (0, 11, 2 ** 32 - 1) for B in (1, 2, 5, 8, 16) for s in (0, 1, 77)]
    want = [[(c, b) for b in range(B)] for c in (0, 11, 2 ** 32 - 1) for B in (1, 2, 5, 8, 16) for s in (0, 1, 77)]
    assert [parse_addr(ln)[1] for ln in cli(lines)] == want
    assert cli(["adv 4 5 5 5 5 6 6 6 6"]) == ["1"]


def test_the_sum_carries_into_the_high_word(cli):
    c0 = 2 ** 32 - 2
    m, rows = parse_addr(cli([addr_line(c0, 4, [3, 1])])[0])
    assert m == 1
    assert rows == [(c0 + 2, 0), (c0 + 3, 0), (c0 + 4, 0), (c0 + 5, 0), (c0, 1), (c0 + 1, 1), (c0 + 2, 1), (c0 + 3, 1)]
    assert rows[0][0] == 2 ** 32 and rows[5][0] == 2 ** 32 - 1  # rows on both sides of the carry
    assert all(ctr >> 32 == (1 if ctr >= 2 ** 32 else 0) for ctr, _ in rows)


def test_negative_counts_clamp_to_zero(cli):
    m, rows = parse_addr(cli([addr_line(10, 2, [-3, 2, 0])])[0])
    assert m == 0
    assert rows == [(10, 0), (11, 0), (12, 1), (13, 1), (10, 2), (11, 2)]
    m, rows = parse_addr(cli([addr_line(10, 2, [-3, -1])])[0])
    assert m == 0 and rows == [(10, 0), (11, 0), (10, 1), (11, 1)]
    assert cli(["adv 2 -3 2 1 2", "adv 2 -3 -1 -3 -1"]) == ["1", "0"]
