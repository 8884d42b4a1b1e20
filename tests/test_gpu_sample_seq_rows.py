"""GPU: the samplers' sequences-x-steps mode (srgpt_sample_seq_rows, srgpt_sample_full_seq_rows: csrc/sample.hip, pick_draw in
csrc/pick.h over csrc/draw_addr.h).  The rows of a launch are B sequences x T successive steps, row b * T + t; sequence b has emitted
steps[b] ids, m = min max(steps, 0), and row (b, t) reads the Philox stream at (counter + max(steps[b], 0) - m + t, b).  The contract
is an identity, so the reference is the library's own B-row entry point (ops.sample / ops.sample_full) called at that counter with
the row's logits in row b: ids and kept sets must be EQUAL (torch.equal), and the counter behind the new call is unchanged.  With
T = 1 and equal counts the call is srgpt_sample / srgpt_sample_full, with B = 1 it is srgpt_sample_rows / srgpt_sample_full_rows.
The B-mode entry points are held to tests/golden/pick_kat.npz in the same process afterwards.

Shapes: V = 2048 (one 16-entry slice per block) and 3002 (slices of 24, a ragged last one of 2); the logits sit between NaN rows and
the ids between sentinel rows (tests/test_gpu_sample_rows.py's data and settings)."""
import os

import numpy as np
import pytest
import torch

from tests import pick_kat
from tests.test_gpu_sample_rows import FULL, SENT, TEMPERATURE, TOPK64, _counter, _logits
from tests.util import GOLD

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (B, T, steps): unequal counts everywhere; one entry at 0, one negative (it counts as 0)
CASES = ((2, 4, (3, 1)), (4, 4, (5, 0, 2, 9)), (3, 2, (4, -2, 6)), (8, 2, (1, 3, 2, 7, 1, 4, 9, 2)))


def _seq_rows_against_b_row_calls(B, T, steps, V, full, top_k, top_p, c0, seed):
    from spatialrgpt_amd import ops

    R = B * T
    big, lg, _ = _logits(R, V, top_k if top_k else 10, seed)
    st = torch.tensor(steps, dtype=torch.int32, device=DEV)
    filled = [max(s, 0) for s in steps]
    m = min(filled)
    # ---- the B-row entry at every counter a row reads: the rows that read it sit in their sequence's row (row 0's logits elsewhere:
    # a row of equal scores would be one tie group, which the top-k-64 sampler reports)
    at = {}
    for b in range(B):
        for t in range(T):
            at.setdefault(c0 + filled[b] - m + t, []).append((b, t))
    ids = torch.full((R,), -1, dtype=torch.int64, device=DEV)
    kept = [None] * R
    for ctr, rows in sorted(at.items()):
        x = lg[:1].repeat(B, 1)
        for b, t in rows:
            x[b] = lg[b * T + t]
        ref = ops.SamplingParams(DEV, B, keep_kept_sets=True).set(TEMPERATURE, top_k, top_p, seed=seed, counter=ctr % 2 ** 64)
        if full:
            i, mask = ops.sample_full(x, ref, kept_mask=True)
        else:
            i, mask = ops.sample(x, ref, check=True), ref.kept
        for b, t in rows:
            ids[b * T + t] = i[b]
            kept[b * T + t] = mask[b].clone()
    kept = torch.stack(kept)
    # ---- one sequences-x-steps call, the ids between sentinel rows
    out = torch.full((3, R), SENT, dtype=torch.int64, device=DEV)
    sp = ops.SamplingParams(DEV, R, keep_kept_sets=True).set(TEMPERATURE, top_k, top_p, seed=seed, counter=c0)
    before = sp.buf.clone()
    if full:
        got, got_kept = ops.sample_full_seq_rows(lg, sp, st, T, kept_mask=True, out=out[1])
    else:
        got, got_kept = ops.sample_seq_rows(lg, sp, st, T, check=True, out=out[1]), sp.kept
    torch.cuda.synchronize()
    what = (B, T, steps, V, full, top_k, top_p, c0)
    assert torch.equal(got, ids), (what, got.tolist(), ids.tolist())
    assert torch.equal(got_kept, kept), what
    assert torch.equal(sp.buf, before) and int(_counter(sp)) == (c0 if c0 < 2 ** 63 else c0 - 2 ** 64), what  # the block is only read
    assert st.tolist() == list(steps)
    assert bool((out[0] == SENT).all()) and bool((out[2] == SENT).all()) and bool(((got >= 0) & (got < V)).all()), what
    assert bool(big[0].isnan().all()) and bool(big[R + 1].isnan().all())
    return got


@pytest.mark.parametrize("V", (2048, 3002))
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[0]}T{c[1]}")
def test_rows_equal_the_b_row_entries_at_the_computed_counter(case, V):
    B, T, steps = case
    drew = []
    for si, (top_k, top_p) in enumerate(TOPK64):
        drew.append(_seq_rows_against_b_row_calls(B, T, steps, V, False, top_k, top_p, c0=3, seed=100 * B + T + si))
    for si, (top_k, top_p) in enumerate(FULL):
        drew.append(_seq_rows_against_b_row_calls(B, T, steps, V, True, top_k, top_p, c0=3, seed=200 * B + T + si))
    assert any(len(set(d.tolist())) > 1 for d in drew)  # the rows really are different draws


def test_one_step_and_equal_counts_is_the_sequences_entry():
    """T = 1, equal steps: ids and kept sets of srgpt_sample / srgpt_sample_full on the same logits at the same counter"""
    from spatialrgpt_amd import ops

    for V in (2048, 3002):
        for B, s in ((1, 0), (4, 1), (8, 6)):
            st = torch.full((B,), s, dtype=torch.int32, device=DEV)
            for si, (full, top_k, top_p) in enumerate([(False, *x) for x in TOPK64] + [(True, *x) for x in FULL]):
                _, lg, _ = _logits(B, V, top_k if top_k else 10, 31 * B + si)
                a = ops.SamplingParams(DEV, B, keep_kept_sets=True).set(TEMPERATURE, top_k, top_p, seed=5 + si, counter=11)
                b = ops.SamplingParams(DEV, B, keep_kept_sets=True).set(TEMPERATURE, top_k, top_p, seed=5 + si, counter=11)
                if full:
                    want, got = ops.sample_full(lg, a, kept_mask=True), ops.sample_full_seq_rows(lg, b, st, 1, kept_mask=True)
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (V, B, top_k, top_p)
                else:
                    want, got = ops.sample(lg, a, check=True), ops.sample_seq_rows(lg, b, st, 1, check=True)
                    assert torch.equal(got, want) and torch.equal(b.kept, a.kept), (V, B, top_k, top_p)
                assert int(_counter(a)) == 12 and int(_counter(b)) == 11


def test_one_sequence_is_the_rows_are_steps_entry():
    """B = 1: ids and kept sets of srgpt_sample_rows / srgpt_sample_full_rows, whatever the sequence's count"""
    from spatialrgpt_amd import ops

    for V in (2048, 3002):
        for T, s in ((2, 1), (4, 7), (16, 0)):
            st = torch.tensor([s], dtype=torch.int32, device=DEV)
            for si, (full, top_k, top_p) in enumerate([(False, *x) for x in TOPK64] + [(True, *x) for x in FULL]):
                _, lg, _ = _logits(T, V, top_k if top_k else 10, 17 * T + si)
                a = ops.SamplingParams(DEV, T, keep_kept_sets=True).set(TEMPERATURE, top_k, top_p, seed=9 + si, counter=2 ** 32 - 1)
                b = ops.SamplingParams(DEV, T, keep_kept_sets=True).set(TEMPERATURE, top_k, top_p, seed=9 + si, counter=2 ** 32 - 1)
                if full:
                    want, got = ops.sample_full_rows(lg, a, kept_mask=True), ops.sample_full_seq_rows(lg, b, st, T, kept_mask=True)
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (V, T, top_k, top_p)
                else:
                    want, got = ops.sample_rows(lg, a, check=True), ops.sample_seq_rows(lg, b, st, T, check=True)
                    assert torch.equal(got, want) and torch.equal(b.kept, a.kept), (V, T, top_k, top_p)
                assert int(_counter(a)) == 2 ** 32 - 1 + T and int(_counter(b)) == 2 ** 32 - 1


def test_row_counters_cross_the_low_words_carry():
    """c0 = 2^32 - 2, steps (3, 1), T = 4: sequence 0 reads 2^32 .. 2^32 + 3, sequence 1 reads 2^32 - 2 .. 2^32 + 1 -- rows on both
    sides of the carry, in one launch"""
    c0 = 2 ** 32 - 2
    for si, (top_k, top_p) in enumerate(TOPK64):
        _seq_rows_against_b_row_calls(2, 4, (3, 1), 2048, False, top_k, top_p, c0=c0, seed=7 + si)
    for si, (top_k, top_p) in enumerate(FULL):
        _seq_rows_against_b_row_calls(2, 4, (3, 1), 2048, True, top_k, top_p, c0=c0, seed=17 + si)


def test_unserved_settings_are_reported_like_srgpt_sample():
    from spatialrgpt_amd import ops

    _, lg, _ = _logits(4, 1000, 10, 1)
    st = torch.tensor([2, 1], dtype=torch.int32, device=DEV)
    with pytest.raises(NotImplementedError):
        ops.sample_seq_rows(lg, ops.SamplingParams(DEV, 4).set(TEMPERATURE, 65, 1.0, seed=1), st, 2, check=True)
    ops.sample_seq_rows(lg, ops.SamplingParams(DEV, 4).set(TEMPERATURE, 64, 1.0, seed=1), st, 2, check=True)


def test_the_old_modes_still_draw_the_recorded_ids():
    """tests/golden/pick_kat.npz on the stored logits, after the sequences-x-steps kernels ran in this process: ops.sample and
    ops.sample_full return the recorded ids and counters for B = 1 and B = 3"""
    from spatialrgpt_amd import _lib as L, ops

    _seq_rows_against_b_row_calls(2, 4, (3, 1), 2048, False, 50, 1.0, c0=3, seed=1)
    _seq_rows_against_b_row_calls(2, 4, (3, 1), 2048, True, 0, 0.9, c0=3, seed=2)
    z = np.load(os.path.join(GOLD, "pick_kat.npz"))
    logits = {V: torch.from_numpy(np.ascontiguousarray(z[f"logits.V{V}"])).to(DEV) for V in pick_kat.STORED_V}
    n = 0
    for name, V, B, counter, which, (temperature, top_k, top_p), seed in pick_kat.cases():
        if V not in logits:
            continue
        n += 1
        sp = ops.SamplingParams(DEV, B).set(temperature, top_k, top_p, seed=seed, counter=counter)
        lg = logits[V][:B].contiguous()
        ids = ops.sample(lg, sp, check=True) if which == "sample" else ops.sample_full(lg, sp)
        assert np.array_equal(ids.cpu().numpy(), z[name + ".ids"]), name
        assert L.Sampling.from_buffer_copy(sp.buf.cpu().numpy().tobytes()).counter == int(z[name + ".counter"]) == counter + 1, name
    assert n == 2 * 2 * 2 * 6
