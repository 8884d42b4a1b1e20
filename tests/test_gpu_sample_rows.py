"""GPU: the samplers' rows-are-steps mode (srgpt_sample_rows, srgpt_sample_full_rows: csrc/sample.hip, pick_draw in csrc/pick.h).
The rows of a launch are T successive steps of ONE sequence: row t draws at Philox counter c0 + t, sequence 0.  The contract is an
identity, so the reference is the library's own B = 1 entry point called T times on the rows one by one: ids, the counter behind
the call and the kept sets must be EQUAL (torch.equal).  The B-mode entry points themselves are held to the answers recorded in
tests/golden/pick_kat.npz (tests/pick_kat.py) on the same process, after the rows-mode kernels ran.

Shapes: T in {2, 4, 16}; V = 1000 (fewer entries than 128 slices x 64 lanes: slices of 8), 2048 (one 16-entry slice per block) and
32003 (slices of 251, a ragged last slice of 126).  The logits sit between NaN rows and the ids between sentinel rows."""
import os

import numpy as np
import pytest
import torch

from tests import pick_kat
from tests.util import GOLD

pytestmark = pytest.mark.gpu
DEV = "cuda"
TEMPERATURE = 0.7
TOPK64 = ((50, 1.0), (20, 0.9), (0, 1.0))  # (top_k, top_p) of the top-k-64 sampler; (0, 1): Gumbel mode
FULL = ((0, 0.9), (200, 0.95))             # ... of the full sampler
SENT = 0x5A5A5A5A5A5A
COUNTER_AT = 24  # byte offset of srgpt_sampling::counter (float, int, float, float, u64 seed, u64 counter)


def _logits(T, V, k, seed):
    """randn * 3 between two NaN rows, with a tie group planted at every row's k-th score: three entries below it are raised to it.
    -> (the whole buffer, its T rows, how many entries of each row TopKLogitsWarper(k) keeps at the tests' temperature)"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn((T, V), generator=g) * 3
    for t in range(T):
        order = rows[t].argsort(descending=True)
        rows[t, order[[k + 3, k + 40, V - 1]]] = float(rows[t, order[k - 1]])
    scores = rows / TEMPERATURE
    n_topk = (scores >= scores.topk(k, dim=1).values[:, -1:]).sum(dim=1)
    assert bool((n_topk >= k + 3).all())
    big = torch.full((T + 2, V), float("nan"))
    big[1:T + 1] = rows
    big = big.to(DEV)
    return big, big[1:T + 1], n_topk


def _counter(sp):
    return sp.buf[COUNTER_AT:COUNTER_AT + 8].clone().view(torch.int64)


def _rows_against_single_calls(T, V, full, top_k, top_p, c0, seed):
    from spatialrgpt_amd import _lib as L, ops

    big, lg, n_topk = _logits(T, V, top_k if top_k else 10, seed)
    assert lg.is_contiguous() and lg.data_ptr() == big.data_ptr() + V * 4
    # ---- T successive B = 1 calls, row by row
    ref = ops.SamplingParams(DEV, 1, keep_kept_sets=True).set(TEMPERATURE, top_k, top_p, seed=seed, counter=c0)
    ids, kept = [], []
    for t in range(T):
        ref.kept.zero_()
        if full:
            i, m = ops.sample_full(lg[t:t + 1], ref, kept_mask=True)
            kept.append(m[0].clone())
        else:
            i = ops.sample(lg[t:t + 1], ref, check=True)
            kept.append(ref.kept[0].clone())
        ids.append(i)
    ids, kept = torch.cat(ids), torch.stack(kept)
    # ---- one rows-mode call, the ids between sentinel rows
    out = torch.full((3, T), SENT, dtype=torch.int64, device=DEV)
    sp = ops.SamplingParams(DEV, T, keep_kept_sets=True).set(TEMPERATURE, top_k, top_p, seed=seed, counter=c0)
    if full:
        got, got_kept = ops.sample_full_rows(lg, sp, kept_mask=True, out=out[1])
    else:
        got, got_kept = ops.sample_rows(lg, sp, check=True, out=out[1]), sp.kept
    torch.cuda.synchronize()
    what = (T, V, full, top_k, top_p, c0)
    assert got.data_ptr() == out[1].data_ptr()
    assert torch.equal(got, ids), (what, got.tolist(), ids.tolist())
    assert torch.equal(_counter(sp), _counter(ref)) and int(_counter(sp)) == c0 + T, what
    assert L.Sampling.from_buffer_copy(sp.buf.cpu().numpy().tobytes()).counter == c0 + T
    assert torch.equal(got_kept, kept), what
    # neither the poison nor the sentinels show
    assert bool((out[0] == SENT).all()) and bool((out[2] == SENT).all()) and bool(((got >= 0) & (got < V)).all()), what
    assert bool(big[0].isnan().all()) and bool(big[T + 1].isnan().all())
    if full or top_k:  # the kept sets are real sets: the planted tie group sits at their edge
        n = kept.sum(dim=1) if full else kept[:, 0]
        assert bool((n >= 1).all()), what
        if top_p >= 1.0:
            assert n.tolist() == n_topk.tolist(), (what, n.tolist())  # top-k keeps every tie at the k-th score
    return got


@pytest.mark.parametrize("V", (1000, 2048, 32003))
@pytest.mark.parametrize("T", (2, 4, 16))
def test_rows_equal_successive_single_row_calls(T, V):
    drew = []
    for si, (top_k, top_p) in enumerate(TOPK64):
        drew.append(_rows_against_single_calls(T, V, False, top_k, top_p, c0=3, seed=100 * T + si))
    for si, (top_k, top_p) in enumerate(FULL):
        drew.append(_rows_against_single_calls(T, V, True, top_k, top_p, c0=3, seed=200 * T + si))
    # the rows really are different draws: not every row of every setting picked its argmax
    assert any(len(set(d.tolist())) > 1 for d in drew)


def test_row_counters_cross_the_low_words_carry():
    """c0 = 2^32 - 2: rows 0 and 1 draw below the carry, rows 2 and 3 above it (the high word of the Philox counter is 1)"""
    c0 = 2 ** 32 - 2
    for si, (top_k, top_p) in enumerate(TOPK64):
        _rows_against_single_calls(4, 2048, False, top_k, top_p, c0=c0, seed=7 + si)
    for si, (top_k, top_p) in enumerate(FULL):
        _rows_against_single_calls(4, 2048, True, top_k, top_p, c0=c0, seed=17 + si)


def test_a_carry_that_is_dropped_would_show():
    """the check above has teeth: the draw at counter 2^32 differs from the draw at counter 0 (what a 32-bit sum would address) for
    at least one of a few seeds, so equal ids across the carry are no accident"""
    from spatialrgpt_amd import ops

    _, lg, _ = _logits(1, 2048, 10, 5)
    differ = 0
    for seed in range(8):
        a = ops.sample(lg, ops.SamplingParams(DEV, 1).set(1.0, 0, 1.0, seed=seed, counter=2 ** 32))
        b = ops.sample(lg, ops.SamplingParams(DEV, 1).set(1.0, 0, 1.0, seed=seed, counter=0))
        differ += int(a) != int(b)
    assert differ > 0


def test_rows_mode_reports_unserved_settings_like_srgpt_sample():
    """top_k = 65 on the top-k-64 sampler: the workspace's error word is raised and srgpt_sample_status says so; the next served call
    on a fresh workspace is clean"""
    from spatialrgpt_amd import ops

    _, lg, _ = _logits(2, 1000, 10, 1)
    with pytest.raises(NotImplementedError):
        ops.sample_rows(lg, ops.SamplingParams(DEV, 2).set(TEMPERATURE, 65, 1.0, seed=1), check=True)
    with pytest.raises(NotImplementedError):
        ops.sample_rows(lg, ops.SamplingParams(DEV, 2).set(TEMPERATURE, 0, 0.9, seed=1), check=True)
    ops.sample_rows(lg, ops.SamplingParams(DEV, 2).set(TEMPERATURE, 64, 1.0, seed=1), check=True)


def test_the_sequence_mode_entry_points_still_draw_the_recorded_ids():
    """tests/golden/pick_kat.npz on the stored logits (V = 70 and 1000), after the rows-mode kernels ran in this process: ops.sample
    and ops.sample_full return the recorded ids and counters for B = 1 and B = 3 -- and row 0 of a rows-mode call over the same three
    rows is the recorded B = 1 draw (row 0 reads the stream at (counter, 0) in both modes)"""
    from spatialrgpt_amd import _lib as L, ops

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
        if B == 1:
            sp3 = ops.SamplingParams(DEV, 3).set(temperature, top_k, top_p, seed=seed, counter=counter)
            rows = ops.sample_rows(logits[V], sp3, check=True) if which == "sample" else ops.sample_full_rows(logits[V], sp3)
            assert int(rows[0]) == int(z[name + ".ids"][0]), name
            assert L.Sampling.from_buffer_copy(sp3.buf.cpu().numpy().tobytes()).counter == counter + 3, name
    assert n == 2 * 2 * 2 * 6
