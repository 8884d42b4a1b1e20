"""GPU: every sampled token against the host restatement of the draw (tests/draw_ref.py): Philox4x32-10 at the draw's address, the
inverse-CDF walk of the top-k-64 sampler, the Gumbel-max key of the pure-temperature path and of the full sampler -- through
ops.sample, ops.sample_full and their rows-are-steps and sequences-x-steps entries.  Per row: the token is the reference's (or, where
the reference itself calls the case ambiguous, one of the tokens it admits), the kept set is the reference's, the block's counter
moved as the entry promises.  The edges: u = 0 and the largest u of the walk, a walk that lands exactly on a boundary, and the three
Gumbel addresses whose 24 random bits are all ones -- the u that rounded to 1 and made its entry win whatever its score."""
import numpy as np
import pytest
import torch

from tests import draw_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from spatialrgpt_amd import ops

    return ops


def _counter(sp):
    from spatialrgpt_amd import _lib as L

    return L.Sampling.from_buffer_copy(sp.buf.cpu().numpy().tobytes()).counter


def _params(which, rows, setting, seed, counter):
    ops = _ops()
    return ops.SamplingParams(DEV, rows, keep_kept_sets=which == "sample" and setting[1] > 0).set(*setting, seed=seed, counter=counter)


def _call(which, entry, lg, sp, *seq):
    """-> (tokens [rows], the kept sets: per row the ranked list of the top-k-64 sampler, the bool mask of the full one, or None)"""
    ops = _ops()
    if which == "sample":
        tok = getattr(ops, entry)(lg, sp, *seq, check=True).cpu().tolist()
        if sp.kept is None:
            return tok, [None] * len(tok)
        kept = sp.kept.cpu().numpy()
        return tok, [kept[r, 1:1 + kept[r, 0]].tolist() for r in range(len(tok))]
    tok, kept = getattr(ops, entry)(lg, sp, *seq, kept_mask=True)
    return tok.cpu().tolist(), list(kept.cpu().numpy())


def _check_row(ref, tok, kept, row, where):
    """one row against its reference; `where` names the address"""
    msg = (f"{where}: drew {tok}, reference {ref.tok} (admits {sorted(ref.ok)}), u = {ref.u!r}, margin {ref.margin:.3e} against "
           f"{ref.d:.3e}, ambiguous: {ref.ambiguous}")
    assert tok in ref.ok, msg
    if ref.ambiguous or kept is None:
        return
    if ref.kind == "icdf":
        assert kept == ref.kept, msg + f"; kept list {kept}, reference {ref.kept}"
    else:  # an entry of score -inf is outside every kept set, whatever the mask says of it: HF marks filtered entries with -inf
        finite = np.isfinite(row)
        assert np.array_equal(kept & finite, ref.kept & finite), msg + f"; kept mask differs at {np.nonzero((kept ^ ref.kept) & finite)[0][:8]}"


@pytest.mark.parametrize("chain", list(R.chains()), ids=R.chain_id)
def test_every_token_is_the_references(chain):
    which, setting, V, rows, seed = (chain[k] for k in ("which", "setting", "V", "rows", "seed"))
    logits = R.case_logits(V)
    lg = torch.from_numpy(np.array(logits[list(rows)])).to(DEV)
    sp = _params(which, len(rows), setting, seed, chain["counter"])
    for i in range(chain["calls"]):
        ctr = (chain["counter"] + i) & R.M64
        tok, kept = _call(which, which, lg, sp)
        assert _counter(sp) == (ctr + 1) & R.M64, (R.chain_id(chain), i)
        for b, row in enumerate(rows):
            ref = R.ref_chain_row(which, setting, V, row, seed, *R.addr_seqs(ctr, b))
            _check_row(ref, tok[b], kept[b], logits[row], f"{R.chain_id(chain)} call {i} row {b} (seed {seed}, ctr {ctr}, seq {b})")


@pytest.mark.parametrize("which,setting", R.MODE_SETTINGS)
@pytest.mark.parametrize("counter", R.STEPS_COUNTERS)
def test_rows_that_are_steps(which, setting, counter):
    """T = 4 rows: row t draws at (counter + t, 0), the sum carried into the high word; the counter moves by T"""
    logits, rows, seed, T = R.case_logits(R.MODE_V), list(R.STEPS_ROWS), R.STEPS_SEED, len(R.STEPS_ROWS)
    lg = torch.from_numpy(np.array(logits[rows])).to(DEV)
    sp = _params(which, T, setting, seed, counter)
    tok, kept = _call(which, which + "_rows", lg, sp)
    assert _counter(sp) == counter + T
    for t, row in enumerate(rows):
        ctr, seq = R.addr_steps(counter, t)
        _check_row(R.ref_draw(which, logits[row], setting, seed, ctr, seq), tok[t], kept[t], logits[row],
                   f"{which}_rows row {t} (seed {seed}, ctr {ctr}, seq {seq})")


@pytest.mark.parametrize("which,setting", R.MODE_SETTINGS)
@pytest.mark.parametrize("steps", R.SEQ_STEPS)
def test_rows_of_sequences_x_steps(which, setting, steps):
    """B = 2 sequences x T = 3 steps: row b * T + t draws at (counter + max(steps[b], 0) - m + t, b); the counter stays"""
    logits, rows, T, seed, counter = R.case_logits(R.MODE_V), list(R.SEQ_ROWS), R.SEQ_T, R.SEQ_SEED, R.SEQ_COUNTER
    lg = torch.from_numpy(np.array(logits[rows])).to(DEV)
    sp = _params(which, len(rows), setting, seed, counter)
    tok, kept = _call(which, which + "_seq_rows", lg, sp, torch.tensor(steps, dtype=torch.int32, device=DEV), T)
    assert _counter(sp) == counter
    for r, row in enumerate(rows):
        ctr, seq = R.addr_seq_steps(counter, steps, T, r // T, r % T)
        _check_row(R.ref_draw(which, logits[row], setting, seed, ctr, seq), tok[r], kept[r], logits[row],
                   f"{which}_seq_rows row {r} (seed {seed}, ctr {ctr}, seq {seq})")


def _one(which, row, setting, counter, seed=1):
    lg = torch.from_numpy(np.array(row[None])).to(DEV)
    tok, kept = _call(which, which, lg, _params(which, 1, setting, seed, counter))
    ref = R.ref_draw(which, row, setting, seed, counter, 0)
    assert not ref.ambiguous, (ref.margin, ref.d)
    _check_row(ref, tok[0], kept[0], row, f"{which} {setting} (seed {seed}, ctr {counter}, seq 0)")
    return tok[0], ref


@pytest.mark.parametrize("setting", R.WALK_EDGE_SETTINGS)
def test_the_walks_first_and_last_uniform(setting):
    """u = 0 picks rank 0; the largest u, 1 - 2^-24, picks the last kept rank (both counters lie above 2^32)"""
    row = R.case_logits(1000)[R.ROW_PLAIN]
    tok, ref = _one("sample", row, setting, R.EDGE_ICDF_ZERO)
    assert ref.n == 0 and tok == ref.kept[0]
    tok, ref = _one("sample", row, setting, R.EDGE_ICDF_LAST)
    assert ref.n == 0xFFFFFF and tok == ref.kept[-1] and len(ref.kept) > 1


@pytest.mark.parametrize("counter,j", R.EDGE_WALK_EXACT)
def test_a_walk_that_lands_on_a_boundary(counter, j):
    """64 equal scores, u = j / 64: u * Z == c_{j - 1} in exact arithmetic, and `target < c` moves on to rank j"""
    row = R.walk_exact_row()
    tok, ref = _one("sample", row, (1.0, 64, None), counter)
    assert ref.n == j << 18 and ref.d == 0.0 and tok == ref.kept[j]


@pytest.mark.parametrize("counter,hit", R.EDGE_GUMBEL)
def test_a_gumbel_uniform_of_all_ones_stays_below_one(counter, hit):
    """the entry whose 24 random bits are all ones sits 30 below the row maximum: with u < 1 its key loses by a wide margin"""
    row = R.edge_gumbel_row(hit)
    assert int(R.gumbel_n(1, counter, 0, hit)) == 0xFFFFFF
    for which in ("sample", "sample_full"):  # pure temperature; the full sampler with everything kept
        tok, ref = _one(which, row, (1.0, 0, None), counter)
        assert tok != hit and ref.tok != hit
    tok, ref = _one("sample_full", row, (1.0, 64, None), counter)  # the hit entry outside the kept set: masked, never drawn
    assert tok != hit and not ref.kept[hit]


@pytest.mark.parametrize("which", ("sample", "sample_full"))
def test_the_gumbel_uniform_carries_its_half(which):
    """two finite entries whose keys stand 0.024 apart with u = (n + 0.5) * 2^-24 and the other way round without the half"""
    row, a, b = R.no_half_row()
    tok, ref = _one(which, row, (1.0, 0, None), R.NO_HALF_CTR)
    assert tok == a and ref.margin > 100 * ref.d
