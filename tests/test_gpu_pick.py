"""GPU: the token pick's contract (csrc/pick.h) -- the argmax of the decode entry points resolves ties like torch.argmax wherever
the equal maxima sit (one wave, two waves of a block, one thread's scan, two slices), and both device samplers draw, bit for bit,
the ids recorded in tests/golden/pick_kat.npz (scripts/mint_pick_kat.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import pick_kat
from tests.util import GOLD

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG = float("-inf")
SLICES = 128  # csrc/pick.h PICK_SLICES
# the tiny model's own vocabulary (one entry per slice), and one that is no multiple of 128 with slices of 301 entries (more than
# the block's 256 threads: a thread scans two entries) and a short last slice
VOCABS = (128, 128 * 300 + 77)


@functools.lru_cache(maxsize=None)
def _engine(V):
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine
    from spatialrgpt_amd.weights import synth_state_dict

    cfg = SrgptConfig(vit_hidden=64, vit_inter=176, vit_layers=3, vit_heads=4, image_size=378, patch_size=14, hidden=64, inter=160,
                      layers=2, heads=4, kv_heads=2, vocab=V, mask_token_id=V - 8, depth_token_id=V - 7, rope_theta=500000.0)
    sd = synth_state_dict(cfg, seed=0, dtype=torch.float32, device=DEV)
    return SrgptEngine(cfg, sd, device=DEV, dtype=torch.float32, rope_positions=512, consume_state_dict=True)


@functools.lru_cache(maxsize=None)
def _planted(V):
    """-> (names, rows fp32 [R, V], torch.argmax of the rows on the CPU): scores below 4 with maxima of 10 planted"""
    per = (V + SLICES - 1) // SLICES
    lo = 5 * per  # slice 5
    plant = {"two slices": (100 * per, 3 * per), "three slices, the last one": (V - 1, 50 * per, 77 * per), "index 0": (0,),
             "index V - 1": (V - 1,), "index 0 and V - 1": (V - 1, 0)}
    if per > 256:
        plant.update({"one wave": (lo + 40, lo + 7), "two waves of one block": (lo + 200, lo + 70, lo + 10),
                      "one thread's scan": (lo + 259, lo + 3), "a wave and another slice": (lo + 7, 9 * per + 130)})
    base = torch.from_numpy(pick_kat.hashed_logits(V)[0] / 2)
    rows = []
    for idx in plant.values():
        r = base.clone()
        r[list(idx)] = 10.0
        rows.append(r)
    names = list(plant) + ["all equal", "-inf except one entry", "-inf except entry 0"]
    rows.append(torch.full((V,), 1.5))
    for keep in (V - 2, 0):
        r = torch.full((V,), NEG)
        r[keep] = -3.0
        rows.append(r)
    rows = torch.stack(rows)
    return names, rows, torch.argmax(rows, dim=-1)


@pytest.mark.parametrize("B", (1, 5))
@pytest.mark.parametrize("V", VOCABS)
def test_argmax_resolves_ties_like_torch(V, B):
    """prefill, plant the rows into st.logits, srgpt_llm_sample_first_ex with sampling off: st.tok == torch.argmax of the rows"""
    from spatialrgpt_amd import _lib as L
    from spatialrgpt_amd import ops

    eng = _engine(V)
    names, rows, want = _planted(V)
    R = rows.shape[0]
    x = torch.randn((B, 4, eng.cfg.hidden), generator=torch.Generator().manual_seed(B)).to(DEV)
    st, _, _ = eng.prefill(x, max_new=4, fresh_state=True)
    assert st.c.sampling is None
    for start in range(0, R, B):
        sel = [(start + b) % R for b in range(B)]
        st.logits.copy_(rows[sel])
        for kind in (L.SAMPLER_TOPK64, L.SAMPLER_FULL):  # sampling off: the kind does not matter
            st.tok.fill_(-1)
            L.check(L.load().srgpt_llm_sample_first_ex(C.byref(eng.w.llm), C.byref(st.c), kind, ops._stream()))
            got = st.tok.cpu()
            assert got.tolist() == want[sel].tolist(), [names[i] for i in sel]
            assert st.out_ids[:, 0].cpu().tolist() == got.tolist() and int(st.step.cpu()) == 1


def test_draws_are_bit_for_bit_the_recorded_ones():
    """every case of tests/pick_kat.py: ids, the counter after the call, and the full sampler's kept mask (count and CRC)"""
    from spatialrgpt_amd import _lib as L
    from spatialrgpt_amd import ops

    z = np.load(os.path.join(GOLD, "pick_kat.npz"))
    got = pick_kat.run_cases(ops, L, {V: z[f"logits.V{V}"] for V in pick_kat.STORED_V}, DEV)
    assert sorted(got) == sorted(k for k in z.files if not k.startswith("logits."))
    assert len(got) == 96 * 2 + 48 * 2
    for k, v in got.items():
        assert np.array_equal(v, z[k]), (k, v, z[k])
