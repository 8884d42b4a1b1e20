"""Known answers of the attention kernels: one launch of every reachable instance of decode_split_kernel, decode_mfma_kernel,
flash_bf16_kernel and simple_attn_kernel (tests/attn_kat.py) has to reproduce, bit for bit, what tests/golden/attn_kat.npz holds --
recorded by scripts/mint_attn_kat.py with the build from before the attention routes moved into csrc/attn_route.h.  The tolerance
tests of this family cannot tell two routes, or two orders of summation, apart; this one can."""
import os

import numpy as np
import pytest

from tests import attn_kat
from tests.util import GOLD

pytestmark = pytest.mark.gpu


def test_every_attention_instance_reproduces_the_recorded_bits():
    from spatialrgpt_amd import ops

    z = np.load(os.path.join(GOLD, "attn_kat.npz"))
    got = attn_kat.run_cases(ops)
    n_decode, n_prefill = len(list(attn_kat.decode_cases())), len(list(attn_kat.prefill_cases()))
    assert (n_decode, n_prefill) == (2 * 4 * 4 + 1, 2 * 6)
    assert sorted(got) == sorted(z.files) and len(got) == 4 * n_decode + 2 * n_prefill
    for k, v in got.items():
        assert v.dtype == z[k].dtype and v.shape == z[k].shape, (k, v.dtype, v.shape, z[k].dtype, z[k].shape)
        assert np.array_equal(v, z[k]), (k, np.flatnonzero(v.ravel() != z[k].ravel())[:8])
        if k.endswith(".tickets"):
            assert not v.any(), k  # re-armed by the merging block
