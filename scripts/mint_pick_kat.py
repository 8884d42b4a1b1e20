"""Mint tests/golden/pick_kat.npz: the draws of both device samplers on fixed logits, seeds and counters (tests/pick_kat.py lists
the cases), recorded with the library build that SRGPT_LIB names (default: the tree's own).  tests/test_gpu_pick.py holds every
later build to these ids -- so mint with the build whose draws are the contract, on an MI355X:
  SRGPT_LIB=<path of a libsrgpt_hip*.so build> python scripts/mint_pick_kat.py [OUT.npz]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from spatialrgpt_amd import _lib  # noqa: E402

if os.environ.get("SRGPT_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["SRGPT_LIB"])
from spatialrgpt_amd import ops  # noqa: E402
from tests import pick_kat  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "pick_kat.npz")
stored = pick_kat.stored_logits()
rec = pick_kat.run_cases(ops, _lib, stored)
rec.update({f"logits.V{V}": a for V, a in stored.items()})
np.savez_compressed(out, **rec)
print(f"{out}: {len(rec)} arrays, {os.path.getsize(out)} bytes, minted with {_lib.LIB_PATH}")
