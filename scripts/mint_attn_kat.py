"""Mint tests/golden/attn_kat.npz: the output bits of one launch of every attention kernel instance on hashed inputs
(tests/attn_kat.py lists the cases), recorded with the library build that SRGPT_LIB names (default: the tree's own).
tests/test_gpu_attn_kat.py holds every later build to these bits -- so mint with the build whose results are the contract, on an
MI355X:
  SRGPT_LIB=<path of a libsrgpt_hip*.so build> python scripts/mint_attn_kat.py [OUT.npz]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from spatialrgpt_amd import _lib  # noqa: E402

if os.environ.get("SRGPT_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["SRGPT_LIB"])
from spatialrgpt_amd import ops  # noqa: E402
from tests import attn_kat  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "attn_kat.npz")
rec = attn_kat.run_cases(ops)
np.savez_compressed(out, **rec)
print(f"{out}: {len(rec)} arrays, {os.path.getsize(out)} bytes, minted with {_lib.LIB_PATH}")
