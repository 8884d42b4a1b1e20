"""The GEMM launchers' route choice (spatialrgpt_amd/csrc/gemm_route.h) on the CPU: which kernel, which tile, single or double
buffer, how many K splits.  Every route computes the same bits, so a slipped threshold only shows as a slower kernel on a workload
shape.  `tests/golden/gemm_routes.json` holds, for the workload's shapes and the edges of the rules, the launch (kernel name with
template arguments, grid in blocks, the reduce kernel that follows) of the selection code as it stood before it moved into the
header, at 256 CUs with the workspace ops.py hands over (profiles/NOTEBOOK.md says how it was made); the header -- compiled alone
into tests/gemm_route_cli.cpp, no HIP -- has to reproduce every row."""
import itertools
import json
import os

import pytest

from tests.util import build_gemm_route_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256
SPLIT_CAP = {"whole_m_288": 8, "glds": 8, "tile_256": 4}


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    run = build_gemm_route_cli(tmp_path_factory.mktemp("gemm_route"))
    return lambda queries: run(queries, CUS)


def launch_of(entry, M, N, r):
    """the one place that says which kernel (name as the trace prints it) and grid (blocks) a route means"""
    if r["family"] == "glds":
        return "gemm_bf16_glds<%d, 128, %d>" % (r["bm"], r["nbuf"]), [cdiv(N, 128), cdiv(M, r["bm"]), r["splits"]]
    if r["family"] == "whole_m_288":
        return "gemm_bf16_288_kernel", [cdiv(N, 128), r["splits"], cdiv(M, r["bm"])]
    assert r["family"] == "tile_256" and r["bm"] == 256
    tiles = cdiv(M, 256) * cdiv(N, 256)
    if entry == "gemm_w8a8":
        return "gemm_f8_256_kernel", [tiles, r["splits"], 1]
    persist = r["splits"] == 1 and tiles > CUS  # gemm256.hip: more tiles than CUs, no split -> one block per CU walks its tiles
    name = "gemm_bf16_256_kernel<%s, %s>" % ("true" if entry == "gemm_w8" else "false", "true" if persist else "false")
    return name, [CUS if persist else tiles, r["splits"], 1]


def test_every_recorded_launch_is_reproduced(cli):
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_routes.json")))
    assert len(rows) >= 24
    # ops.py's workspace: 8 slabs of M x N fp32 up to 2^24 elements, bf16 / fp8 products only
    routes = cli([(r["entry"], r["M"], r["N"], r["K"], int(r["M"] * r["N"] <= 1 << 24), 32 * r["M"] * r["N"]) for r in rows])
    for row, got in zip(rows, routes):
        what = "%s M=%d N=%d K=%d: %s" % (row["entry"], row["M"], row["N"], row["K"], got)
        name, grid = launch_of(row["entry"], row["M"], row["N"], got)
        assert name == row["kernel"], what
        assert grid == row["grid"], what
        assert (row["reduce"] is not None) == (got["splits"] > 1), what
        if row["reduce"]:  # the vectorised reductions keep 4 or 8 slabs in flight
            assert row["reduce"].startswith("splitk_reduce") and row["reduce"].endswith(", %d>" % (4 if got["splits"] <= 4 else 8)), what
    seen = {launch_of(r["entry"], r["M"], r["N"], g)[0] for r, g in zip(rows, routes)}
    for k in ("gemm_bf16_glds<128, 128, 1>", "gemm_bf16_glds<96, 128, 1>", "gemm_bf16_glds<96, 128, 2>", "gemm_bf16_glds<64, 128, 2>",
              "gemm_bf16_288_kernel", "gemm_bf16_256_kernel<false, false>", "gemm_bf16_256_kernel<false, true>",
              "gemm_bf16_256_kernel<true, false>", "gemm_f8_256_kernel"):
        assert k in seen, k + " has no row in the table"


def test_structure_of_every_route(cli):
    Ms = (1, 63, 64, 65, 224, 225, 259, 272, 273, 383, 384, 518, 1036, 2072)
    Ns = (64, 1000, 4096, 12288, 28672)
    Ks = (64, 136, 512, 1024, 4096, 14336)
    queries = []
    for M, N, K in itertools.product(Ms, Ns, Ks):
        for have_ws, ws_bytes in ((0, 0), (1, 32 * M * N), (1, 4 * M * N)):
            queries.append(("gemm", M, N, K, have_ws, ws_bytes))
            if K % 64 == 0:  # srgpt_gemm_w8 takes its scalar kernel otherwise
                queries.append(("gemm_w8", M, N, K, have_ws, ws_bytes))
            if K % 128 == 0 and K >= 256:  # srgpt_gemm_w8a8 refuses anything else
                queries.append(("gemm_w8a8", M, N, K, have_ws, ws_bytes))
    split = set()
    for (entry, M, N, K, have_ws, ws_bytes), r in zip(queries, cli(queries)):
        what = "%s M=%d N=%d K=%d ws=%d/%d: %s" % (entry, M, N, K, have_ws, ws_bytes, r)
        nk = r["nk"]
        assert r["splits"] >= 1, what
        assert r["splits"] * r["tps"] >= nk, what
        assert (r["splits"] - 1) * r["tps"] < nk, what  # no empty split
        if r["splits"] > 1:
            assert r["splits"] * M * N * 4 <= ws_bytes, what
            split.add(r["family"])
        if not have_ws or ws_bytes == 4 * M * N:
            assert r["splits"] == 1, what
        assert r["splits"] <= SPLIT_CAP[r["family"]], what
        if r["family"] == "whole_m_288":
            assert 224 < M <= 272 and K % 64 == 0 and r["bm"] == 272, what
        elif r["family"] == "tile_256":
            assert K % 64 == 0 and (entry != "gemm" or M >= 384) and r["bm"] == 256, what
        else:
            assert entry == "gemm" and r["family"] == "glds" and r["bm"] in (64, 96, 128) and r["nbuf"] in (1, 2), what
            assert r["bm"] != 128 or (r["nbuf"] == 1 and r["splits"] == 1), what
    assert split == set(SPLIT_CAP)  # the sweep reaches split-K on every family


def test_swiglu_fused_shape(cli):
    """srgpt_gemm_swiglu's fused form: 225 .. 272 rows, whole 64-column K tiles (at least 4) and gate / up pairs, half a block per CU"""
    q = [(259, 14336, 4096), (272, 11008, 4096), (225, 8192, 256), (224, 14336, 4096), (273, 14336, 4096), (259, 14336, 4128),
         (259, 14336, 192), (259, 14368, 4096), (259, 8128, 4096)]
    got = cli([("swiglu", M, I, K, 0, 0) for M, I, K in q])
    assert got == ["fused"] * 3 + ["unfused"] * 6
