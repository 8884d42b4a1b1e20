"""The decode products' route choice (spatialrgpt_amd/csrc/gemv_route.h) on the CPU: which kernel family, which template instance,
which grid, and how a call of many rows is cut into weight passes.  Every route computes the same bits, so a slipped threshold only
shows as a slower decode step.  `tests/golden/gemv_routes.json` holds, for every product of the decode step at the three LLM
geometries (rows 1, 2, 4, 8, 16, 17; bf16, fp8 row-major and fp8 packed weights) and for the edges of the rules, the launches (kernel
name with template arguments, grid and block size) of the selection code as it stood before it moved into the header, at 256 CUs
(profiles/NOTEBOOK.md says how it was made); the header -- compiled alone into tests/gemv_route_cli.cpp, no HIP -- has to reproduce
every row."""
import itertools
import json
import os

import pytest

from tests.util import build_gemv_route_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_CAP = 150 * 1024
ROWSS_STRIDE = 512  # SRGPT_ROWSS_STRIDE
DEFAULT_LDS = 48 * 1024  # dynamic LDS a kernel may use without srgpt_ensure_dyn_lds raising its limit
DTYPE_OF_ENTRY = {"gemv_bf16": "bf16", "gemv_f32": "f32", "gemv_w8": "fp8", "rowss_bf16": "bf16", "rowss_fp8": "fp8"}


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return build_gemv_route_cli(tmp_path_factory.mktemp("gemv_route"))


def launch_of(dtype, swiglu, family, p):
    """the one place that says which kernel (name with template arguments) and block size a route's pass means"""
    b = ("false", "true")
    if family == "skinny":
        return "skinny_kernel<%s, %d, %d, %s, %s, %s>" % (b[swiglu], p["NI"], p["NW"], b[dtype == "fp8"], b[p["PUB"]], b[p["PK"]]), 64 * p["NW"]
    if family == "gemv_reg":
        return "gemv_reg_kernel<%s, false, %d>" % (b[swiglu], p["NIT"]), 256
    if family == "gemv_w8":
        return "gemv_w8_kernel<%d, %s, %d>" % (p["B"], b[swiglu], p["NX"]), 256
    assert family == "gemv"
    return "gemv_kernel<%s, %d, %s, %d, %d>" % ("bf16" if dtype == "bf16" else "float", p["B"], b[swiglu], p["NX"], p["UB"]), 256


def test_every_recorded_launch_is_reproduced(cli):
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "gemv_routes.json")))
    products = {(r["product"], r["geometry"], r["format"], r["rows"]) for r in rows if r["geometry"]}
    assert len(products) == 5 * 3 * 3 * 6  # q/k/v, o, gate/up, down, lm_head x geometries x weight formats x rows
    routes = [None] * len(rows)
    for cus in sorted({r["cus"] for r in rows}):  # 256; 304 where the statistics table has too few slots
        idx = [i for i, r in enumerate(rows) if r["cus"] == cus]
        got = cli([(DTYPE_OF_ENTRY[rows[i]["entry"]], rows[i]["rows"], rows[i]["N"], rows[i]["K"], rows[i]["norm"], rows[i]["swiglu"],
                    rows[i]["ss_in"], rows[i]["packed"]) for i in idx], cus)
        for i, g in zip(idx, got):
            routes[i] = g
    assert {(r["cus"], r["rowss_supported"]) for r in rows} == {(256, 0), (256, 1), (304, 0)}
    seen = set()
    for row, got in zip(rows, routes):
        what = "%s %s %s %s rows=%d N=%d K=%d: %s" % (row["product"], row["geometry"], row["format"], row["entry"], row["rows"], row["N"],
                                                      row["K"], got)
        assert got["rowss_supported"] == row["rowss_supported"], what
        assert len(got["passes"]) == len(row["launches"]), what
        for want, p in zip(row["launches"], got["passes"]):
            name, block = launch_of(DTYPE_OF_ENTRY[row["entry"]], row["swiglu"], got["family"], p)
            assert (name, p["grid"], block, p["rows"]) == (want["kernel"], want["grid"], want["block"], want["rows"]), what
            # dynamic LDS, and what the kernel's limit is raised to (0: left alone)
            limit = (p["lds"] if p["lds"] > DEFAULT_LDS else 0) if got["family"] == "skinny" else (LDS_CAP if p["raise"] else 0)
            assert (p["lds"], limit) == (want["lds"], want["lds_limit"]), what
            seen.add(name)
    # every family, both NX instances, the register kernel, batches of 7 loads, PUB, PK, both block sizes, every NI
    for pat in ("gemv_kernel<bf16, 1, false, 2, 8>", "gemv_kernel<bf16, 1, false, 8, 8>", "gemv_kernel<bf16, 1, true, 2, 8>",
                "gemv_kernel<bf16, 1, false, 8, 7>", "gemv_kernel<float, 4, false, 8, 8>", "gemv_reg_kernel<false, false, 5>",
                "gemv_reg_kernel<false, false, 8>", "gemv_reg_kernel<false, false, 14>", "gemv_reg_kernel<true, false, 5>",
                "gemv_w8_kernel<1, false, 2>", "gemv_w8_kernel<1, false, 8>", "gemv_w8_kernel<1, true, 2>",
                "skinny_kernel<false, 2, 4, false, false, false>", "skinny_kernel<false, 4, 8, false, true, false>",
                "skinny_kernel<true, 4, 4, true, true, true>", "skinny_kernel<false, 4, 4, true, false, true>",
                "skinny_kernel<false, 8, 4, true, false, true>", "skinny_kernel<true, 8, 8, false, true, false>",
                "skinny_kernel<false, 4, 4, false, false, true>"):
        assert pat in seen, pat + " has no row in the table"


@pytest.mark.parametrize("cus", [8, 104, 256, 304])
def test_structure_of_every_route(cli, cus):
    Ns = (1, 17, 100, 1000, 4096, 6144, 16 * cus, 16 * cus + 1, 24 * cus, 32 * cus, 32 * cus + 1, 56 * cus, 128258)
    Ks = (8, 64, 264, 2560, 4096, 4104, 6912, 11008, 14336, 35848, 38400)
    ROWS = (*range(1, 10), 15, 16, 17, 18, 31, 32, 33, 40)
    queries = []
    for dtype, rows, N, K, norm, swiglu in itertools.product(("bf16", "f32", "fp8"), ROWS, Ns, Ks, (0, 1), (0, 1)):
        for ss_in, packed in ((0, 0), (1, 0), (0, 4), (1, 8), (1, 16)):
            if dtype == "f32" and (ss_in or packed):
                continue
            if (ss_in and not norm) or (packed and (N % packed or K % 64)):  # refused by the entry points
                continue
            queries.append((dtype, rows, N, K, norm, swiglu, ss_in, packed))
    families = set()
    for (dtype, rows, N, K, norm, swiglu, ss_in, packed), r in zip(queries, cli(queries, cus)):
        what = "%s rows=%d N=%d K=%d norm=%d swiglu=%d ss_in=%d packed=%d: %s" % (dtype, rows, N, K, norm, swiglu, ss_in, packed, r)
        families.add(r["family"])
        assert sum(p["rows"] for p in r["passes"]) == rows, what
        assert all(1 <= p["rows"] <= r["chunk"] for p in r["passes"]), what
        # every pass of a call is on the first pass's family: same kernel template, same block size
        kernels = [launch_of(dtype, swiglu, r["family"], p) for p in r["passes"]]
        assert len({(k.split("<")[0], blk) for k, blk in kernels}) == 1, what
        es = 4 if dtype == "f32" else 2
        for p in r["passes"]:
            if r["family"] == "skinny":
                assert dtype != "f32" and p["rows"] <= 16 and p["NI"] == (2 if p["rows"] <= 4 else 4 if p["rows"] <= 8 else 8), what
                assert p["NW"] in (4, 8) and (p["NW"] == 4 or norm), what
                assert p["grid"] * p["cw"] >= N > (p["grid"] - 1) * p["cw"], what
                assert p["cw"] >= 16 and (not packed or (p["cw"] % packed == 0 and 1 << p["gr_shift"] == packed)), what
                assert p["grid"] <= (cus if p["NW"] == 8 else 2 * cus), what
                if 2 * cus <= ROWSS_STRIDE:  # where srgpt_gemv_rowss is supported, every producer block has its slot
                    assert p["grid"] <= ROWSS_STRIDE, what
                assert p["PUB"] == ss_in and p["PK"] == (packed != 0), what
                assert 0 < p["lds"] <= LDS_CAP, what
            else:
                assert p["B"] == p["rows"] <= 4, what
                per_cu = 1 if p["rows"] * K * es > 70 * 1024 else 2
                assert 1 <= p["grid"] <= cus * per_cu, what
                if r["family"] == "gemv_reg":
                    assert dtype == "bf16" and rows == 1 and not norm and p["lds"] == 0 and p["NIT"] in (5, 8, 14), what
                    continue
                assert p["NX"] in (2, 8) and p["UB"] in (7, 8), what
                assert p["UB"] == 8 or (dtype == "bf16" and rows == 1 and not swiglu and p["NX"] == 8 and r["family"] == "gemv"), what
                assert (r["family"] == "gemv_w8") == (dtype == "fp8") and (dtype != "fp8" or rows == 1), what
                assert p["lds"] == p["rows"] * K * es and p["raise"] == (p["lds"] > 48 * 1024), what
                if rows > 4 or rows * K * es <= LDS_CAP:  # (1 - 4 rows that do not fit: the launcher refuses the call)
                    assert p["lds"] <= LDS_CAP, what
        if dtype != "f32" and rows >= 2:  # 2+ bf16 rows: the MFMA kernel, 16 rows per weight pass
            assert r["family"] == "skinny" and r["chunk"] == 16, what
    assert families == {"gemv", "gemv_reg", "gemv_w8", "skinny"}
