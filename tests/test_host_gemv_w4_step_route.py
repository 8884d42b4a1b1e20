"""CPU: the routes of an MXFP4 engine's decode-shaped steps (spatialrgpt_amd/csrc/gemv_route.h: gemv_w4_step_route, W4_MFMA_MIN_ROWS
and the MFMA launch over the packed copies) as pure functions, through tests/gemv_w4_step_route_cli.cpp."""
import json
import os
import re
import subprocess

import pytest

from tests.util import ROOT, _build_route_cli

G = 16            # W4_GRANULE_ROWS
PRODUCTS = {      # Llama-3-8B geometry: N, K, swiglu, norm, ss_in (as layer i > 0 of the step launches them)
    "qkv": (6144, 4096, 0, 1, 1), "o_proj": (4096, 4096, 0, 0, 0), "gate_up": (14336, 4096, 1, 1, 1), "down": (4096, 14336, 0, 0, 0)}
VALU_KEYS = ("rows", "B", "NX", "NIT", "grid", "lds", "raise")
MFMA_KEYS = ("rows", "NI", "NW", "PUB", "PK", "grid", "cw", "gr_shift", "lds")


def _min_rows():
    src = open(os.path.join(ROOT, "spatialrgpt_amd", "csrc", "gemv_route.h")).read()
    return int(re.search(r"constexpr int W4_MFMA_MIN_ROWS = (\d+);", src).group(1))


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    exe = _build_route_cli(tmp_path_factory.mktemp("gemv_w4_step_route"), "gemv_w4_step_route_cli")

    def run(queries, cus=256):
        text = "".join("%d %d %d %d %d %d %d\n" % tuple(q) for q in queries)
        out = subprocess.run([exe, str(int(cus))], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        assert len(out) == len(queries)
        res = []
        for ln in out:
            head, *passes = ln.split(" | ")
            family, chunk = head.split()
            keys = VALU_KEYS if family == "gemv_w4" else MFMA_KEYS
            res.append(dict(family=family, chunk=int(chunk), launches=[dict(zip(keys, map(int, p.split()))) for p in passes]))
        return res

    return run


@pytest.fixture(scope="module")
def w4_cli(tmp_path_factory):
    """the unbound reference: gemv_w4_route / gemv_w4_launch through their own program"""
    exe = _build_route_cli(tmp_path_factory.mktemp("gemv_w4_route_ref"), "gemv_w4_route_cli")

    def run(queries, cus):
        text = "".join("%d %d %d %d\n" % tuple(q) for q in queries)
        return subprocess.run([exe, str(int(cus))], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]

    return run


def test_threshold_is_two_rows():
    assert _min_rows() == 2


def test_recorded_routes_of_the_step_are_reproduced(cli):
    """tests/golden/gemv_w4_step_routes.json: the four products (Llama-3-8B geometry) at 1, 2, 3, 4, 5, 16 and 17 rows, 256 CUs,
    bound and unbound"""
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "gemv_w4_step_routes.json")))
    assert {(r["product"], r["rows"], r["bound"]) for r in rows} == {(p, n, b) for p in PRODUCTS for n in (1, 2, 3, 4, 5, 16, 17)
                                                                       for b in (0, 1)}
    for r in rows:
        assert (r["N"], r["K"], r["swiglu"], r["norm"], r["ss_in"]) == PRODUCTS[r["product"]] and r["cus"] == 256
    got = cli([(r["rows"], r["N"], r["K"], r["swiglu"], r["norm"], r["ss_in"], r["bound"]) for r in rows], 256)
    for want, g in zip(rows, got):
        assert g == {k: want[k] for k in ("family", "chunk", "launches")}, (want, g)
    # 5 .. 16 rows are ONE pass over the packed copy where the VALU kernel takes two to four
    by = {(r["product"], r["rows"], r["bound"]): r for r in rows}
    for p in PRODUCTS:
        assert len(by[p, 16, 1]["launches"]) == 1 and len(by[p, 16, 0]["launches"]) == 4
        assert len(by[p, 5, 1]["launches"]) == 1 and len(by[p, 5, 0]["launches"]) == 2


@pytest.mark.parametrize("cus", [8, 104, 256, 304])
def test_structure_of_every_route(cli, w4_cli, cus):
    thr = _min_rows()
    shapes = [(N, K, sw, norm, ss) for N in (1, 3, 16, 17, 64, 4096, 6144, 14336, 40000) for K in (128, 384, 2048, 2176, 4096, 14336)
              for sw in (0, 1) for norm, ss in ((0, 0), (1, 0), (1, 1)) if not (sw and N % G)]
    queries = [(rows, *s, bound) for rows in (*range(1, 10), 16, 17, 33) for s in shapes for bound in (0, 1)]
    ref = w4_cli([(q[0], q[1], q[2], q[3]) for q in queries], cus)
    for (rows, N, K, sw, norm, ss, bound), r, ref_line in zip(queries, cli(queries, cus), ref):
        what = "rows=%d N=%d K=%d swiglu=%d norm=%d ss_in=%d bound=%d: %s" % (rows, N, K, sw, norm, ss, bound, r)
        if not bound or rows < thr:  # gemv_w4_route's answer, launch for launch
            assert r["family"] == "gemv_w4" and r["chunk"] == min(rows, 4), what
            head, *passes = ref_line.split(" | ")
            assert head.split()[:2] == ["gemv_w4", str(r["chunk"])], what
            assert r["launches"] == [dict(zip(VALU_KEYS, map(int, p.split()))) for p in passes], what
            continue
        assert r["family"] == "gemv_w4_mfma" and r["chunk"] == 16, what
        assert [p["rows"] for p in r["launches"]] == [16] * (rows // 16) + ([rows % 16] if rows % 16 else []), what
        for p in r["launches"]:
            assert p["NI"] == (2 if p["rows"] <= 4 else 4 if p["rows"] <= 8 else 8), what
            assert p["NW"] == (8 if norm and (N + cus - 1) // cus <= 32 else 4), what  # gemv_skinny_launch's rule
            assert p["PK"] == 1 and p["PUB"] == ss and p["gr_shift"] == 4, what
            assert p["cw"] % G == 0 and p["cw"] >= 16 and p["grid"] * p["cw"] >= N and (p["grid"] - 1) * p["cw"] < N, what
            assert p["grid"] <= (cus if p["NW"] == 8 else 2 * cus), what
            assert p["lds"] == max(p["NW"] * 2 * p["NI"] * 544, p["NW"] * 4 * 64 * 16), what  # activation stages only | reduction
