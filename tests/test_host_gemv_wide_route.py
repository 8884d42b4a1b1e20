"""The wide pass's route (spatialrgpt_amd/csrc/gemv_route.h: gemv_wide_route, gemv_wide_launch) on the CPU, through
tests/gemv_wide_route_cli.cpp -- the header compiled alone, no HIP.  With the option off (pass_rows = 16), or at 16 rows or fewer, a
call is exactly what gemv_route_cli says for it.  With pass_rows = 32 a call is cut into chunks of 32 rows and a tail; a chunk of 17 -
32 rows is a wide launch with the column split of the 16-row launch, a tail of 16 rows or fewer the 16-row launch of its row count.
tests/golden/gemv_wide_routes.json pins the five products of the decode step at the Llama-3-8B and Llama-2-7B geometries."""
import itertools
import json
import os
import subprocess

import pytest

from tests.util import ROOT, _build_route_cli

LDS_CU = 160 * 1024  # LDS of a CU
NAMES = ("rows", "NI", "NW", "PUB", "PK", "grid", "cw", "gr_shift", "lds")
# Products gemv_wide_route keeps at passes of 16 rows, as (format, packed) -> the route's reason
KEPT_AT_16 = {("bf16", p): "the wide instance of packed bf16 weights spills 2 VGPRs: not built" for p in (4, 8, 16)}


def _lines(exe, queries, cus, fmt):
    text = "".join(fmt % tuple(q) for q in queries)
    out = subprocess.run([exe, str(int(cus))], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(out) == len(queries)
    return out


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    exe = _build_route_cli(tmp_path_factory.mktemp("gemv_wide_route"), "gemv_wide_route_cli")
    return lambda queries, cus=256: _lines(exe, queries, cus, "%s %d %d %d %d %d %d %d %d\n")


@pytest.fixture(scope="module")
def narrow(tmp_path_factory):
    exe = _build_route_cli(tmp_path_factory.mktemp("gemv_route_for_wide"), "gemv_route_cli")
    return lambda queries, cus=256: _lines(exe, queries, cus, "%s %d %d %d %d %d %d %d\n")


def parse(line):
    head, *passes = line.split(" | ")
    family, chunk, supported = head.split()
    assert family in ("skinny", "w4_mfma"), line
    return dict(family=family, chunk=int(chunk), passes=[dict(zip(NAMES, map(int, p.split()))) for p in passes])


Ns = (1, 17, 100, 1000, 4096, 6144, 16 * 256, 16 * 256 + 1, 24 * 256, 32 * 256, 32 * 256 + 1, 56 * 256, 128258)
Ks = (8, 64, 264, 2560, 4096, 4104, 6912, 11008, 14336, 35848, 38400)
ROWS = (*range(1, 10), 15, 16, 17, 18, 31, 32, 33, 40)


def shapes(rows_of):
    for dtype, rows, N, K, norm, swiglu in itertools.product(("bf16", "fp8"), rows_of, Ns, Ks, (0, 1), (0, 1)):
        for ss_in, packed in ((0, 0), (1, 0), (0, 4), (1, 8), (1, 16)):
            if (ss_in and not norm) or (packed and (N % packed or K % 64)):  # refused by the entry points
                continue
            yield dtype, rows, N, K, norm, swiglu, ss_in, packed


@pytest.mark.parametrize("cus", [8, 104, 256, 304])
def test_option_off_or_16_rows_is_the_existing_route(wide, narrow, cus):
    """pass_rows = 16 at every row count, and pass_rows = 32 at 16 rows or fewer: gemv_route_cli's line, character for character"""
    off = [q + (16,) for q in shapes(ROWS)]
    assert wide(off, cus) == narrow([q[:8] for q in off], cus)
    few = [q + (32,) for q in shapes([r for r in ROWS if r <= 16])]
    assert wide(few, cus) == narrow([q[:8] for q in few], cus)
    odd = [q + (p,) for q in shapes((17, 33)) for p in (0, 24, 31, 64)]  # only 32 asks for the wide pass
    assert wide(odd, cus) == narrow([q[:8] for q in odd], cus)


@pytest.mark.parametrize("cus", [8, 104, 256, 304])
def test_structure_of_every_wide_route(wide, narrow, cus):
    queries = [q + (32,) for q in shapes([r for r in ROWS if r > 16] + [48, 64])]
    queries += [("w4", rows, N, K, norm, sw, ss_in, 16, 32) for rows in (17, 24, 32, 33, 40, 64) for N in (16, 4096, 6144, 14336)
                for K in (128, 4096, 14336) for norm, sw, ss_in in ((0, 0, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1))]
    # the 16-row launch of the same product: the reference for NW, cw, grid and gr_shift (w4: the bf16 rule at granules of 16)
    ref = [parse(ln)["passes"][0] for ln in narrow([("bf16" if q[0] == "w4" else q[0], 16) + q[2:8] for q in queries], cus)]
    seen_wide = 0
    for q, ln, r16 in zip(queries, wide(queries, cus), ref):
        fmt, rows, N, K, norm, swiglu, ss_in, packed, _ = q
        r, what = parse(ln), "%s: %s" % (q, ln)
        assert r["family"] == ("w4_mfma" if fmt == "w4" else "skinny"), what
        kept = KEPT_AT_16.get((fmt, packed))
        assert r["chunk"] == (16 if kept else 32), what
        assert sum(p["rows"] for p in r["passes"]) == rows, what
        assert [p["rows"] for p in r["passes"]] == [r["chunk"]] * (rows // r["chunk"]) + ([rows % r["chunk"]] if rows % r["chunk"] else []), what
        for p in r["passes"]:
            for k in ("NW", "cw", "grid", "gr_shift", "PUB", "PK"):  # nothing but NI and the LDS size depends on the row count
                assert p[k] == r16[k], what
            if p["rows"] > 16:
                seen_wide += 1
                assert p["NI"] == 16, what
                assert p["lds"] <= LDS_CU, what
                if p["NW"] == 4:  # the 16-row launch runs two 4-wave blocks per CU: so does the wide one
                    assert 2 * r16["lds"] <= LDS_CU and 2 * p["lds"] <= LDS_CU and p["lds"] <= 80 * 1024, what
                # stages of half a slice, rows of 288 bytes: 32 activation rows per wave and (row-major weights) 16 weight rows
                assert p["lds"] == p["NW"] * (32 + (0 if p["PK"] else 16)) * 288, what
            else:  # a tail: the existing launch of its row count
                assert p["NI"] == (2 if p["rows"] <= 4 else 4 if p["rows"] <= 8 else 8), what
                assert p["lds"] == max(p["NW"] * (2 * p["NI"] + (0 if p["PK"] else 16)) * 544, p["NW"] * 4 * 64 * 16), what
    assert seen_wide or all(KEPT_AT_16.get((q[0], q[7])) for q in queries)


def test_recorded_wide_routes_of_the_decode_step_are_reproduced(wide):
    """tests/golden/gemv_wide_routes.json: q/k/v, o_proj, gate/up, down_proj and lm_head of the Llama-3-8B and Llama-2-7B geometries at
    17, 24, 32, 33, 40 and 64 rows, 256 CUs, as a bf16, an fp8 packed and an MXFP4 packed engine launch them with decode_pass_rows = 32"""
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "gemv_wide_routes.json")))
    assert {(r["product"], r["geometry"], r["format"], r["rows"]) for r in rows} == set(itertools.product(
        ("qkv", "o", "gate_up", "down", "lm_head"), ("llama3_8b", "llama2_7b"), ("bf16", "fp8_packed", "mxfp4_packed"), (17, 24, 32, 33, 40, 64)))
    got = wide([(r["weights"], r["rows"], r["N"], r["K"], r["norm"], r["swiglu"], r["ss_in"], r["packed"], 32) for r in rows], 256)
    for want, ln in zip(rows, got):
        g = parse(ln)
        assert (g["family"], g["chunk"], g["passes"]) == (want["family"], want["chunk"], want["passes"]), (want, ln)
