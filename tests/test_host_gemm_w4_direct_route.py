"""Which `_direct` W4 products multiply their MXFP4 codes inside the GEMM kernel (spatialrgpt_amd/csrc/gemm_route.h:
gemm_w4_direct_in_kernel, gemm_swiglu_w4_direct_in_kernel, gemm288_w4_scales_fit), on the CPU.  The `_direct` entries take the route
of the bf16 product, as the plain ones do; they answer "in the kernel" wherever the plain entry does, and also on the whole-M kernel
(and its fused SwiGLU form) when K % 64 == 0, there are at least 4 K tiles and the scale bytes of a block's K range fit the LDS the
three stages leave.  tests/golden/gemm_w4_direct_routes.json pins the four products of the 8B layer at 32 and 259 rows, 256 CUs,
with the workspace ops.py hands over."""
import itertools
import json
import os
import subprocess

import pytest

from tests.util import _build_route_cli, build_gemm_route_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCTS = {"qkv": ("gemm_w4", 6144, 4096), "o": ("gemm_w4", 4096, 4096), "gate_up": ("swiglu_w4", 14336, 4096),
            "down": ("gemm_w4", 4096, 14336)}
KEYS = ("family", "bm", "nbuf", "splits", "tps", "nk", "in_kernel", "direct_in_kernel", "fits")
# what gemm288_w4_scales_fit allows: 160 KiB of LDS less three stages of 38 KiB, 260 bytes of table per K tile
MAX_TILES = (160 * 1024 - 3 * 38 * 1024) // 260


@pytest.fixture(scope="module")
def clis(tmp_path_factory):
    d = tmp_path_factory.mktemp("gemm_w4_direct_route")
    exe = _build_route_cli(d, "gemm_w4_direct_route_cli")
    plain_exe = _build_route_cli(d, "gemm_w4_route_cli")

    def run(exe_, queries, cus, n):
        text = "".join("%s %d %d %d %d %d\n" % tuple(q) for q in queries)
        out = subprocess.run([exe_, str(int(cus))], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        assert len(out) == len(queries)
        res = []
        for ln in out:
            f = ln.split()
            assert len(f) == n, ln
            res.append(dict(zip(KEYS, [f[0]] + [int(x) for x in f[1:]])))
        return res

    return (lambda q, cus: run(exe, q, cus, 9)), (lambda q, cus: run(plain_exe, q, cus, 7)), build_gemm_route_cli(d)


def _ws(M, rows):
    """ops.py's workspace for an [M, rows] product: 8 fp32 slabs up to 2^24 elements"""
    return int(M * rows <= 1 << 24), 32 * M * rows


def test_max_tiles_is_the_lds_left():
    assert MAX_TILES == 181


def test_the_8b_products_are_pinned(clis):
    direct, plain, _ = clis
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_w4_direct_routes.json")))
    assert {(r["product"], r["M"]) for r in rows} == set(itertools.product(PRODUCTS, (32, 259)))
    queries = []
    for r in rows:
        entry, N, K = PRODUCTS[r["product"]]
        assert (r["entry"], r["N"], r["K"]) == (entry, N, K)
        queries.append((entry, r["M"], N, K) + _ws(r["M"], 2 * N if entry == "swiglu_w4" else N))
    keys = ("family", "bm", "nbuf", "splits", "tps", "in_kernel", "direct_in_kernel")
    for r, got in zip(rows, direct(queries, 256)):
        assert {k: got[k] for k in keys} == {k: r[k] for k in keys}, "%s M=%d: %s" % (r["product"], r["M"], got)
    by = {(r["product"], r["M"]): r for r in rows}
    # 259 rows: q/k/v and down_proj on the whole-M kernel, gate/up fused, o_proj on glds<96, 128, 2> -- all four in the kernel
    assert [(by[(p, 259)]["family"], by[(p, 259)]["direct_in_kernel"]) for p in ("qkv", "down", "gate_up")] == \
        [("whole_m_288", 1), ("whole_m_288", 1), ("fused", 1)]
    o = by[("o", 259)]
    assert (o["family"], o["bm"], o["nbuf"], o["direct_in_kernel"]) == ("glds", 96, 2, 1)
    # 32 rows: as the plain table
    golden_plain = {(r["product"], r["M"]): r for r in json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_w4_routes.json")))}
    for p in PRODUCTS:
        r, g = by[(p, 32)], golden_plain[(p, 32)]
        assert all(r[k] == g[k] for k in ("family", "bm", "nbuf", "splits", "tps", "in_kernel")) and r["direct_in_kernel"] == g["in_kernel"] == 1
    # and the plain answers of this CLI are the plain CLI's
    for g, pl in zip(direct(queries, 256), plain(queries, 256)):
        assert all(g[k] == pl[k] for k in KEYS[:7]), (g, pl)


@pytest.mark.parametrize("cus", (8, 104, 256, 304))
def test_structure_over_a_shape_sweep(clis, cus):
    direct, plain, bf16 = clis
    Ms = (1, 33, 64, 65, 224, 225, 259, 272, 273, 383, 384, 518, 1036, 2072)
    Ns = (64, 1000, 4096, 12288, 28672)
    Ks = (32, 64, 96, 160, 512, 1024, 4096, 4128, 14336)
    queries = []
    for M, N, K in itertools.product(Ms, Ns, Ks):
        for have_ws, ws_bytes in ((0, 0), (1, 32 * M * N), (1, 4 * M * N)):
            queries.append(("gemm_w4", M, N, K, have_ws, ws_bytes))
    got = direct(queries, cus)
    ref = bf16([("gemm",) + q[1:] for q in queries], cus)
    pl = plain(queries, cus)
    seen = set()
    for q, g, r, p in zip(queries, got, ref, pl):
        what = "%s at %d CUs: %s" % (q, cus, g)
        K = q[3]
        assert {k: g[k] for k in r} == r, what + " -- the bf16 product takes %s" % r  # the route is gemm_route's own
        assert g["in_kernel"] == p["in_kernel"], what
        if g["direct_in_kernel"]:
            assert K % 64 == 0 and g["family"] != "tile_256", what
        if g["in_kernel"]:
            assert g["direct_in_kernel"], what
        if g["in_kernel"] != g["direct_in_kernel"]:
            assert g["family"] == "whole_m_288" and g["fits"] and g["tps"] <= MAX_TILES and g["nk"] >= 4, what
        if g["family"] == "whole_m_288":  # the family's own requirements (K % 64 == 0, >= 4 tiles) hold: the fit rule decides
            assert g["direct_in_kernel"] == g["fits"] == int(g["tps"] <= MAX_TILES), what
        seen.add((g["family"], g["in_kernel"], g["direct_in_kernel"]))
    assert {("glds", 1, 1), ("glds", 0, 0), ("tile_256", 0, 0)} <= seen
    assert cus == 8 or {("whole_m_288", 0, 1), ("whole_m_288", 0, 0)} <= seen  # (K = 14336 without a workspace: 224 tiles do not fit)
    # SwiGLU: the fused shape multiplies the codes when its K tiles fit; every other shape is the plain product of the stacked matrix
    sq = [("swiglu_w4", M, I, K) + _ws(M, 2 * I) for M, I, K in itertools.product((37, 225, 259, 272, 273, 600), (1408, 8192, 14336),
                                                                                 (256, 512, 4096, 4128, 12288))]
    sg = direct(sq, cus)
    fused = bf16([("swiglu",) + q[1:] for q in sq], cus)
    stacked = direct([("gemm_w4", q[1], 2 * q[2]) + q[3:] for q in sq], cus)
    for q, g, f, s in zip(sq, sg, fused, stacked):
        if f == "fused":
            assert (g["family"], g["in_kernel"], g["direct_in_kernel"]) == ("fused", 0, int(q[3] // 64 <= MAX_TILES)), (q, g)
            assert q[3] % 64 == 0 and q[3] // 64 >= 4
        else:
            assert g == s, (q, g, s)


def test_a_scale_range_that_does_not_fit_expands(clis):
    """(259, 16384, K) without a workspace is un-split on the whole-M kernel: 181 K tiles are the last that fit"""
    direct, _, _ = clis
    a, b, c = direct([("gemm_w4", 259, 16384, 64 * t, 0, 0) for t in (181, 182, 192)], 256)
    for g, t in ((a, 181), (b, 182), (c, 192)):
        assert (g["family"], g["splits"], g["tps"], g["in_kernel"]) == ("whole_m_288", 1, t, 0), g
    assert (a["direct_in_kernel"], a["fits"]) == (1, 1)
    assert (b["direct_in_kernel"], b["fits"]) == (0, 0) and (c["direct_in_kernel"], c["fits"]) == (0, 0)
    # the fused form at such a K
    f = direct([("swiglu_w4", 259, 8192, 12288) + _ws(259, 16384)], 256)[0]
    assert (f["family"], f["in_kernel"], f["direct_in_kernel"]) == ("fused", 0, 0)


def test_the_gpu_cases_name_the_routes_of_256_cus(clis):
    """tests/test_gpu_gemm_w4_direct.py asserts these on the device; here the tables themselves are checked where no GPU is needed"""
    from tests import test_gpu_gemm_w4_direct as G

    direct, _, _ = clis
    q = [("gemm_w4", M, N, K) + _ws(M, N) for (M, N, K), _, _ in G.PRODUCTS]
    for ((shape, route, dik), g) in zip(G.PRODUCTS, direct(q, 256)):
        assert ((g["family"], g["bm"], g["nbuf"], g["splits"]), g["direct_in_kernel"]) == (route, dik), (shape, g)
    q = [("swiglu_w4", M, I, K) + _ws(M, 2 * I) for M, I, K, _, _ in G.SWIGLU]
    for ((M, I, K, route, dik), g) in zip(G.SWIGLU, direct(q, 256)):
        assert ((g["family"], g["bm"], g["nbuf"], g["splits"]), g["direct_in_kernel"]) == (route, dik), ((M, I, K), g)
