"""Which W4 products multiply their MXFP4 codes inside the GEMM kernel, and which expand them first
(spatialrgpt_amd/csrc/gemm_route.h: gemm_w4_in_kernel, gemm_swiglu_w4_in_kernel), on the CPU.  A W4 product takes the route of the
bf16 product of the same shape -- gemm_route is asked unchanged -- so the route printed by tests/gemm_w4_route_cli.cpp has to equal
the one tests/gemm_route_cli.cpp prints, and only the direct-to-LDS family with whole 64-column K tiles answers "in the kernel".
tests/golden/gemm_w4_routes.json pins both answers at 256 CUs, with the workspace ops.py hands over, for the four products of the
8B layer (q/k/v 6144 x 4096, o_proj 4096 x 4096, gate / up 2 x 14336 x 4096, down_proj 4096 x 14336) at the row counts of the decode
verify steps, the append, the bs = 1 prefill and its edges, and the batched prefills."""
import itertools
import json
import os
import subprocess

import pytest

from tests.util import _build_route_cli, build_gemm_route_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = (1, 5, 32, 224, 225, 259, 272, 273, 518, 1036)
PRODUCTS = {"qkv": ("gemm_w4", 6144, 4096), "o": ("gemm_w4", 4096, 4096), "gate_up": ("swiglu_w4", 14336, 4096),
            "down": ("gemm_w4", 4096, 14336)}


@pytest.fixture(scope="module")
def clis(tmp_path_factory):
    d = tmp_path_factory.mktemp("gemm_w4_route")
    exe = _build_route_cli(d, "gemm_w4_route_cli")

    def w4(queries, cus):
        text = "".join("%s %d %d %d %d %d\n" % tuple(q) for q in queries)
        out = subprocess.run([exe, str(int(cus))], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        assert len(out) == len(queries)
        res = []
        for ln in out:
            f = ln.split()
            assert len(f) == 7, ln
            res.append(dict(family=f[0], bm=int(f[1]), nbuf=int(f[2]), splits=int(f[3]), tps=int(f[4]), nk=int(f[5]), in_kernel=int(f[6])))
        return res

    return w4, build_gemm_route_cli(d)


def _ws(M, rows):
    """ops.py's workspace for an [M, rows] product: 8 fp32 slabs up to 2^24 elements"""
    return int(M * rows <= 1 << 24), 32 * M * rows


def test_the_8b_products_are_pinned(clis):
    w4, bf16 = clis
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_w4_routes.json")))
    assert {(r["product"], r["M"]) for r in rows} == set(itertools.product(PRODUCTS, MS))
    queries = []
    for r in rows:
        entry, N, K = PRODUCTS[r["product"]]
        assert (r["entry"], r["N"], r["K"]) == (entry, N, K)
        queries.append((entry, r["M"], N, K) + _ws(r["M"], 2 * N if entry == "swiglu_w4" else N))
    keys = ("family", "bm", "nbuf", "splits", "tps", "in_kernel")
    for r, got in zip(rows, w4(queries, 256)):
        assert {k: got[k] for k in keys} == {k: r[k] for k in keys}, "%s M=%d: %s" % (r["product"], r["M"], got)
    by = {(r["product"], r["M"]): r for r in rows}
    # the 32-row append: every product on glds<64, 128, 2>, split 3 .. 8 ways, codes in the kernel
    for p in PRODUCTS:
        r = by[(p, 32)]
        assert (r["family"], r["bm"], r["nbuf"], r["in_kernel"]) == ("glds", 64, 2, 1) and 3 <= r["splits"] <= 8, r
    # the 259-row prefill: o_proj on glds<96, 128, 2> with 4 splits in the kernel; the other three on the whole-M kernel, which has
    # no W4 mode and expands
    assert {k: by[("o", 259)][k] for k in keys} == dict(family="glds", bm=96, nbuf=2, splits=4, tps=16, in_kernel=1)
    assert [(by[(p, 259)]["family"], by[(p, 259)]["in_kernel"]) for p in ("qkv", "gate_up", "down")] == \
        [("whole_m_288", 0), ("fused", 0), ("whole_m_288", 0)]
    # the bf16 products take the same routes
    plain = [(r, q) for r, q in zip(rows, queries) if r["family"] != "fused"]
    got = bf16([("gemm", q[1], 2 * q[2] if q[0] == "swiglu_w4" else q[2]) + q[3:] for _, q in plain], 256)
    for (r, _), g in zip(plain, got):
        assert (g["family"], g["bm"], g["nbuf"], g["splits"], g["tps"]) == (r["family"], r["bm"], r["nbuf"], r["splits"], r["tps"]), r
    fused = [q for r, q in zip(rows, queries) if r["family"] == "fused"]
    assert bf16([("swiglu",) + q[1:] for q in fused], 256) == ["fused"] * len(fused) and len(fused) == 3


@pytest.mark.parametrize("cus", (8, 104, 256, 304))
def test_structure_over_a_shape_sweep(clis, cus):
    w4, bf16 = clis
    Ms = (1, 33, 64, 65, 224, 225, 259, 272, 273, 383, 384, 518, 1036, 2072)
    Ns = (64, 1000, 4096, 12288, 28672)
    Ks = (32, 64, 96, 160, 512, 1024, 4096, 4128, 14336)
    queries = []
    for M, N, K in itertools.product(Ms, Ns, Ks):
        for have_ws, ws_bytes in ((0, 0), (1, 32 * M * N), (1, 4 * M * N)):
            queries.append(("gemm_w4", M, N, K, have_ws, ws_bytes))
    got = w4(queries, cus)
    ref = bf16([("gemm",) + q[1:] for q in queries], cus)
    seen = set()
    for q, g, r in zip(queries, got, ref):
        what = "%s at %d CUs: %s" % (q, cus, g)
        assert {k: g[k] for k in r} == r, what + " -- the bf16 product takes %s" % r  # the route is gemm_route's own
        K = q[3]
        assert g["in_kernel"] == int(g["family"] == "glds" and K % 64 == 0), what
        if g["family"] == "tile_256" or K % 64 != 0:
            assert g["in_kernel"] == 0, what
        seen.add((g["family"], g["in_kernel"]))
    assert {("glds", 1), ("glds", 0), ("tile_256", 0)} <= seen
    assert cus == 8 or ("whole_m_288", 0) in seen
    # SwiGLU: the fused shape never multiplies codes; every other shape is the plain product of the stacked matrix
    sq = [("swiglu_w4", M, I, K) + _ws(M, 2 * I) for M, I, K in itertools.product((37, 225, 259, 272, 273, 600), (1408, 8192, 14336),
                                                                                 (256, 512, 4096, 4128))]
    sg = w4(sq, cus)
    fused = bf16([("swiglu",) + q[1:] for q in sq], cus)
    stacked = w4([("gemm_w4", q[1], 2 * q[2]) + q[3:] for q in sq], cus)
    for q, g, f, s in zip(sq, sg, fused, stacked):
        if f == "fused":
            assert (g["family"], g["in_kernel"]) == ("fused", 0), (q, g)
        else:
            assert g == s, (q, g, s)


def test_the_gpu_cases_name_the_routes_of_256_cus(clis):
    """tests/test_gpu_gemm_w4.py asserts these on the device; here the table itself is checked where no GPU is needed"""
    from tests import test_gpu_gemm_w4 as G

    w4, _ = clis
    q = [("gemm_w4", M, N, K) + _ws(M, N) for (M, N, K), _, _ in G.PRODUCTS]
    for ((shape, route, in_kernel), g) in zip(G.PRODUCTS, w4(q, 256)):
        assert ((g["family"], g["bm"], g["nbuf"], g["splits"]), g["in_kernel"]) == (route, in_kernel), (shape, g)
    assert {r for _, r, k in G.PRODUCTS if k} == {("glds", 64, 2, 1), ("glds", 64, 1, 1), ("glds", 96, 2, 1), ("glds", 96, 1, 1),
                                                  ("glds", 128, 1, 1), ("glds", 96, 2, 2), ("glds", 96, 2, 4), ("glds", 64, 2, 8)}
