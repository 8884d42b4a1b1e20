"""CPU: the route of srgpt_decode_attention_multi (attn_decode_multi_route, spatialrgpt_amd/csrc/attn_route.h) -- compiled alone into
tests/attn_route_multi_cli.cpp, no HIP.  Pinned: the MFMA family for bf16 / head_dim 128 with query head g of token t in column
t * G + g, so T <= 16 / G and T = cap + 1 is refused, and the kernel instance is the column count rounded up to 2 / 4 / 8 / 16; the key
ranges of the single-token route (64 keys per block up to 4096 cached positions, 128 at 8192); the workspace (T * Hq columns' partials, then B * Hq tickets); the composition for everything else."""
import subprocess

import pytest

from tests.util import _build_route_cli

SPLIT_MAX = 64


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    exe = _build_route_cli(tmp_path_factory.mktemp("attn_route_multi"), "attn_route_multi_cli")

    def run(queries):
        text = "".join(" ".join(str(x) for x in q) + "\n" for q in queries)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        assert len(out) == len(queries)
        names = ("G", "T", "cols", "nc", "nsplit", "kpb", "blocks", "ws_floats", "cap")
        return [dict(status=f[0], family=f[1], **dict(zip(names, map(int, f[2:])))) for f in (ln.split() for ln in out)]

    return run


# max_pos -> (nsplit, kpb) of the single-token MFMA route (tests/golden/attn_routes.json has the same pairs)
RANGES = {128: (2, 64), 4096: (64, 64), 8192: (64, 128)}


def test_multi_route_is_pinned(cli):
    Hkv, B, D = 2, 1, 128
    queries, want = [], []
    for G in (1, 2, 4, 8):
        cap = 16 // G
        for T in (2, cap, cap + 1):
            for max_pos, (nsplit, kpb) in RANGES.items():
                queries.append(("bf16", B, T, G * Hkv, Hkv, D, max_pos))
                want.append(dict(status="ok" if T <= cap else "columns", family="multi_mfma", G=G, T=T, cols=T * G,
                                 nc=0 if T > cap else next(c for c in (2, 4, 8, 16) if c >= T * G), nsplit=nsplit, kpb=kpb,
                                 blocks=Hkv * nsplit * B, ws_floats=B * T * G * Hkv * SPLIT_MAX * (D + 2) + B * G * Hkv, cap=cap))
    assert cli(queries) == want
    # the shipped geometries: Llama-3-8B (32 / 8 heads) takes 4 rows per step, a 32 / 32 model 16
    got = cli([("bf16", 1, 4, 32, 8, 128, 4096), ("bf16", 1, 5, 32, 8, 128, 4096), ("bf16", 1, 16, 32, 32, 128, 2048),
               ("bf16", 3, 2, 8, 2, 128, 384)])
    assert [(r["status"], r["cols"], r["blocks"]) for r in got] == [("ok", 16, 8 * 64), ("columns", 20, 8 * 64), ("ok", 16, 32 * 32),
                                                                   ("ok", 8, 2 * 6 * 3)]
    assert got[0]["ws_floats"] == 4 * 32 * 64 * 130 + 32 and got[3]["ws_floats"] == 3 * 2 * 8 * 64 * 130 + 3 * 8


def test_everything_else_is_the_composition(cli):
    queries = [("f32", 1, 3, 4, 2, 16, 512), ("f32", 2, 4, 8, 2, 128, 512), ("bf16", 1, 3, 8, 8, 64, 2048), ("bf16", 1, 40, 6, 2, 128, 512),
               ("f32", 1, 17, 32, 8, 128, 4096)]
    for (dtype, B, T, Hq, Hkv, D, max_pos), r in zip(queries, cli(queries)):
        assert r["status"] == "ok" and r["family"] == "composed" and (r["nc"], r["nsplit"], r["kpb"], r["blocks"]) == (0, 0, 0, 0), r
        assert r["G"] == Hq // Hkv and r["cols"] == T * r["G"] and r["ws_floats"] == B * T * Hq * SPLIT_MAX * (D + 2) + B * Hq, r
