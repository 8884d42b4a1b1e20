"""The attention kernels' route choice (spatialrgpt_amd/csrc/attn_route.h) on the CPU: flash or one-wave kernel for a prefill call,
MFMA or VALU kernel for a decode call, template instance, grid, splits and keys per block, the three refusals, and the layout of the
decode workspace.  Every route computes the same result within tolerance, so a slipped threshold only shows as a slower step (or as
other bits).  `tests/golden/attn_routes.json` holds, for the prefill and decode attention of the three LLM geometries and of both
towers at 1 / 4 / 8 requests, for every parametrisation of tests/test_gpu_attention_ragged.py and tests/attn_kat.py, for the edges of
each rule and for each refusal, what the selection code answered before it moved into the header, at 256 CUs
(profiles/NOTEBOOK.md says how it was made); the header -- compiled alone into tests/attn_route_cli.cpp, no HIP -- has to reproduce
every row."""
import itertools
import json
import os

import pytest

from tests.util import build_attn_route_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_MAX, CHUNK_MAX = 64, 256
ERR_UNSUPPORTED = -2  # SRGPT_ERR_UNSUPPORTED
CTYPE = {"bf16": "bf16_t", "f32": "float"}


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return build_attn_route_cli(tmp_path_factory.mktemp("attn_route"))


def query_of(r):
    if r["what"] == "decode":
        return ("decode", r["dtype"], r["B"], r["Hq"], r["Hkv"], r["D"], r["max_pos"])
    return ("prefill", r["dtype"], r["D"], r["Tq"], r["Tk"], r["Hq"], r["B"], *r["strides"], r["qkv_aligned16"], r["o_aligned8"],
            r["scale_positive"])


def launch_of(row, got):
    """the one place that says which kernel (name with template arguments), grid and block a route means -- or, for a refused decode
    call, the message and code srgpt_decode_attention answers with"""
    if row["what"] == "prefill":
        name = "flash_bf16_kernel<%d, %s>" % (got["hdp"], ("false", "true")[row["causal"]]) if got["family"] == "flash" else \
               "simple_attn_kernel<%s>" % CTYPE[row["dtype"]]
        return dict(kernel=name, grid=got["grid"], block=got["block"])
    if got["status"] != "ok":
        msg = {"max_pos": "max_pos %d exceeds %d cached positions" % (row["max_pos"], SPLIT_MAX * CHUNK_MAX),
               "head_dim": "head_dim %d not supported (16,32,64,128)" % row["D"],
               "group": "heads/kv_heads = %d not supported (1,2,4,8)" % got["G"]}[got["status"]]
        return dict(refusal="srgpt_decode_attention: " + msg, code=ERR_UNSUPPORTED)
    name = "decode_mfma_kernel<%d>" % got["G"] if got["family"] == "decode_mfma" else \
           "decode_split_kernel<%s, %d, %d>" % (CTYPE[row["dtype"]], row["D"], got["G"])
    return dict(kernel=name, grid=[got["n_attn"], 1, 1], block=256, nsplit=got["nsplit"], kpb=got["kpb"])


def test_every_recorded_launch_is_reproduced(cli):
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "attn_routes.json")))
    assert {r["cus"] for r in rows} == {256}
    seen, refusals = set(), set()
    for row, got in zip(rows, cli([query_of(r) for r in rows], 256)):
        launch = launch_of(row, got)
        want = {k: row[k] for k in ("kernel", "grid", "block", "nsplit", "kpb", "refusal", "code") if k in row}
        assert launch == want, "%s: %s" % (row, got)
        seen.add(launch.get("kernel"))
        refusals.add(got.get("status"))
    # the models' attention: 3 LLM geometries x B 1 / 4 / 8 x max_pos 512 / 2048 / 4096 (decode and prefill), 2 towers x B 1 / 4 / 8
    assert sum(r["name"].endswith(" decode") for r in rows) == 27 and sum(" prefill max_pos " in r["name"] for r in rows) == 27
    assert sum(r["name"].endswith(" tower") for r in rows) == 6
    # every reachable instance: 4 + 28 decode, 8 flash, 2 one-wave
    want = {"decode_mfma_kernel<%d>" % g for g in (1, 2, 4, 8)} | {"simple_attn_kernel<bf16_t>", "simple_attn_kernel<float>"} | \
           {"flash_bf16_kernel<%d, %s>" % (h, c) for h in (32, 64, 96, 128) for c in ("false", "true")} | \
           {"decode_split_kernel<%s, %d, %d>" % (t, d, g) for t in ("bf16_t", "float") for d in (16, 32, 64, 128) for g in (1, 2, 4, 8)
            if (t, d) != ("bf16_t", 128)}
    assert seen - {None} == want
    assert refusals == {"ok", None, "max_pos", "head_dim", "group"}


@pytest.mark.parametrize("cus", [8, 104, 256, 304])
def test_structure_of_every_decode_route(cli, cus):
    MAX_POS = (1, 63, 64, 65, 512, 513, 4096, 4097, 8192, 16384, 16385)
    queries = [("decode", dtype, B, G * Hkv, Hkv, D, mp)
               for dtype, D, G, Hkv, B, mp in itertools.product(("bf16", "f32"), (16, 20, 32, 64, 128, 256), range(1, 10), (1, 2, 8, 32),
                                                                (1, 2, 3, 8, 40), MAX_POS)]
    families = set()
    for (_, dtype, B, Hq, Hkv, D, mp), r in zip(queries, cli(queries, cus)):
        what = "%s B=%d Hq=%d Hkv=%d D=%d max_pos=%d: %s" % (dtype, B, Hq, Hkv, D, mp, r)
        G = Hq // Hkv
        assert r["G"] == G and 1 <= r["nsplit"] <= SPLIT_MAX and r["n_attn"] == Hkv * r["nsplit"] * B, what
        mfma = dtype == "bf16" and D == 128 and G in (1, 2, 4, 8)
        assert (r["family"] == "decode_mfma") == mfma, what
        if mfma:
            assert r["status"] == "ok" and r["nsplit"] * r["kpb"] >= mp and r["kpb"] % 64 == 0 and r["kpb"] >= 64, what
        else:
            assert r["kpb"] == 0, what
            assert (-(-mp // r["nsplit"]) <= CHUNK_MAX) == (r["status"] != "max_pos"), what
            assert r["nsplit"] <= max(16 if B == 1 else 8, -(-mp // CHUNK_MAX)), what
        if r["status"] == "ok":
            assert D in (16, 32, 64, 128) and G in (1, 2, 4, 8), what
            families.add(r["family"])
        elif r["status"] == "head_dim":
            assert D not in (16, 32, 64, 128), what
        elif r["status"] == "group":
            assert D in (16, 32, 64, 128) and G not in (1, 2, 4, 8), what
        # the workspace: include/srgpt.h (B * Hq * 64 * (D + 2) partial floats, then the tickets; tests/test_capi_symbols.py pins
        # srgpt_decode_attn_ws_floats(32, 64, 128) = 32 * 64 * 130 + 32) and ops.decode_attention_ws, which slices at the same offset
        assert r["partial_floats"] == B * Hq * SPLIT_MAX * (D + 2) and r["tickets_reserved"] == B * Hq, what
        assert r["ws_floats"] == r["partial_floats"] + r["tickets_reserved"], what
        assert r["tickets_used"] == B * Hkv <= r["tickets_reserved"] and r["last_ticket"] == r["tickets_used"] - 1, what
        # the last group's last row ends where the partials end: groups of G heads x 64 rows of D + 2 floats, dense, in (b, hk) order
        assert r["last_group"] == (B * Hkv - 1) * G * SPLIT_MAX * (D + 2), what
        assert r["last_row"] == ((G - 1) * SPLIT_MAX + r["nsplit"] - 1) * (D + 2), what
        assert r["last_group"] + (G * SPLIT_MAX) * (D + 2) == r["partial_floats"], what
    assert families == {"decode_mfma", "decode_valu"}


def test_structure_of_every_prefill_route(cli):
    queries, keys = [], []
    for dtype, D, Tq, Tk, pad, a16, o8, sp in itertools.product(("bf16", "f32"), (*range(8, 137), 192, 256), (1, 64, 65, 729), (1, 130, 4096),
                                                                (0, 4, 8), (0, 1), (0, 1), (0, 1)):
        Hq, Hkv, B = 4, 2, 3
        ts, kts = Hq * D + pad, Hkv * D + pad
        queries.append(("prefill", dtype, D, Tq, Tk, Hq, B, Tq * ts, ts, D, Tk * kts, kts, D, Tk * kts, kts, D, a16, o8, sp))
        keys.append((dtype, D, Tq, Hq, B, ts, kts, a16, o8, sp))
    families = set()
    for (dtype, D, Tq, Hq, B, ts, kts, a16, o8, sp), r in zip(keys, cli(queries)):
        what = "%s: %s" % ((dtype, D, Tq, Hq, B, ts, kts, a16, o8, sp), r)
        flash = dtype == "bf16" and D % 8 == 0 and D <= 128 and ts % 8 == 0 and kts % 8 == 0 and a16 and o8 and sp
        assert (r["family"] == "flash") == bool(flash), what
        if flash:
            assert r["hdp"] in (32, 64, 96, 128) and r["hdp"] - 32 < D <= r["hdp"], what
            assert r["grid"] == [-(-Tq // 64), Hq, B] and r["block"] == 256, what
        else:
            assert r["grid"] == [Tq, Hq, B] and r["block"] == 64, what
        families.add(r["family"])
    assert families == {"flash", "one_wave"}
