"""The MXFP4 additions to the C ABI (include/srgpt.h: srgpt_gemv_w4, srgpt_dequant_mxfp4, the trailing fields of srgpt_llm_weights)
and to the decode products' routes (spatialrgpt_amd/csrc/gemv_route.h: gemv_w4_route, gemv_w4_launch), without a GPU."""
import ctypes
import json
import os
import re
import subprocess

import pytest

from tests.util import ROOT, _build_route_cli

W4_FIELDS = ["wqkv4", "wqkv4_scale", "wo4", "wo4_scale", "wgu4", "wgu4_scale", "wdown4", "wdown4_scale"]


def test_new_symbols_are_exported_under_abi_9():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    assert lib.srgpt_abi_version() == _lib.ABI_VERSION == 9
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srgpt.h")).read(), flags=re.S)
    for name in ("srgpt_gemv_w4", "srgpt_dequant_mxfp4"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in include/srgpt.h"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {"srgpt_gemv_w4", "srgpt_dequant_mxfp4"} <= {ln.split()[-1] for ln in out.splitlines() if ln.split()}


def test_weight_struct_gains_trailing_fields_in_header_order():
    from spatialrgpt_amd import _lib

    names = [f[0] for f in _lib.LlmWeights._fields_]
    assert names[-8:] == W4_FIELDS and names[-9] == "pk_rows_down"
    src = open(os.path.join(ROOT, "include", "srgpt.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} srgpt_llm_weights;", src).group(1), flags=re.S)
    decl = [re.findall(r"([A-Za-z_0-9]+)\s*$", part.strip())[0] for d in body.split(";") if d.strip() for part in d.split(",")]
    assert decl == names
    # eight pointers behind the four ints that ended the struct before
    assert ctypes.sizeof(_lib.LlmWeights) == _lib.LlmWeights.pk_rows_qkv.offset + 16 + 8 * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.LlmWeights.wqkv4.offset == _lib.LlmWeights.pk_rows_qkv.offset + 16
    w = _lib.LlmWeights()
    assert all(not getattr(w, f) for f in W4_FIELDS)  # zero-initialised = the formats that existed


def test_entry_points_validate_on_the_host():
    """argument errors are detected before any launch (and before the device is asked anything): safe without a GPU"""
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    ok = dict(x=16, W4=16, sc=16, out=16)
    for missing in ok:
        a = dict(ok, **{missing: None})
        rc = lib.srgpt_gemv_w4(a["x"], a["W4"], a["sc"], None, 0.0, None, a["out"], 1, 8, 64, 0, 0, None)
        assert rc == _lib.ERR_ARG and b"null" in lib.srgpt_last_error(), missing
    rc = lib.srgpt_gemv_w4(16, 16, 16, None, 0.0, None, 16, 1, 8, 48, 0, 0, None)  # K = 48: half a block
    assert rc == _lib.ERR_ARG and b"multiple of 32" in lib.srgpt_last_error()
    rc = lib.srgpt_gemv_w4(16, 16, 16, None, 0.0, 16, 16, 1, 8, 64, 1, 0, None)  # swiglu + residual
    assert rc == _lib.ERR_ARG and b"swiglu" in lib.srgpt_last_error()
    rc = lib.srgpt_gemv_w4(16, 16, 16, None, 0.0, None, 16, 1, 8, 64, 1, 1, None)  # swiglu + out_f32
    assert rc == _lib.ERR_ARG and b"swiglu" in lib.srgpt_last_error()
    rc = lib.srgpt_gemv_w4(16, 16, 16, None, 0.0, None, 16, 0, 8, 64, 0, 0, None)  # no rows
    assert rc == _lib.ERR_ARG and b"shape" in lib.srgpt_last_error()
    for args in ((None, 16, 16), (16, None, 16), (16, 16, None)):
        rc = lib.srgpt_dequant_mxfp4(*args, 8, 64, None)
        assert rc == _lib.ERR_ARG and b"null" in lib.srgpt_last_error()
    rc = lib.srgpt_dequant_mxfp4(16, 16, 16, 8, 48, None)
    assert rc == _lib.ERR_ARG and b"multiple of 32" in lib.srgpt_last_error()
    rc = lib.srgpt_dequant_mxfp4(16, 16, 16, 0, 64, None)
    assert rc == _lib.ERR_ARG and b"shape" in lib.srgpt_last_error()


def test_incomplete_mxfp4_weights_are_refused_before_any_launch():
    """llm_format: wqkv4 set means MXFP4, and then the other three matrices, every block-scale array, the fp8 lm_head and a bf16
    dtype must be there -- checked on the host by every LLM entry point"""
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    w, st = _lib.LlmWeights(), _lib.LlmState()
    w.dtype, w.hidden, w.inter, w.layers, w.heads, w.kv_heads, w.head_dim, w.vocab = _lib.BF16, 64, 128, 1, 2, 2, 32, 100
    one = (_lib.vp * 1)(16)
    for f in ("kcache", "vcache", "pos", "tok", "out_ids", "step", "ws", "logits"):
        setattr(st, f, 16)
    st.batch, st.max_pos, st.max_new, st.ws_tokens = 1, 64, 4, 8
    w.wqkv4 = one
    rc = lib.srgpt_llm_decode_step(ctypes.byref(w), ctypes.byref(st), None)
    assert rc == _lib.ERR_ARG and b"MXFP4" in lib.srgpt_last_error()
    for f in W4_FIELDS:
        setattr(w, f, one)
    rc = lib.srgpt_llm_prefill(ctypes.byref(w), ctypes.byref(st), 16, 4, None, None, None)  # no fp8 lm_head
    assert rc == _lib.ERR_ARG and b"lm_head" in lib.srgpt_last_error()
    w.lm_head8, w.lm_head_scale = 16, 16
    w.dtype = _lib.F32
    rc = lib.srgpt_llm_decode_step(ctypes.byref(w), ctypes.byref(st), None)
    assert rc == _lib.ERR_ARG and b"bf16" in lib.srgpt_last_error()
    w.dtype, w.inter = _lib.BF16, 144  # not a multiple of 32
    rc = lib.srgpt_llm_decode_step(ctypes.byref(w), ctypes.byref(st), None)
    assert rc == _lib.ERR_ARG and b"multiples of 32" in lib.srgpt_last_error()
    w.inter, w.wqkv8 = 128, one  # both quantised formats at once
    rc = lib.srgpt_llm_decode_step(ctypes.byref(w), ctypes.byref(st), None)
    assert rc == _lib.ERR_ARG and b"both" in lib.srgpt_last_error()


def test_workspace_grows_by_the_scratch_under_the_format_only():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    w = _lib.LlmWeights()
    w.dtype, w.hidden, w.inter, w.layers, w.heads, w.kv_heads, w.head_dim, w.vocab = _lib.BF16, 512, 1408, 3, 8, 2, 64, 1000
    base = lib.srgpt_llm_ws_bytes(ctypes.byref(w), 3, 40)
    w.wqkv8 = (_lib.vp * 3)()
    assert lib.srgpt_llm_ws_bytes(ctypes.byref(w), 3, 40) == base  # fp8: unchanged
    w.wqkv8 = None
    w.wqkv4 = (_lib.vp * 3)()
    # one bf16 scratch for the largest matrix (gate / up: 2 * 1408 x 512), rounded up to the carve's 256 bytes
    assert lib.srgpt_llm_ws_bytes(ctypes.byref(w), 3, 40) == base + (2 * 1408 * 512 * 2 + 255) // 256 * 256


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    exe = _build_route_cli(tmp_path_factory.mktemp("gemv_w4_route"), "gemv_w4_route_cli")

    def run(queries, cus=256):
        text = "".join("%d %d %d %d\n" % tuple(q) for q in queries)
        out = subprocess.run([exe, str(int(cus))], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        assert len(out) == len(queries)
        res = []
        for ln in out:
            head, *passes = ln.split(" | ")
            family, chunk, cols = head.split()
            res.append(dict(family=family, chunk=int(chunk), unit_cols=int(cols),
                            launches=[dict(zip(("rows", "B", "NX", "NIT", "grid", "lds", "raise"), map(int, p.split()))) for p in passes]))
        return res

    return run


def test_recorded_routes_of_the_decode_step_are_reproduced(cli):
    """tests/golden/gemv_w4_routes.json: the four products of the decode step (Llama-3-8B geometry) at 1 .. 4, 5 and 16 rows, 256 CUs"""
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "gemv_w4_routes.json")))
    assert {(r["product"], r["rows"]) for r in rows} == {(p, n) for p in ("qkv", "o_proj", "gate_up", "down") for n in (1, 2, 3, 4, 5, 16)}
    got = cli([(r["rows"], r["N"], r["K"], r["swiglu"]) for r in rows], 256)
    for want, g in zip(rows, got):
        assert g == {k: want[k] for k in ("family", "chunk", "unit_cols", "launches")}, (want, g)


@pytest.mark.parametrize("cus", [8, 104, 256, 304])
def test_structure_of_every_route(cli, cus):
    queries = [(rows, N, K, sw) for rows in (*range(1, 10), 16, 17) for N in (1, 3, 7, 64, 4096, 14336, 40000)
               for K in (32, 2048, 2080, 4096, 14336) for sw in (0, 1)]
    for (rows, N, K, sw), r in zip(queries, cli(queries, cus)):
        what = "rows=%d N=%d K=%d swiglu=%d: %s" % (rows, N, K, sw, r)
        assert r["family"] == "gemv_w4" and r["chunk"] == min(rows, 4) and r["unit_cols"] == 2, what
        assert [p["rows"] for p in r["launches"]] == [4] * (rows // 4) + ([rows % 4] if rows % 4 else []), what  # every pass on this kernel
        for p in r["launches"]:
            assert p["B"] == p["rows"] and p["lds"] == p["rows"] * K * 2 and p["raise"] == (p["lds"] > 48 * 1024), what
            assert p["lds"] <= 150 * 1024, what  # 4 rows of K = 14336 fit the cap
            assert p["NX"] == (2 if p["rows"] * K // 8 <= 512 else 8) and p["NIT"] == (K // 32 + 63) // 64, what
            units = (N + 1) // 2
            assert p["grid"] == max(1, min((units + 3) // 4, cus * (1 if p["lds"] > 70 * 1024 else 2))), what
