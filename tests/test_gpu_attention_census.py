"""Which keys every attention kernel sees, exactly once: srgpt_attention, srgpt_attention_append, srgpt_decode_attention and
srgpt_decode_attention_multi on the census data of tests/attn_census.py -- every softmax weight is exactly 1 or underflows, V spells
the key's index, so an output row times its number of keys is a table of integer counts.  Each case runs the three query families
(uniform, lit at the first invisible key, lit at the last visible key) against the float64 masked softmax of include/srgpt.h's rule
under a DERIVED tolerance (two ulps of the output type, 2^-60 where the reference is 0; attn_census.REL / ZERO), decodes the census
(`round(out * n) == counts`, the message names the row and the keys that are missing, counted twice or extra), and first asserts,
through the route CLIs, that the call runs on the kernel family and instance the case is meant for.  tests/test_host_attn_census.py
proves on the CPU that this data tells each of ten wrong key selections from the right one by 8 tolerances or more.

Decode entries: identity RoPE tables, a finite lure in every cache row at or behind the row's position, NaN workspace partials and
zero tickets; after every launch the caches must equal, bit for bit, the caches before it with the T new rows in place, and the
tickets must be zero."""
import os
import subprocess

import pytest
import torch

from tests import attn_census as ac
from tests.test_gpu_kernels import DEV, _ops
from tests.util import _build_route_cli, build_attn_route_cli

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DT = {BF16: "bf16", F32: "f32"}


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _route_query(case):
    Hq, Hkv, D, B = case.Hq, case.Hkv, case.D, case.B or len(case.launches[0])
    if case.entry in ("attention", "append"):
        qs, ks = (case.Tq * Hq * D, Hq * D, D), (case.Tk * Hkv * D, Hkv * D, D)  # dense tensors, 16-byte aligned (asserted at the call)
        return ("prefill", DT[case.dtype], D, case.Tq, case.Tk, Hq, B, *qs, *ks, *ks, 1, 1, 1)
    if case.entry == "decode":
        return ("decode", DT[case.dtype], B, Hq, Hkv, D, case.max_pos)
    return (DT[case.dtype], B, case.T, Hq, Hkv, D, case.max_pos)


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """case id -> the kernel csrc/attn_route.h picks for the case's call on this device, in the form of Case.route: both route CLIs
    compiled and asked once for all cases"""
    d = tmp_path_factory.mktemp("attn_census_routes")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    one = [c for c in ac.CASES if c.entry != "multi"]
    got = {}
    for c, r in zip(one, build_attn_route_cli(d)([_route_query(c) for c in one], cus)):
        if c.entry == "decode":
            assert r["status"] == "ok", (c.id, r)
            got[c.id] = (r["family"], r["G"], r["nsplit"]) + ((r["kpb"],) if r["family"] == "decode_mfma" else ())
        else:
            got[c.id] = (r["family"], r["hdp"]) if r["family"] == "flash" else (r["family"],)
    multi = [c for c in ac.CASES if c.entry == "multi"]
    text = "".join(" ".join(str(x) for x in _route_query(c)) + "\n" for c in multi)
    out = subprocess.run([_build_route_cli(d, "attn_route_multi_cli")], input=text, capture_output=True, text=True, check=True).stdout
    lines = out.split("\n")[:-1]
    assert len(lines) == len(multi)
    for c, ln in zip(multi, lines):
        f = ln.split()  # STATUS FAMILY G T COLS NC NSPLIT KPB BLOCKS WS_FLOATS CAP
        assert f[0] == "ok", (c.id, ln)
        got[c.id] = (f[1], int(f[2]), int(f[5]), int(f[6]), int(f[7])) if f[1] == "multi_mfma" else (f[1],)
    return got


def _assert_route(case, routes):
    """the call runs on the kernel the case names -> a line for the profile note"""
    assert routes[case.id] == case.route, f"{case.id}: runs on {routes[case.id]}, meant for {case.route}"
    log = os.environ.get("SRGPT_CENSUS_ROUTES")  # the case list of profiles/attention_census.txt
    if log:
        with open(log, "a") as f:
            f.write("%-34s %-6s %s\n" % (case.id, "causal" if case.entry != "attention" or case.causal else "full", routes[case.id]))


def _prefill(ops, case, p):
    dt = case.dtype
    q, k, v = (t.to(dt).to(DEV) for t in (p.q, p.k, p.v))
    assert all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in (q, k, v))
    kv_len = None if case.kv_len is None else torch.tensor(case.kv_len, dtype=torch.int32).to(DEV)
    if case.entry == "attention":
        out = ops.attention(q, k, v, causal=case.causal, kv_len=kv_len)
    else:
        out = ops.attention_append(q, k, v, torch.tensor(case.q_pos0, dtype=torch.int32).to(DEV), kv_len=kv_len, Tk=case.Tk)
    torch.cuda.synchronize()
    err = ac.census_error(out, p, dt)
    assert err is None, err


def _decode(ops, case, p, tables, ws, tickets):
    dt, Hq, Hkv, D = case.dtype, case.Hq, case.Hkv, case.D
    kc, vc, k_want, v_want = ac.decode_caches(p, dt, "cpu")  # built on the host: the test launches nothing but the kernel under test
    kc, vc = kc.to(DEV), vc.to(DEV)
    pos = torch.tensor(p.q_pos0, dtype=torch.int32).to(DEV)
    if case.entry == "decode":
        out = ops.decode_attention(p.qkv[:, 0].to(dt).to(DEV), kc, vc, pos, *tables, Hq, Hkv, D, ws=ws)
    else:
        out = ops.decode_attention_multi(p.qkv.to(dt).to(DEV), kc, vc, pos, *tables, Hq, Hkv, D, ws=ws)
    torch.cuda.synchronize()
    err = ac.census_error(out, p, dt)
    assert err is None, err
    # the T new rows in place bit for bit (the identity tables make the k rows exact too), nothing else moved
    for now, want, name in ((kc.cpu(), k_want, "k"), (vc.cpu(), v_want, "v")):
        if not torch.equal(_bits(now), _bits(want)):
            where = (_bits(now) != _bits(want)).nonzero()[0].tolist()
            raise AssertionError(f"{p.what}: {name} cache differs at (row, kv head, position, channel) {where}")
    assert int(torch.count_nonzero(tickets.cpu())) == 0, ("tickets", p.what, tickets.tolist())


@pytest.mark.parametrize("case", ac.CASES, ids=[c.id for c in ac.CASES])
def test_census(case, routes):
    ops, L = _ops()
    _assert_route(case, routes)
    if case.entry in ("attention", "append"):
        for family in ac.FAMILIES:
            for p in case.problems(family):
                _prefill(ops, case, p)
        return
    B, Hq, D = len(case.launches[0]), case.Hq, case.D
    assert all(len(pos) == B for pos in case.launches)
    half = (case.max_pos, D // 2)
    tables = (torch.ones(half, dtype=case.dtype).to(DEV), torch.zeros(half, dtype=case.dtype).to(DEV))  # RoPE: the identity
    # the workspace (include/srgpt.h): the partials NaN, behind them B * Hq tickets, zero; one workspace for all launches
    n = int(L.load().srgpt_decode_attn_ws_floats(B, Hq, D) if case.entry == "decode" else
            L.load().srgpt_decode_attn_multi_ws_floats(B, case.T, Hq, D))
    assert n == B * case.T * Hq * 64 * (D + 2) + B * Hq
    host = torch.full((n,), float("nan"), dtype=F32)
    host[n - B * Hq:] = 0.0
    ws = host.to(DEV)
    tickets = ws[n - B * Hq:].view(torch.int32)
    for family in ac.FAMILIES:
        for p in case.problems(family):
            _decode(ops, case, p, tables, ws, tickets)
