"""llm_weight_format="mxfp4_w4a8" through the engine, at the geometry of
tests/test_gpu_fp8_mfma.py::test_w8a8_prefill_vs_oracle_restatement (hidden 512, inter 1408, 8 heads of 64, 2 kv heads, 3 layers,
T = 37, batch 1 and 3): the prefill (per-token e4m3 activations x MXFP4 codes, srgpt_gemm_w4a8) against the oracle's
llama_forward(act_quant=fp8_rowwise_fake_quant) on the MXFP4-dequantised layer weights and the fp8-dequantised lm_head, at that
test's bars; the decode steps after it, which are the "mxfp4" engine's bit for bit; the append prefill; what the engine routes and
what its workspace holds; the packed 2-row decode step."""
import ctypes as C
import functools

import pytest
import torch

from tests.test_gpu_mxfp4 import KW, dequantised_state_dict
from tests.util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
H, T, G = KW["hidden"], 37, 3


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == BF16 else t.contiguous().view(torch.int32)


def _x(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 0.5).to(BF16)


@functools.lru_cache(maxsize=None)
def _setup():
    """(oracle config, the oracle's weights = what both engines multiply, the mxfp4_w4a8 engine, an mxfp4 engine on the same weights)"""
    from oracle import srgpt_oracle as so
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine

    ocfg = so.SrgptConfig(**KW)
    w = so.synth_weights(ocfg, seed=3, dtype=BF16)
    eng = SrgptEngine(SrgptConfig(**KW), dict(w), device=DEV, dtype=BF16, rope_positions=512, llm_weight_format="mxfp4_w4a8")
    engm = SrgptEngine(SrgptConfig(**KW), dict(w), device=DEV, dtype=BF16, rope_positions=512, llm_weight_format="mxfp4")
    for k in ("wqkv", "wo", "wgu", "wdown"):  # the same codes and scales as "mxfp4"
        for a, b in zip(eng.w.llm_q4[k][0] + eng.w.llm_q4[k][1], engm.w.llm_q4[k][0] + engm.w.llm_q4[k][1]):
            assert torch.equal(a, b), k
    return ocfg, dequantised_state_dict(eng, w), eng, engm


@pytest.mark.parametrize("batch", [1, 3])
def test_prefill_vs_oracle_then_the_decode_steps_of_the_mxfp4_engine(batch):
    from oracle import srgpt_oracle as so

    ocfg, wq, eng, engm = _setup()
    assert eng.w.fp8_act is True and eng.w.llm_weight_format == "mxfp4"
    x = _x((batch, T, H), 5)
    st = eng.new_state(batch, 64, G + 1)
    _, all_logits, _ = eng.prefill(x.to(DEV), max_new=G + 1, all_logits=True, state=st)
    pos = torch.arange(T)[None].expand(batch, -1)
    kv = so.KVCache(ocfg.layers)
    ref = so.llama_forward(wq, ocfg, x, pos, kv, act_quant=so.fp8_rowwise_fake_quant)
    tol = 3e-2 * float(ref.abs().max())
    assert_close(all_logits, ref, tol, 0, "W4A8 prefill logits vs the oracle's restatement")
    assert_close(st.logits, ref[:, -1], tol, 0, "last-position logits vs the oracle's restatement")
    # what the activation quantisation costs against "mxfp4" (the same weights, bf16 activations)
    stm = engm.new_state(batch, 64, G + 1)
    _, all_m, _ = engm.prefill(x.to(DEV), max_new=G + 1, all_logits=True, state=stm)
    dev = float((all_logits.float() - all_m.float()).pow(2).mean().sqrt() / all_m.float().pow(2).mean().sqrt())
    print(f"\nW4A8 vs W4A16 prefill logits: relative rms deviation {dev:.4f} (batch {batch})")
    assert 0 < dev < 0.15, f"W4A8 prefill deviates {dev:.3f} rms from W4A16"
    # decode: W4A16 on the cache the W4A8 prefill wrote.  Teacher-forced against the oracle doing the same, and bit for bit the
    # "mxfp4" engine's step on a copy of that cache with the same token
    stm.kcache.copy_(st.kcache)
    stm.vcache.copy_(st.vcache)
    g = torch.Generator().manual_seed(9)
    for s in range(G):
        tok = torch.randint(3, 900, (batch, 1), generator=g)
        got = eng.step(st, tok.to(DEV))
        emb = torch.nn.functional.embedding(tok, wq["llm.model.embed_tokens.weight"])
        r = so.llama_forward(wq, ocfg, emb, torch.full((batch, 1), T + s), kv)
        assert_close(got, r[:, 0], tol, 0, f"W4A16 decode step {s} on the W4A8-written cache vs the oracle")
        gotm = engm.step(stm, tok.to(DEV))
        assert torch.equal(_bits(got), _bits(gotm)), f"decode step {s}: not the mxfp4 engine's bits"
        assert torch.equal(_bits(st.kcache[:, :, :, :T + s + 1]), _bits(stm.kcache[:, :, :, :T + s + 1])), f"decode step {s}: k cache"
    from spatialrgpt_amd import _lib as L, ops
    assert L.load().srgpt_llm_decode_sync_state(C.byref(eng.w.llm), C.byref(st.c), ops._stream()) == 0


def test_append_of_8_rows_over_37_cached_rows_vs_oracle():
    from oracle import srgpt_oracle as so

    ocfg, wq, eng, _ = _setup()
    x = _x((1, T + 8, H), 6)
    pos = torch.arange(T + 8)[None]
    ref = so.llama_forward(wq, ocfg, x, pos, so.KVCache(ocfg.layers), act_quant=so.fp8_rowwise_fake_quant)
    tol = 3e-2 * float(ref.abs().max())
    st = eng.new_state(1, 64, 2)
    eng.prefill(x[:, :T].to(DEV), max_new=1, state=st)
    _, al, _ = eng.append(st, x[:, T:].to(DEV), all_logits=True)
    assert st.pos.tolist() == [T + 8]
    assert_close(al, ref[:, T:], tol, 0, "appended rows' logits vs the oracle continuing with act_quant")
    assert_close(st.logits, ref[:, -1], tol, 0, "st.logits vs the oracle's last row")
    # ragged prefill goes through the same sequence: row 1 of a right-padded batch against the oracle of that row alone
    xr = _x((2, T, H), 7)
    lens = torch.tensor([T, 21])
    str_ = eng.new_state(2, 64, 2)
    eng.prefill(xr.to(DEV), max_new=1, lens=lens, state=str_)
    r1 = so.llama_forward(wq, ocfg, xr[1:, :21], torch.arange(21)[None], so.KVCache(ocfg.layers), act_quant=so.fp8_rowwise_fake_quant)
    assert_close(str_.logits[1], r1[0, -1], 3e-2 * float(r1.abs().max()), 0, "ragged prefill, the short row")


def test_routing_and_workspace():
    """fp8_act = 1, mxfp4_direct = 0; the workspace is the "mxfp4" one without the bf16 expansion scratch (the last region there,
    each region rounded up to 256 bytes) and with the activation bytes [rows, max K] and scales [rows]: nothing can expand"""
    _, _, eng, engm = _setup()
    assert eng.w.llm.fp8_act == 1 and eng.w.llm.mxfp4_direct == 0 and eng.mxfp4_prefill_direct is False
    assert engm.w.llm.fp8_act == 0

    def up(n):
        return (n + 255) // 256 * 256

    cfg = eng.cfg
    for batch, tokens in ((1, 64), (3, 40)):
        st, stm = eng.new_state(batch, tokens, 2), engm.new_state(batch, tokens, 2)
        hqd, qkvw = cfg.heads * cfg.head_dim, (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim
        scratch = 2 * max(qkvw * cfg.hidden, cfg.hidden * hqd, 2 * cfg.inter * cfg.hidden, cfg.hidden * cfg.inter)
        rows, kmax = batch * tokens, max(cfg.hidden, cfg.inter, hqd)
        assert st.ws.numel() == stm.ws.numel() - up(scratch) + up(rows * kmax) + up(rows * 4)
        assert st.ws.numel() < stm.ws.numel()


def test_packed_two_row_decode_step_is_the_mxfp4_packed_engines():
    """mxfp4_packed composes: the engine binds, and a 2-row decode step after the W4A8 prefill returns the bits of the "mxfp4" packed
    engine's step on a copy of the same cache (decode_pass_rows goes down unchanged too)"""
    from oracle import srgpt_oracle as so
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine

    w = so.synth_weights(so.SrgptConfig(**KW), seed=3, dtype=BF16)
    eng = SrgptEngine(SrgptConfig(**KW), dict(w), device=DEV, dtype=BF16, rope_positions=512, llm_weight_format="mxfp4_w4a8",
                      mxfp4_packed=True, decode_pass_rows=32)
    engm = SrgptEngine(SrgptConfig(**KW), dict(w), device=DEV, dtype=BF16, rope_positions=512, llm_weight_format="mxfp4",
                       mxfp4_packed=True, decode_pass_rows=32)
    try:
        assert eng.w.mxfp4_packed is True and engm.w.mxfp4_packed is True and eng.decode_pass_rows == 32
        assert eng.w.llm.fp8_act == 1 and eng.w.llm.decode_pass_rows == 32
        x = _x((2, T, H), 8).to(DEV)
        st, stm = eng.new_state(2, 64, 2), engm.new_state(2, 64, 2)
        eng.prefill(x, max_new=2, state=st)
        engm.prefill(x, max_new=2, state=stm)
        assert not torch.equal(_bits(st.logits), _bits(stm.logits))  # the prefills are different arithmetics
        stm.kcache.copy_(st.kcache)
        stm.vcache.copy_(st.vcache)
        tok = torch.tensor([[11], [500]], device=DEV)
        got, gotm = eng.step(st, tok), engm.step(stm, tok)
        assert bool(torch.isfinite(got).all()) and torch.equal(_bits(got), _bits(gotm))
    finally:
        eng.w.mxfp4_unbind()
        engm.w.mxfp4_unbind()
