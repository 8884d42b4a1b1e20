"""decode_pass_rows = 32 through the engine, on the 3-layer, 8B-width geometry of
tests/test_gpu_kernels.py::test_batched_decode_step_equals_rowss_composition_bit_for_bit (hidden 4096, inter 14336, 32 / 8 heads, vocab
4098, a prefill of 60 positions, 3 steps): the step's logits and caches equal, bit for bit, the composition of the `wide=True` per-op
entries and ops.decode_attention, step after step; the captured loop equals the eager one; an engine left at 16 returns the bits of
the existing composition at 20 rows (the option off is today's step), and at 8 rows the two engines return the same logits.  Then the
surface: LlavaLlamaModel(decode_pass_rows=32).generate of 20 tiny-bf16 rows, every id the argmax of the step's logits."""
import ctypes as C
import functools

import pytest
import torch

from tests.util import load_tiny

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
T0, G = 60, 3
FORMATS = {"bf16": {}, "fp8": dict(llm_weight_format="fp8"), "mxfp4": dict(llm_weight_format="mxfp4", mxfp4_packed=True)}


def _mods():
    from spatialrgpt_amd import _lib as L
    from spatialrgpt_amd import ops
    return L, ops


@functools.lru_cache(maxsize=None)
def _config_and_weights():
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.weights import synth_state_dict

    cfg = SrgptConfig(vit_hidden=64, vit_inter=176, vit_layers=2, vit_heads=4, image_size=42, patch_size=14, layers=3, vocab=4098,
                      mask_token_id=4096, depth_token_id=4097, hidden=4096, inter=14336, heads=32, kv_heads=8)
    return cfg, synth_state_dict(cfg, seed=5, dtype=BF16, device=DEV)


@functools.lru_cache(maxsize=None)
def engine(fmt, pass_rows):
    """one engine per (format, option), shared by the tests below; the state dict is shared and left unchanged"""
    from spatialrgpt_amd.engine import SrgptEngine

    cfg, sd = _config_and_weights()
    eng = SrgptEngine(cfg, dict(sd), device=DEV, dtype=BF16, rope_positions=512, decode_pass_rows=pass_rows, **FORMATS[fmt])
    assert eng.decode_pass_rows == pass_rows == eng.w.llm.decode_pass_rows  # the option reached srgpt_llm_weights
    assert fmt != "mxfp4" or eng.w.mxfp4_packed
    return eng


def inputs(B):
    g = torch.Generator(device=DEV).manual_seed(3)
    x = (torch.randn((B, T0, 4096), device=DEV, generator=g) * 0.5).to(BF16)
    toks = torch.randint(3, 4096, (G, B), device=DEV, generator=g)
    return x, toks


def composition_step(eng, fmt, wide, tok, kc, vc, t):
    """one step as the per-op entries compute it (wide: the `_wide` entries) -> fp32 logits; appends to kc / vc"""
    L, ops = _mods()
    cfg, w = eng.cfg, eng.w
    B = tok.shape[0]

    def prod(name, i, x, **kw):
        if fmt == "mxfp4":
            return ops.gemv_w4p(x, w.p4[name][i][1], w.llm_q4[name][0][i].shape[0], wide=wide, **kw)
        if fmt == "fp8":  # the packed copy the step streams
            return ops.gemv_rowss(x, w8=w.llm_pk[name][i], wscale=w.llm_q[name][1][i], packed_rows=w.pk_rows[name],
                                  n_rows=w.llm_q[name][0][i].shape[0], wide=wide, **kw)
        return ops.gemv_rowss(x, w=w.llm_t[name][i], wide=wide, **kw)

    h = ops.embed_rows(w.embed, tok.reshape(-1))
    pos = torch.full((B,), T0 + t, device=DEV, dtype=torch.int32)
    ss = None
    for i in range(cfg.layers):
        qkv = prod("wqkv", i, h, norm_w=w.llm_t["attn_norm"][i], eps=cfg.rms_eps, rowss_in=ss)
        a = ops.decode_attention(qkv, kc[i], vc[i], pos, w.rope_cos, w.rope_sin, cfg.heads, cfg.kv_heads, cfg.head_dim)
        h, ss = prod("wo", i, a, residual=h, publish=True)
        act = prod("wgu", i, h, norm_w=w.llm_t["mlp_norm"][i], eps=cfg.rms_eps, swiglu=True, rowss_in=ss)
        h, ss = prod("wdown", i, act, residual=h, publish=True)
    head = dict(w=w.lm_head) if fmt == "bf16" else dict(w8=w.lm_head8, wscale=w.lm_head_scale)
    return ops.gemv_rowss(h, norm_w=w.final_norm, eps=cfg.rms_eps, out_f32=True, rowss_in=ss, wide=wide, **head)


def step_equals_composition(fmt, pass_rows, B):
    L, ops = _mods()
    eng = engine(fmt, pass_rows)
    if fmt == "fp8":
        assert set(eng.w.llm_pk) == {"wqkv", "wo", "wgu", "wdown"}
    x, toks = inputs(B)
    eng._state = None
    st, _, _ = eng.prefill(x, max_new=G + 2)
    kc, vc = st.kcache.clone(), st.vcache.clone()
    for t in range(G):
        tok = toks[t].reshape(B, 1)
        got = eng.step(st, tok)
        ref = composition_step(eng, fmt, pass_rows == 32, tok, kc, vc, t)
        assert torch.equal(got, ref), "%s pass_rows=%d B=%d step %d: %d of %d logits differ, max %g" % (
            fmt, pass_rows, B, t, int((got != ref).sum()), got.numel(), float((got - ref).abs().max()))
    assert torch.equal(st.kcache[:, :, :, :T0 + G].view(torch.int16), kc[:, :, :, :T0 + G].view(torch.int16))
    assert torch.equal(st.vcache[:, :, :, :T0 + G].view(torch.int16), vc[:, :, :, :T0 + G].view(torch.int16))
    assert L.load().srgpt_llm_decode_sync_state(C.byref(eng.w.llm), C.byref(st.c), ops._stream()) == 0, L.last_error()


@pytest.mark.parametrize("fmt,B", [("bf16", 20), ("bf16", 32), ("fp8", 20), ("fp8", 32), ("mxfp4", 20)])
def test_wide_step_equals_the_composition_of_the_wide_entries(fmt, B):
    step_equals_composition(fmt, 32, B)


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_option_off_is_todays_step_at_20_rows(fmt):
    step_equals_composition(fmt, 16, 20)


@pytest.mark.parametrize("fmt,B", [("bf16", 20), ("bf16", 32), ("fp8", 20), ("fp8", 32), ("mxfp4", 20)])
def test_captured_wide_loop_equals_the_eager_one(fmt, B):
    eng = engine(fmt, 32)
    x, _ = inputs(B)
    runs = []
    try:
        for use_graph in (True, False):
            eng.use_graph = use_graph
            eng._state = None
            st, _, _ = eng.prefill(x, max_new=G + 2)
            ids = eng.greedy_decode(st, G + 1)
            runs.append((ids.clone(), st.logits.clone(), st.kcache[:, :, :, :T0 + G].clone()))
    finally:
        eng.use_graph = True
    assert runs[0][0].shape == (B, G + 1) and torch.equal(runs[0][0], runs[1][0]), "ids"
    assert torch.equal(runs[0][1], runs[1][1]), "the last step's logits"
    assert torch.equal(runs[0][2].view(torch.int16), runs[1][2].view(torch.int16)), "the cache"


@pytest.mark.parametrize("fmt", ["bf16", "fp8", "mxfp4"])
def test_at_8_rows_both_engines_return_the_same_logits(fmt):
    x, toks = inputs(8)
    outs = []
    for pass_rows in (16, 32):
        eng = engine(fmt, pass_rows)
        eng._state = None
        st, _, _ = eng.prefill(x, max_new=G + 2)
        outs.append([eng.step(st, toks[t, :8].reshape(8, 1)) for t in range(G)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_generate_of_20_rows_with_the_option_on():
    """the surface: 20 tiny-bf16 rows through model.generate; every generated id is the argmax of the step logits the engine records"""
    from spatialrgpt_amd.model import LlavaLlamaModel

    from spatialrgpt_amd.config import SrgptConfig

    cfgd, dtype, sd, _, _ = load_tiny("tiny_bf16.npz")
    cfg = SrgptConfig.from_dict(cfgd)
    assert dtype == BF16
    with pytest.raises(ValueError, match="decode_pass_rows"):
        LlavaLlamaModel(cfg, dict(sd), device=DEV, dtype=BF16, rope_positions=512, decode_pass_rows=24)
    model = LlavaLlamaModel(cfg, dict(sd), device=DEV, dtype=BF16, rope_positions=512, decode_pass_rows=32)
    assert model.decode_pass_rows == 32 and model.engine.w.llm.decode_pass_rows == 32
    with pytest.raises(AttributeError):
        model.decode_pass_rows = 16  # read-only: captured graphs hold launches
    B, P, n = 20, 12, 6
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(3, min(cfg.vocab, cfg.mask_token_id, cfg.depth_token_id) - 1, (B, P), generator=g).to(DEV)
    out = model.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=None)
    assert out.shape == (B, n) and out.dtype == torch.int64
    # the same request step by step through the engine: every id is the argmax of the logits of the step before it
    eng = model.engine
    st, _, _ = eng.prefill(eng.embed_tokens(ids).to(BF16), max_new=n + 2)
    logits = st.logits.clone()
    for t in range(n):
        pick = logits.argmax(-1)
        assert torch.equal(pick, out[:, t]), "step %d" % t
        if t + 1 < n:
            logits = eng.step(st, out[:, t].reshape(B, 1))

