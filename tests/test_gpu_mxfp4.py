"""llm_weight_format="mxfp4" through the engine, on the geometry of
tests/test_gpu_pipeline.py::test_fp8_weight_decode_vs_oracle_on_dequantised_weights (hidden 512, inter 1408, 3 layers, heads 8 / 2),
batch 1 and 3: the prefill against a native bf16 engine on the dequantised weights (bit for bit), the decode step against its per-op
composition (bit for bit), both against the CPU oracle on the dequantised weights (that test's 3e-2 * max |logits|), the append
prefill, the lookup steps, what the engine holds, and the workspace of the other formats.  One composition case runs at the 8B
layer geometry (hidden 4096, inter 14336, heads 32 / 8): the shapes the decode step exists for, where the attention launch carries
the L2 prefetch of o_proj's code bytes.  The lookup requests run on the peaked weights of tests/test_gpu_lookup.py, whose greedy
continuation has a margin that survives the arithmetic."""
import ctypes as C
import functools

import pytest
import torch

from tests.util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
KW = dict(vit_hidden=64, vit_inter=128, vit_layers=2, vit_heads=4, image_size=56, patch_size=14, hidden=512, inter=1408,
          layers=3, heads=8, kv_heads=2, vocab=1000, mask_token_id=998, depth_token_id=999, rope_theta=10000.0)
H = KW["hidden"]
MATS = ("wqkv", "wo", "wgu", "wdown")


def _lib():
    from spatialrgpt_amd import _lib as L, ops
    return L.load(), L, ops


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def _x(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 0.5).to(BF16)


def dequantised_state_dict(eng, w):
    """the state dict whose LLM matrices are what an mxfp4 engine multiplies: code * scale of its own codes, split back into the
    checkpoint's q / k / v and gate / up rows; lm_head: the fp8 values; everything else as given"""
    cfg = eng.cfg
    out = dict(w)
    nq, nkv, I = cfg.heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim, cfg.inter
    for i in range(cfg.layers):
        p = f"llm.model.layers.{i}."
        qkv, gu = eng.w.dequantised("wqkv", i).cpu(), eng.w.dequantised("wgu", i).cpu()
        out[p + "self_attn.q_proj.weight"], out[p + "self_attn.k_proj.weight"], out[p + "self_attn.v_proj.weight"] = \
            qkv[:nq], qkv[nq:nq + nkv], qkv[nq + nkv:]
        out[p + "self_attn.o_proj.weight"] = eng.w.dequantised("wo", i).cpu()
        out[p + "mlp.gate_proj.weight"], out[p + "mlp.up_proj.weight"] = gu[:I], gu[I:]
        out[p + "mlp.down_proj.weight"] = eng.w.dequantised("wdown", i).cpu()
    out["llm.lm_head.weight"] = eng.w.dequantised("lm_head").cpu()
    return out


@functools.lru_cache(maxsize=None)
def _setup():
    """(oracle config, the synthetic weights, the mxfp4 engine, its dequantised state dict, a native bf16 engine built from that)"""
    from oracle import srgpt_oracle as so
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine

    ocfg = so.SrgptConfig(**KW)
    w = so.synth_weights(ocfg, seed=3, dtype=BF16)
    eng = SrgptEngine(SrgptConfig(**KW), dict(w), device=DEV, dtype=BF16, rope_positions=512, llm_weight_format="mxfp4")
    wd = dequantised_state_dict(eng, w)
    engd = SrgptEngine(SrgptConfig(**KW), dict(wd), device=DEV, dtype=BF16, rope_positions=512)
    return ocfg, w, eng, wd, engd


def test_the_engine_holds_codes_and_scales_only():
    from spatialrgpt_amd import ops

    _, w, eng, wd, _ = _setup()
    ew = eng.w
    assert ew.llm_weight_format == "mxfp4" and ew.lm_head is None and ew.lm_head8 is not None
    for k in MATS:
        assert all(t is None for t in ew.llm_t[k]), k  # no bf16 copy
        assert not ew.llm_q.get(k), k                   # no fp8 copy
        for codes, scales in zip(*ew.llm_q4[k]):
            assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8 and codes.shape[1] == 16 * scales.shape[1]
            assert int(scales.min()) >= 1 and int(scales.max()) <= 254
    # the loader's codes are the quantiser's, and dequantised() is code * scale of the same rule
    wdown1 = w["llm.model.layers.1.mlp.down_proj.weight"]
    codes, scales, deq = ops.quantize_mxfp4_rows(wdown1.to(DEV))
    assert torch.equal(codes, ew.llm_q4["wdown"][0][1]) and torch.equal(scales, ew.llm_q4["wdown"][1][1])
    assert torch.equal(ew.dequantised("wdown", 1), deq) and torch.equal(deq.cpu(), wd["llm.model.layers.1.mlp.down_proj.weight"])
    # 4.25 bits per weight for the four matrices, 8 bits + a row scale for lm_head
    mat_bf16 = sum(t.numel() * 2 for k, t in w.items() if k.startswith("llm.model.layers.") and "proj" in k)
    bound = 0.32 * (mat_bf16 + ew.lm_head8.numel() + 4 * ew.lm_head_scale.numel())
    print("\nllm_weight_bytes %d, bound %.0f, bf16 bytes of the four matrices %d" % (ew.llm_weight_bytes(), bound, mat_bf16))
    assert ew.llm_weight_bytes() < bound


def test_resize_vocab_keeps_working():
    """lm_head is fp8 under the format: new rows are quantised with the loader's rule and appended, the codes are untouched"""
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine

    _, w, eng, _, _ = _setup()
    ew = SrgptEngine(SrgptConfig(**KW), dict(w), device=DEV, dtype=BF16, rope_positions=512, llm_weight_format="mxfp4").w
    before, codes = ew.lm_head8.clone(), ew.llm_q4["wqkv"][0][0].clone()
    ew.resize_vocab(1008)
    assert ew.lm_head8.shape[0] == 1008 and ew.embed.shape[0] == 1008 and torch.equal(ew.lm_head8[:1000], before) and ew.llm.vocab == 1008
    assert torch.equal(ew.llm_q4["wqkv"][0][0], codes) and torch.equal(codes, eng.w.llm_q4["wqkv"][0][0])
    ew.resize_vocab(1000)
    assert torch.equal(ew.lm_head8, before) and ew.llm.vocab == 1000


@pytest.mark.parametrize("batch", [1, 3])
def test_prefill_is_a_bf16_engines_on_the_dequantised_weights_bit_for_bit(batch):
    _, _, eng, _, engd = _setup()
    x = _x((batch, 37, H), 5).to(DEV)
    eng._state = engd._state = None
    st, al, hs = eng.prefill(x, max_new=2, all_logits=True, hidden_states=True)
    std, ald, hsd = engd.prefill(x, max_new=2, all_logits=True, hidden_states=True)
    assert torch.equal(_bits(hs), _bits(hsd)), "hidden_out"
    assert torch.equal(_bits(st.kcache[:, :, :, :37]), _bits(std.kcache[:, :, :, :37])) and torch.equal(_bits(st.vcache[:, :, :, :37]), _bits(std.vcache[:, :, :, :37]))
    # (lm_head runs on the fp8 kernels there and on the bf16 ones here: the same values, another summation order)
    assert_close(al, ald.float().cpu(), 3e-2 * float(ald.abs().max()), 0, "all-position logits")


@pytest.mark.parametrize("batch", [1, 3])
def test_decode_step_equals_per_op_composition_bit_for_bit(batch):
    _decode_composition(_setup()[2], batch, T0=37, G=6)


def test_decode_step_composition_at_the_8b_layer_geometry():
    """hidden 4096, inter 14336, heads 32 / 8, 2 layers: every product on the shapes of the 8B decode step (two 1-KiB wave loads per
    row of q/k/v, o_proj and gate/up, seven for down_proj), and the attention launch with the L2 prefetch of o_proj's codes"""
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine
    from spatialrgpt_amd.weights import synth_state_dict

    cfg = SrgptConfig(vit_hidden=64, vit_inter=176, vit_layers=2, vit_heads=4, image_size=42, patch_size=14, layers=2, vocab=4098,
                      mask_token_id=4096, depth_token_id=4097, hidden=4096, inter=14336, heads=32, kv_heads=8)
    eng = SrgptEngine(cfg, synth_state_dict(cfg, seed=5, dtype=BF16, device=DEV), device=DEV, dtype=BF16, rope_positions=256,
                      llm_weight_format="mxfp4")
    _decode_composition(eng, 1, T0=20, G=3)


def _decode_composition(eng, batch, T0, G):
    lib, L, ops = _lib()
    cfg, w = eng.cfg, eng.w
    Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
    g = torch.Generator(device=DEV).manual_seed(3)
    x = (torch.randn((batch, T0, cfg.hidden), device=DEV, generator=g) * 0.5).to(BF16)
    eng._state = None
    st, _, _ = eng.prefill(x, max_new=G + 2)
    kc, vc = st.kcache.clone(), st.vcache.clone()  # the composition keeps its own copy of the cache
    q4 = w.llm_q4
    for t in range(G):
        tok = torch.randint(3, 900, (batch, 1), device=DEV, generator=g)
        got = eng.step(st, tok)
        h = ops.embed_rows(w.embed, tok.reshape(-1))
        pos = torch.full((batch,), T0 + t, device=DEV, dtype=torch.int32)
        for i in range(cfg.layers):
            qkv = ops.gemv_w4(h, q4["wqkv"][0][i], q4["wqkv"][1][i], norm_w=w.llm_t["attn_norm"][i], eps=cfg.rms_eps)
            a = ops.decode_attention(qkv, kc[i], vc[i], pos, w.rope_cos, w.rope_sin, Hq, Hkv, D)
            h = ops.gemv_w4(a, q4["wo"][0][i], q4["wo"][1][i], residual=h)
            act = ops.gemv_w4(h, q4["wgu"][0][i], q4["wgu"][1][i], norm_w=w.llm_t["mlp_norm"][i], eps=cfg.rms_eps, swiglu=True)
            h = ops.gemv_w4(act, q4["wdown"][0][i], q4["wdown"][1][i], residual=h)
        ref = ops.gemv_w8(h, w.lm_head8, w.lm_head_scale, norm_w=w.final_norm, eps=cfg.rms_eps, out_f32=True)
        assert torch.equal(got, ref), f"batch {batch}, step {t}: max diff {float((got - ref).abs().max())}"
    assert torch.equal(_bits(st.kcache[:, :, :, :T0 + G]), _bits(kc[:, :, :, :T0 + G]))
    assert lib.srgpt_llm_decode_sync_state(C.byref(w.llm), C.byref(st.c), ops._stream()) == 0, L.last_error()


@pytest.mark.parametrize("batch", [1, 3])
def test_decode_and_prefill_logits_vs_oracle_on_the_dequantised_weights(batch):
    from oracle import srgpt_oracle as so

    lib, L, ops = _lib()
    ocfg, _, eng, wd, _ = _setup()
    T, G = 37, 5
    x = _x((batch, T, H), 5)
    eng._state = None
    st, _, _ = eng.prefill(x.to(DEV), max_new=G + 1)
    L.check(lib.srgpt_llm_sample_first(C.byref(eng.w.llm), C.byref(st.c), ops._stream()))
    dec_logits = [st.logits.clone()]
    for _ in range(G):
        L.check(lib.srgpt_llm_decode_step(C.byref(eng.w.llm), C.byref(st.c), ops._stream()))
        dec_logits.append(st.logits.clone())
    ids = st.out_ids[:, :G + 1].clone()
    full = torch.cat([x.to(DEV), eng.embed_tokens(ids[:, :G])], dim=1)
    eng._state = None
    _, all_logits, _ = eng.prefill(full, max_new=1, all_logits=True)
    tol = 3e-2 * float(all_logits.abs().max())
    for s in range(G + 1):
        assert_close(dec_logits[s], all_logits[:, T - 1 + s], tol, 0, f"mxfp4 decode step {s} vs prefill on the dequantised weights")
    kv = so.KVCache(ocfg.layers)
    ref = so.llama_forward(wd, ocfg, full.cpu(), torch.arange(T + G)[None].expand(batch, -1), kv)
    assert_close(all_logits, ref, tol, 0, "prefill logits vs oracle (dequantised weights)")
    for s in range(G + 1):
        assert_close(dec_logits[s], ref[:, T - 1 + s], tol, 0, f"mxfp4 decode step {s} vs oracle")


def _append_case(eng, batch, P=32, T=5):
    """-> (k, v bits of cache rows P .. P + T - 1 after prefill(P) + append(T), the same rows after one prefill of P + T rows)"""
    x = _x((batch, P + T, H), 9).to(DEV)
    whole = eng.new_state(batch, 128, 2)
    eng.prefill(x, max_new=2, state=whole)
    st = eng.new_state(batch, 128, 2)
    eng.prefill(x[:, :P].contiguous(), max_new=2, state=st)
    eng.append(st, x[:, P:].contiguous())
    assert st.pos.tolist() == [P + T] * batch
    rows = slice(P, P + T)
    return (_bits(st.kcache[:, :, :, rows]), _bits(st.vcache[:, :, :, rows])), (_bits(whole.kcache[:, :, :, rows]), _bits(whole.vcache[:, :, :, rows]))


@pytest.mark.parametrize("batch", [1, 3])
def test_append_of_a_five_row_segment_writes_the_whole_prefills_cache_rows(batch):
    _, _, eng, _, engd = _setup()
    (k, v), (kw_, vw) = _append_case(eng, batch)
    (kd, vd), _ = _append_case(engd, batch)
    print("\nbatch %d: cache elements of the 5 appended rows that differ from the whole prefill's: k %d, v %d of %d"
          % (batch, int((k != kw_).sum()), int((v != vw).sum()), k.numel()))
    # the format's own share: the append's launches are a bf16 engine's on the dequantised weights
    assert torch.equal(k, kd) and torch.equal(v, vd), "append under mxfp4 differs from the bf16 engine on the dequantised weights"
    assert torch.equal(k, kw_) and torch.equal(v, vw), "appended cache rows differ from the whole prefill's"


def test_other_formats_report_the_workspace_they_did():
    """srgpt_llm_ws_bytes of a native and an fp8 engine: what the layout sums to without the MXFP4 scratch, computed here from the
    struct alone by asking for the bytes with the MXFP4 pointers set and cleared"""
    lib, L, ops = _lib()
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine

    _, w, eng4, _, engd = _setup()
    eng8 = SrgptEngine(SrgptConfig(**KW), dict(w), device=DEV, dtype=BF16, rope_positions=512, llm_weight_format="fp8")
    scratch = (2 * KW["inter"] * H * 2 + 255) // 256 * 256
    for batch, tokens in ((1, 37), (3, 64)):
        n4 = lib.srgpt_llm_ws_bytes(C.byref(eng4.w.llm), batch, tokens)
        for e in (engd, eng8):
            n = lib.srgpt_llm_ws_bytes(C.byref(e.w.llm), batch, tokens)
            assert n == n4 - scratch, (batch, tokens, n, n4)
            assert not e.w.llm.wqkv4
            e.w.llm.wqkv4 = eng4.w.llm.wqkv4  # the same struct with the MXFP4 pointer set asks for the scratch on top, nothing else
            try:
                assert lib.srgpt_llm_ws_bytes(C.byref(e.w.llm), batch, tokens) == n + scratch
            finally:
                e.w.llm.wqkv4 = None
            assert lib.srgpt_llm_ws_bytes(C.byref(e.w.llm), batch, tokens) == n


# ------------------------------------------------------------------------------------------------ lookup requests (peaked weights)
def test_lookup_request_returns_the_plain_loops_ids():
    from tests.test_gpu_lookup import K, _gen, _model, _prompt_full
    from tests.test_gpu_lookup_batch import _partial, A2

    model = _model("mxfp4")
    assert model.engine.w.llm_weight_format == "mxfp4" and K == 3
    for prompt, n in ((_prompt_full(), 12), (_partial(A2), 12)):
        plain = _gen(model, prompt, max_new_tokens=n)
        assert model.last_lookup["mode"] == "plain"
        out = _gen(model, prompt, max_new_tokens=n, prompt_lookup_num_tokens=K)
        ll = dict(model.last_lookup)
        print("\nlookup under mxfp4:", ll)
        assert ll["mode"] == "lookup" and ll["tokens"] == n, ll
        assert ll["accepted"] > 0 or prompt != _prompt_full(), ll  # the walk repeats the prompt: its drafts are kept
        assert torch.equal(out, plain), (out.tolist(), plain.tolist())


def test_batched_lookup_request_of_two_rows_returns_the_plain_loops_ids():
    from tests.test_gpu_lookup import K, _model, _prompt_full
    from tests.test_gpu_lookup_batch import _pad, _partial, A2

    model = _model("mxfp4")
    model.engine._state = None
    ids, mask = _pad([_prompt_full(), _partial(A2)], "right")
    n = 12
    plain = model.generate(ids, attention_mask=mask, do_sample=False, eos_token_id=None, max_new_tokens=n)
    model.lookup_batch = True
    model.engine._state = None
    try:
        out = model.generate(ids, attention_mask=mask, do_sample=False, eos_token_id=None, max_new_tokens=n, prompt_lookup_num_tokens=K)
        ll = dict(model.last_lookup)
    finally:
        model.lookup_batch = False
    print("\nbatched lookup under mxfp4:", ll)
    assert ll["mode"] == "lookup" and ll["batch"] == 2 and ll["tokens"] == 2 * n and ll["accepted"] > 0, ll
    assert torch.equal(out, plain), (out.tolist(), plain.tolist())
