"""llm_weight_format="mxfp4" with mxfp4_packed=True through the engine, on the geometry of tests/test_gpu_mxfp4.py and from the same
weights as its default engine: what the packed engine holds and binds; the one-row step unchanged; every decode-shaped step of 2+ rows
-- the batched step (3 rows, and 8 rows as ONE weight pass), the lookup step (T = 4) and the batched lookup step (2, 4), eager and
as replayed graphs -- bit for bit equal to its per-op composition over srgpt_gemv_w4p with the row-statistics chain; the requests on
the peaked weights of tests/test_gpu_lookup.py; the CPU oracle on the dequantised weights; unbinding; one case at the 8B layer
geometry."""
import ctypes as C
import functools

import pytest
import torch

from tests.test_gpu_mxfp4 import KW, MATS, H, _bits, _setup, _x
from tests.util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


def _lib():
    from spatialrgpt_amd import _lib as L, ops
    return L.load(), L, ops


@functools.lru_cache(maxsize=None)
def _packed_engine():
    """a second engine from the weights of test_gpu_mxfp4.py's, with the packed copies"""
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine

    _, w, _, _, _ = _setup()
    return SrgptEngine(SrgptConfig(**KW), dict(w), device=DEV, dtype=BF16, rope_positions=512, llm_weight_format="mxfp4", mxfp4_packed=True)


def _mat(w, name, i):
    """the packed copy of layer i's matrix as gemv_w4p's operands"""
    return dict(packed=w.p4[name][i][1], n_rows=w.llm_q4[name][0][i].shape[0])


def _layers_lm_head(ops, eng, h, attention):
    """the decode-layer sequence of a step on the MFMA path: attention(i, qkv) -> the attention rows; -> fp32 logits"""
    cfg, w = eng.cfg, eng.w
    ss = None
    for i in range(cfg.layers):
        qkv = ops.gemv_w4p(h, norm_w=w.llm_t["attn_norm"][i], eps=cfg.rms_eps, rowss_in=ss, **_mat(w, "wqkv", i))
        a = attention(i, qkv)
        h, ss = ops.gemv_w4p(a, residual=h, publish=True, **_mat(w, "wo", i))
        act = ops.gemv_w4p(h, norm_w=w.llm_t["mlp_norm"][i], eps=cfg.rms_eps, swiglu=True, rowss_in=ss, **_mat(w, "wgu", i))
        h, ss = ops.gemv_w4p(act, residual=h, publish=True, **_mat(w, "wdown", i))
    return ops.gemv_rowss(h, w8=w.lm_head8, wscale=w.lm_head_scale, norm_w=w.final_norm, eps=cfg.rms_eps, out_f32=True, rowss_in=ss)


def test_the_packed_engine_holds_the_same_codes_and_binds_every_matrix():
    _, _, ops = _lib()
    eng, engp = _setup()[2], _packed_engine()
    assert engp.w.mxfp4_packed is True and eng.w.mxfp4_packed is False and eng.w.mxfp4_packed_bytes() == 0
    total = 0
    for k in MATS:
        for i, (c, cp) in enumerate(zip(eng.w.llm_q4[k][0], engp.w.llm_q4[k][0])):
            assert torch.equal(c, cp) and torch.equal(eng.w.llm_q4[k][1][i], engp.w.llm_q4[k][1][i]), (k, i)
            assert ops.mxfp4_bound(cp) and not ops.mxfp4_bound(c), (k, i)
            codes, packed = engp.w.p4[k][i]
            assert codes.data_ptr() == cp.data_ptr()
            rows, K = cp.shape[0], cp.shape[1] * 2
            assert packed.numel() == ops.mxfp4_packed_bytes(rows // 2 if k == "wgu" else rows, K, k == "wgu") == rows * K * 17 // 32
            back = ops.unpack_mxfp4(packed, rows // 2 if k == "wgu" else rows, K, k == "wgu")
            assert torch.equal(back[0], cp) and torch.equal(back[1], engp.w.llm_q4[k][1][i]), (k, i)
            total += packed.numel()
    assert engp.w.mxfp4_packed_bytes() == total
    assert engp.w.llm_weight_bytes() == eng.w.llm_weight_bytes()  # the batch-1 stream is the row-major codes'


def test_a_shape_outside_the_domain_packs_nothing():
    """inter 1440 (down_proj's K % 128 != 0): the keyword is accepted, nothing is packed or bound, the engine is the default one"""
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.weights import PreparedWeights, synth_state_dict

    _, _, ops = _lib()
    cfg = SrgptConfig(**dict(KW, inter=1440, layers=1))
    w = PreparedWeights(cfg, synth_state_dict(cfg, seed=1, dtype=BF16, device=DEV), DEV, BF16, rope_positions=64, llm_weight_format="mxfp4",
                        parts=("llm",), mxfp4_packed=True)
    assert w.mxfp4_packed is False and w.mxfp4_packed_bytes() == 0 and not any(ops.mxfp4_bound(c) for k in MATS for c in w.llm_q4[k][0])


def test_one_row_step_is_the_default_engines():
    """a bound engine changes nothing below the threshold: logits and cache rows of the default engine, bit for bit"""
    eng, engp = _setup()[2], _packed_engine()
    x = _x((1, 37, H), 5).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(3)
    eng._state = engp._state = None
    st, _, _ = eng.prefill(x, max_new=6)
    stp, _, _ = engp.prefill(x, max_new=6)
    for t in range(4):
        tok = torch.randint(3, 900, (1, 1), device=DEV, generator=g)
        assert torch.equal(eng.step(st, tok), engp.step(stp, tok)), t
    assert torch.equal(_bits(st.kcache[:, :, :, :41]), _bits(stp.kcache[:, :, :, :41])) and torch.equal(_bits(st.vcache[:, :, :, :41]), _bits(stp.vcache[:, :, :, :41]))


def _decode_composition(eng, batch, T0, G):
    lib, L, ops = _lib()
    cfg, w = eng.cfg, eng.w
    Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
    assert w.mxfp4_packed and ops.gemv_rowss_supported(batch, True)
    g = torch.Generator(device=DEV).manual_seed(3)
    x = (torch.randn((batch, T0, cfg.hidden), device=DEV, generator=g) * 0.5).to(BF16)
    eng._state = None
    st, _, _ = eng.prefill(x, max_new=G + 2)
    kc, vc = st.kcache.clone(), st.vcache.clone()  # the composition keeps its own copy of the cache
    for t in range(G):
        tok = torch.randint(3, 900, (batch, 1), device=DEV, generator=g)
        got = eng.step(st, tok)
        h = ops.embed_rows(w.embed, tok.reshape(-1))
        pos = torch.full((batch,), T0 + t, device=DEV, dtype=torch.int32)
        ref = _layers_lm_head(ops, eng, h, lambda i, qkv: ops.decode_attention(qkv, kc[i], vc[i], pos, w.rope_cos, w.rope_sin, Hq, Hkv, D))
        assert torch.equal(got, ref), f"batch {batch}, step {t}: max diff {float((got - ref).abs().max())}"
    assert torch.equal(_bits(st.kcache[:, :, :, :T0 + G]), _bits(kc[:, :, :, :T0 + G]))
    assert torch.equal(_bits(st.vcache[:, :, :, :T0 + G]), _bits(vc[:, :, :, :T0 + G]))
    assert lib.srgpt_llm_decode_sync_state(C.byref(w.llm), C.byref(st.c), ops._stream()) == 0, L.last_error()


@pytest.mark.parametrize("batch", [3, 8])
def test_batched_step_equals_per_op_composition_bit_for_bit(batch):
    """3 rows, and 8 rows as ONE pass over the packed copies (two passes of the VALU kernel in a default engine)"""
    _decode_composition(_packed_engine(), batch, T0=37, G=4)


def test_step_composition_at_the_8b_layer_geometry():
    """hidden 4096, inter 14336, heads 32 / 8, 2 layers, batch 4, 2 steps: every product on the shapes of the 8B decode step"""
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine
    from spatialrgpt_amd.weights import synth_state_dict

    cfg = SrgptConfig(vit_hidden=64, vit_inter=176, vit_layers=2, vit_heads=4, image_size=42, patch_size=14, layers=2, vocab=4098,
                      mask_token_id=4096, depth_token_id=4097, hidden=4096, inter=14336, heads=32, kv_heads=8)
    eng = SrgptEngine(cfg, synth_state_dict(cfg, seed=5, dtype=BF16, device=DEV), device=DEV, dtype=BF16, rope_positions=256,
                      llm_weight_format="mxfp4", mxfp4_packed=True)
    assert eng.w.mxfp4_packed
    _decode_composition(eng, 4, T0=20, G=2)
    eng.w.mxfp4_unbind()


def test_batch_3_decode_logits_vs_oracle_on_the_dequantised_weights():
    from oracle import srgpt_oracle as so

    lib, L, ops = _lib()
    ocfg, _, _, wd, _ = _setup()
    eng = _packed_engine()
    batch, T, G = 3, 37, 4
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
    tol = 3e-2 * float(all_logits.abs().max())  # tests/test_gpu_mxfp4.py's bound
    kv = so.KVCache(ocfg.layers)
    ref = so.llama_forward(wd, ocfg, full.cpu(), torch.arange(T + G)[None].expand(batch, -1), kv)
    for s in range(G + 1):
        assert_close(dec_logits[s], ref[:, T - 1 + s], tol, 0, f"packed mxfp4 decode step {s} vs oracle")


def test_after_unbind_the_batched_step_is_the_default_engines():
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine

    _, _, ops = _lib()
    _, w, eng, _, _ = _setup()
    engu = SrgptEngine(SrgptConfig(**KW), dict(w), device=DEV, dtype=BF16, rope_positions=512, llm_weight_format="mxfp4", mxfp4_packed=True)
    codes = [c for k in MATS for c in engu.w.llm_q4[k][0]]
    assert engu.w.mxfp4_packed and all(ops.mxfp4_bound(c) for c in codes)
    x = _x((3, 37, H), 5).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(3)
    eng._state = None
    st, _, _ = eng.prefill(x, max_new=6)
    stu, _, _ = engu.prefill(x, max_new=6)
    tok = torch.randint(3, 900, (3, 1), device=DEV, generator=g)
    # which copy a step multiplies shows once the copies differ (fp32 sums in another order round to the same bf16 almost always):
    # with layer 0's packed down_proj zeroed the bound step's logits move, the row-major codes' do not
    engu.w.p4["wdown"][0][1].zero_()
    want, bound = eng.step(st, tok).clone(), engu.step(stu, tok).clone()
    assert not torch.equal(want, bound), "the bound engine's 3-row step does not read the packed copies"
    engu.w.mxfp4_unbind()
    assert engu.w.mxfp4_packed is False and not any(ops.mxfp4_bound(c) for c in codes) and engu.w.mxfp4_packed_bytes() == 0
    engu._state = None
    stu, _, _ = engu.prefill(x, max_new=6)
    assert torch.equal(engu.step(stu, tok), want)
    assert torch.equal(_bits(st.kcache[:, :, :, :38]), _bits(stu.kcache[:, :, :, :38]))


# ------------------------------------------------------------------------------------------------ lookup steps (peaked weights)
@functools.lru_cache(maxsize=None)
def _packed_model():
    from spatialrgpt_amd.model import LlavaLlamaModel
    from tests.test_gpu_lookup import _bundle

    b = _bundle()
    m = LlavaLlamaModel(b["cfg"], dict(b["sd"]), device=DEV, dtype=BF16, rope_positions=512, llm_weight_format="mxfp4", mxfp4_packed=True)
    assert m.engine.w.mxfp4_packed
    return m


def test_lookup_step_equals_per_op_composition_bit_for_bit():
    """srgpt_llm_lookup_step at T = 4, two eager steps and two replays of its graph, as tests/test_gpu_lookup.py composes it"""
    from tests.test_gpu_lookup import A0, K, V, _chain, _state_after_first_token

    lib, L, ops = _lib()
    eng = _packed_model().engine
    cfg, w = eng.cfg, eng.w
    T = K + 1
    Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
    chain = _chain(A0, 12)
    prompt = chain[:6] + [chain[6], 999, chain[7], chain[8], 998] + [A0]
    st, _ = _state_after_first_token(eng, prompt, 16)
    lk = st.ensure_lookup(K, 2, torch.tensor(prompt, dtype=torch.int64))
    graph = None
    for rnd in range(4):
        kc, vc = st.kcache.clone(), st.vcache.clone()
        tok, out_ids, pos, step = st.tok.clone(), st.out_ids.clone(), st.pos.clone(), st.step.clone()
        stats = lk["stats"].clone()
        draft, nd = ops.lookup_draft(lk["prompt"], out_ids[0], step, K, 2, V)
        rows = [int(tok)] + draft[:int(nd)].tolist()
        rows += [rows[-1]] * (T - len(rows))
        h = ops.embed_rows(w.embed, torch.tensor(rows, device=DEV))
        ref = _layers_lm_head(ops, eng, h, lambda i, qkv: ops.decode_attention_multi(qkv[None], kc[i], vc[i], pos, w.rope_cos, w.rope_sin, Hq, Hkv, D)[0])
        ops.lookup_accept(ops.argmax(ref), draft, nd, tok, out_ids[0], pos, step, st.max_pos, stats=stats)
        with torch.cuda.stream(eng.stream):
            eng.stream.wait_stream(torch.cuda.default_stream())
            if rnd < 2:
                L.check(lib.srgpt_llm_lookup_step(C.byref(w.llm), C.byref(st.c), C.byref(lk["c"]), ops._stream()))
            else:
                graph = graph or st.ensure_lookup_graph()
                L.check(lib.srgpt_graph_launch(graph, 1, ops._stream()))
        eng.stream.synchronize()
        what = f"round {rnd}"
        assert torch.equal(lk["logits"], ref), f"{what}: logits differ, max {float((lk['logits'] - ref).abs().max())}"
        assert torch.equal(st.out_ids, out_ids) and torch.equal(st.pos, pos) and torch.equal(st.step, step) and torch.equal(st.tok, tok), what
        assert torch.equal(lk["stats"], stats), what
        assert torch.equal(_bits(st.kcache), _bits(kc)) and torch.equal(_bits(st.vcache), _bits(vc)), what
    assert lib.srgpt_llm_lookup_sync_state(C.byref(w.llm), C.byref(st.c), C.byref(lk["c"]), ops._stream()) == 0, L.last_error()


def test_batched_lookup_step_equals_per_op_composition_bit_for_bit():
    """srgpt_llm_lookup_step_batch at (2, 4), two eager steps and two replays of its graph, as tests/test_gpu_lookup_batch.py composes it"""
    from tests.test_gpu_lookup import K, V
    from tests.test_gpu_lookup_batch import STEP_CASES, T, _state, _step

    lib, L, ops = _lib()
    eng = _packed_model().engine
    cfg, w = eng.cfg, eng.w
    B = 2
    R = B * T
    Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
    prompts = STEP_CASES[B]()
    st, _, ids, mask = _state(eng, prompts, 32)
    lk = st.ensure_lookup_batch(K, 2, ids, mask)
    lk["steps"].fill_(1)
    graph = None
    for rnd in range(4):
        kc, vc = st.kcache.clone(), st.vcache.clone()
        tok, out_ids, pos, step, steps = st.tok.clone(), st.out_ids.clone(), st.pos.clone(), st.step.clone(), lk["steps"].clone()
        stats = lk["stats"].clone()
        draft, nd = ops.lookup_draft_batch(lk["prompt"], lk["n_prompt"], out_ids, steps, K, 2, V)
        rows = []
        for b in range(B):
            r = [int(tok[b])] + draft[b, :int(nd[b])].tolist()
            rows += r + [r[-1]] * (T - len(r))
        h = ops.embed_rows(w.embed, torch.tensor(rows, device=DEV))
        ref = _layers_lm_head(ops, eng, h, lambda i, qkv: ops.decode_attention_multi(qkv.view(B, T, -1), kc[i], vc[i], pos, w.rope_cos, w.rope_sin,
                                                                                    Hq, Hkv, D).view(R, -1))
        ops.lookup_accept_batch(ops.argmax(ref), draft, nd, tok, out_ids, pos, steps, step, st.max_pos, stats=stats)
        if rnd >= 2 and graph is None:
            with torch.cuda.stream(eng.stream):
                eng.stream.wait_stream(torch.cuda.default_stream())
                graph = st.ensure_lookup_batch_graph()
        _step(eng, st, lk, graph if rnd >= 2 else None)
        what = f"round {rnd}"
        assert torch.equal(lk["logits"], ref), f"{what}: logits differ, max {float((lk['logits'] - ref).abs().max())}"
        assert torch.equal(st.out_ids, out_ids) and torch.equal(st.pos, pos) and torch.equal(st.tok, tok), what
        assert torch.equal(lk["steps"], steps) and torch.equal(st.step, step) and torch.equal(lk["stats"], stats), what
        assert torch.equal(_bits(st.kcache), _bits(kc)) and torch.equal(_bits(st.vcache), _bits(vc)), what
    assert lib.srgpt_llm_lookup_sync_state_batch(C.byref(w.llm), C.byref(st.c), C.byref(lk["c"]), ops._stream()) == 0, L.last_error()


def test_lookup_requests_return_the_packed_engines_own_plain_loops_ids():
    """a lookup request (T = 4 rows per step: the MFMA path) and a two-row batched one (plain loop of 2 rows and steps of 8 rows: the
    MFMA path on both sides) against the same model's plain loop"""
    from tests.test_gpu_lookup import K, _gen, _prompt_full
    from tests.test_gpu_lookup_batch import A2, _pad, _partial

    model = _packed_model()
    n = 12
    for prompt in (_prompt_full(), _partial(A2)):
        model.engine._state = None
        plain = _gen(model, prompt, max_new_tokens=n)
        assert model.last_lookup["mode"] == "plain"
        out = _gen(model, prompt, max_new_tokens=n, prompt_lookup_num_tokens=K)
        ll = dict(model.last_lookup)
        print("\nlookup under packed mxfp4:", ll)
        assert ll["mode"] == "lookup" and ll["tokens"] == n, ll
        assert torch.equal(out, plain), (out.tolist(), plain.tolist())
    model.engine._state = None
    ids, mask = _pad([_prompt_full(), _partial(A2)], "right")
    plain = model.generate(ids, attention_mask=mask, do_sample=False, eos_token_id=None, max_new_tokens=n)
    model.lookup_batch = True
    model.engine._state = None
    try:
        out = model.generate(ids, attention_mask=mask, do_sample=False, eos_token_id=None, max_new_tokens=n, prompt_lookup_num_tokens=K)
        ll = dict(model.last_lookup)
    finally:
        model.lookup_batch = False
    print("\nbatched lookup under packed mxfp4:", ll)
    assert ll["mode"] == "lookup" and ll["batch"] == 2 and ll["tokens"] == 2 * n, ll
    assert torch.equal(out, plain), (out.tolist(), plain.tolist())
