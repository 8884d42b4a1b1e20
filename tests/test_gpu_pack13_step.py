"""GPU: the batch-1 bf16 decode step with 13-bit packed copies bound (PreparedWeights pack13="all") against the same engine with the
switch off -- logits, ids and cache bit for bit, eagerly and from the captured graph, and the bindings' life cycle."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _engines():
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine
    from spatialrgpt_amd.weights import synth_state_dict

    cfg = SrgptConfig(vit_hidden=64, vit_inter=176, vit_layers=2, vit_heads=4, image_size=42, patch_size=14, layers=2, vocab=1002,
                      mask_token_id=1000, depth_token_id=1001, hidden=512, inter=1024, heads=8, kv_heads=4)
    dt = torch.bfloat16
    mk = lambda p13: SrgptEngine(cfg, synth_state_dict(cfg, seed=7, dtype=dt, device=DEV), device=DEV, dtype=dt, rope_positions=512,
                                 pack13=p13)
    return cfg, mk("all"), mk(False)


def test_decode_step_bound_equals_unbound_bit_for_bit():
    from spatialrgpt_amd import _lib as L
    from spatialrgpt_amd import ops

    cfg, on, off = _engines()
    # every product of the step but o_proj is bound, with no exception row (nothing runs on the raw fallback), and nothing of `off` is
    assert sorted(on.w.p13) == ["lm_head", "wdown", "wgu", "wqkv"] and all(e is not None for v in on.w.p13.values() for e in v)
    assert on.w.pack13_exception_rows() == 0 and off.w.p13 == {}
    assert all(ops.pack13_bound(t) for k in ("wqkv", "wgu", "wdown") for t in on.w.llm_t[k]) and ops.pack13_bound(on.w.lm_head)
    assert not any(ops.pack13_bound(t) for t in on.w.llm_t["wo"])
    assert not any(ops.pack13_bound(t) for k in ("wqkv", "wgu", "wdown") for t in off.w.llm_t[k]) and not ops.pack13_bound(off.w.lm_head)
    assert on.w.llm_weight_bytes() != off.w.llm_weight_bytes()
    T0, G = 122, 12  # contexts 122 .. 133: across the 128-row cache granule
    g = torch.Generator(device=DEV).manual_seed(3)
    x = (torch.randn((1, T0, cfg.hidden), device=DEV, generator=g) * 0.5).to(torch.bfloat16)
    toks = torch.randint(3, 1000, (G,), device=DEV, generator=g)
    st_on, _, _ = on.prefill(x, max_new=G + 2)
    st_off, _, _ = off.prefill(x, max_new=G + 2)
    for t in range(G):
        tok = toks[t:t + 1].reshape(1, 1)
        a, b = on.step(st_on, tok), off.step(st_off, tok)
        assert torch.equal(a, b), f"step {t}: {int((a != b).sum())} logits differ"
    for a, b in ((st_on.kcache, st_off.kcache), (st_on.vcache, st_off.vcache)):  # the written positions (the rest is uninitialised)
        assert torch.equal(a[:, :, :, :T0 + G], b[:, :, :, :T0 + G])
    for eng, st in ((on, st_on), (off, st_off)):  # the arrival tickets of the decode attention are re-armed
        assert L.load().srgpt_llm_decode_sync_state(C.byref(eng.w.llm), C.byref(st.c), ops._stream()) == 0, L.last_error()
    # the captured graph (greedy loop) replays the same ids
    ids = []
    for eng in (on, off):
        st, _, _ = eng.prefill(x, max_new=G + 2)
        ids.append(eng.greedy_decode(st, G).clone())
        assert L.load().srgpt_llm_decode_sync_state(C.byref(eng.w.llm), C.byref(st.c), ops._stream()) == 0, L.last_error()
    assert ids[0].shape[-1] == G and torch.equal(ids[0], ids[1])


def test_bindings_follow_the_raw_matrices():
    """resize_vocab re-packs lm_head (the old binding goes before the old matrix does); teardown unbinds everything"""
    from spatialrgpt_amd import ops

    cfg, on, off = _engines()
    del off
    old = on.w.lm_head
    on.w.resize_vocab(1030)
    assert not ops.pack13_bound(old) and ops.pack13_bound(on.w.lm_head) and on.w.p13["lm_head"][0][0] is on.w.lm_head
    assert torch.equal(ops.unpack13(on.w.p13["lm_head"][0][1], on.w.p13["lm_head"][0][2], on.w.lm_head).view(torch.int16),
                       on.w.lm_head.view(torch.int16))
    x = (torch.randn((1, 5, cfg.hidden), device=DEV) * 0.5).to(torch.bfloat16)
    st, _, _ = on.prefill(x, max_new=4)
    logits = on.step(st, torch.tensor([[7]], device=DEV))
    assert logits.shape == (1, 1030)
    raws = [t for k in ("wqkv", "wgu", "wdown") for t in on.w.llm_t[k]] + [on.w.lm_head]
    on.w.pack13_unbind()
    assert on.w.p13 == {} and not any(ops.pack13_bound(t) for t in raws)


def test_engines_built_from_the_same_device_tensors_do_not_share_bindings():
    """a state dict already on the device in the engine dtype is used without a copy (lm_head, down_proj), and the binding table is
    keyed by address: a matrix that gets bound is cloned first, so a second engine over the same tensors neither streams, replaces
    nor tears down the first one's copies"""
    import gc

    from spatialrgpt_amd import ops
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine
    from spatialrgpt_amd.weights import synth_state_dict

    cfg = SrgptConfig(vit_hidden=64, vit_inter=176, vit_layers=2, vit_heads=4, image_size=42, patch_size=14, layers=2, vocab=1002,
                      mask_token_id=1000, depth_token_id=1001, hidden=512, inter=1024, heads=8, kv_heads=4)
    dt = torch.bfloat16
    sd = synth_state_dict(cfg, seed=7, dtype=dt, device=DEV)
    head, down0 = sd["llm.lm_head.weight"], sd["llm.model.layers.0.mlp.down_proj.weight"]
    mk = lambda p13: SrgptEngine(cfg, sd, device=DEV, dtype=dt, rope_positions=512, pack13=p13)
    a, off, b = mk("all"), mk(False), mk("all")
    # the unpacked engine uses the caller's tensors as they are, and nobody bound those
    assert off.w.lm_head.data_ptr() == head.data_ptr() and off.w.llm_t["wdown"][0].data_ptr() == down0.data_ptr()
    assert not ops.pack13_bound(head) and not ops.pack13_bound(down0)
    for e in (a, b):  # every packing engine bound matrices of its own, and its C struct points at them
        assert e.w.lm_head.data_ptr() != head.data_ptr() and e.w.llm_t["wdown"][0].data_ptr() != down0.data_ptr()
        assert e.w.llm.lm_head == e.w.lm_head.data_ptr() and e.w.llm.wdown[0] == e.w.llm_t["wdown"][0].data_ptr()
        assert ops.pack13_bound(e.w.lm_head) and all(ent is not None for v in e.w.p13.values() for ent in v)
    assert a.w.lm_head.data_ptr() != b.w.lm_head.data_ptr()
    x = (torch.randn((1, 9, cfg.hidden), device=DEV) * 0.5).to(dt)
    tok = torch.tensor([[11]], device=DEV)
    ref = off.step(off.prefill(x, max_new=4)[0], tok).clone()
    b_head = b.w.lm_head
    del a
    gc.collect()
    # tearing down one engine left the other's bindings alone, and it still computes the raw engine's bits
    assert ops.pack13_bound(b_head) and all(ops.pack13_bound(t) for t in b.w.llm_t["wdown"])
    assert torch.equal(b.step(b.prefill(x, max_new=4)[0], tok), ref)
    # an address somebody else has bound is left alone: that matrix runs raw here, and the foreign binding survives our teardown
    wgu = b.w.llm_t["wgu"][0]
    assert b.w._pack13_bind(wgu) is None and ops.pack13_bound(wgu)
