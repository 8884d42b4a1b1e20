"""The MXFP4 engine's prefill and append prefill through the W4 entry points (Prefill::layer_w4a16, model.hip) at the 8B layer
geometry: hidden 4096, inter 14336, heads 32 / 8, one layer, a small vocabulary.  Every hidden state and both caches must equal,
bit for bit, those of a bf16 engine built on the dequantised state dict."""
import functools

import pytest
import torch

from tests.test_gpu_mxfp4 import dequantised_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
HID, INTER, HQ, HKV, D = 4096, 14336, 32, 8, 128
QW = (HQ + 2 * HKV) * D
T0, TA = 259, 32


def _bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _engines():
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine
    from spatialrgpt_amd.weights import synth_state_dict

    kw = dict(vit_hidden=64, vit_inter=176, vit_layers=2, vit_heads=4, image_size=42, patch_size=14, layers=1, vocab=4098,
              mask_token_id=4096, depth_token_id=4097, hidden=HID, inter=INTER, heads=HQ, kv_heads=HKV)
    sd = synth_state_dict(SrgptConfig(**kw), seed=5, dtype=BF16, device=DEV)
    eng = SrgptEngine(SrgptConfig(**kw), dict(sd), device=DEV, dtype=BF16, rope_positions=512, llm_weight_format="mxfp4")
    sdd = dequantised_state_dict(eng, {k: v.cpu() for k, v in sd.items()})
    engd = SrgptEngine(SrgptConfig(**kw), sdd, device=DEV, dtype=BF16, rope_positions=512)
    return eng, engd


def _x(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, device=DEV, generator=g) * 0.5).to(BF16)


def _same(st, std, hs, hsd, rows, what):
    assert torch.equal(_bits(hs), _bits(hsd)), what + ": hidden states"
    assert torch.equal(_bits(st.kcache[:, :, :, rows]), _bits(std.kcache[:, :, :, rows])), what + ": k cache"
    assert torch.equal(_bits(st.vcache[:, :, :, rows]), _bits(std.vcache[:, :, :, rows])), what + ": v cache"
    assert bool(torch.isfinite(hs.float()).all()), what


def test_prefill_of_259_rows_then_an_append_of_32_equal_the_bf16_engine():
    """Which products multiply their codes in the kernel (256 CUs): all four of the 32-row append (glds<64, 128, 2>, split K), and
    o_proj of the 259-row prefill (glds<96, 128, 2>, 4 splits, the RMSNorm in the reduction).  q/k/v, gate / up and down_proj of the
    259-row prefill run on the whole-M kernel, which has no W4 mode: they keep the expansion into the workspace's scratch (answer 0)."""
    from spatialrgpt_amd import _lib, ops

    eng, engd = _engines()
    if _lib.load().srgpt_device_cus() == 256:
        ik = lambda M, N, K, swiglu=False: ops.gemm_w4_in_kernel(M, N, K, swiglu=swiglu)  # noqa: E731
        assert [ik(TA, QW, HID), ik(TA, HID, HQ * D), ik(TA, INTER, HID, True), ik(TA, HID, INTER)] == [True] * 4
        assert [ik(T0, QW, HID), ik(T0, HID, HQ * D), ik(T0, INTER, HID, True), ik(T0, HID, INTER)] == [False, True, False, False]
    x = _x((1, T0 + TA, HID), 7)
    st, std = eng.new_state(1, 320, 2), engd.new_state(1, 320, 2)
    _, _, hs = eng.prefill(x[:, :T0].contiguous(), max_new=2, hidden_states=True, state=st)
    _, _, hsd = engd.prefill(x[:, :T0].contiguous(), max_new=2, hidden_states=True, state=std)
    _same(st, std, hs, hsd, slice(0, T0), "259-row prefill")
    _, _, hs = eng.append(st, x[:, T0:].contiguous(), hidden_states=True)
    _, _, hsd = engd.append(std, x[:, T0:].contiguous(), hidden_states=True)
    assert st.pos.tolist() == std.pos.tolist() == [T0 + TA]
    _same(st, std, hs, hsd, slice(0, T0 + TA), "32-row append over 259 cached rows")


def test_batched_prefill_of_3_x_200_rows_stays_bit_equal_through_the_expansion():
    """M = 600: every product on the 256 x 256 tiles, which have no W4 kernel"""
    from spatialrgpt_amd import _lib, ops

    eng, engd = _engines()
    if _lib.load().srgpt_device_cus() == 256:
        assert not any(ops.gemm_w4_in_kernel(600, N, K, swiglu=s) for N, K, s in ((QW, HID, False), (HID, HQ * D, False),
                                                                                  (INTER, HID, True), (HID, INTER, False)))
    x = _x((3, 200, HID), 9)
    st, std = eng.new_state(3, 208, 2), engd.new_state(3, 208, 2)
    _, _, hs = eng.prefill(x, max_new=2, hidden_states=True, state=st)
    _, _, hsd = engd.prefill(x, max_new=2, hidden_states=True, state=std)
    _same(st, std, hs, hsd, slice(0, 200), "3 x 200-row prefill")
