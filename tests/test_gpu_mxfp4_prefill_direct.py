"""mxfp4_prefill_direct through the engine (srgpt_llm_weights::mxfp4_direct -> Prefill::layer_w4a16, model.hip), on two layers of
the Llama-3-8B geometry (hidden 4096, inter 14336, heads 32 / 8, a small vocabulary): an MXFP4 engine with the option on and one
with it off, built on the same codes, must return the same BITS -- all-position logits, last-position logits, both caches and
every hidden state -- for prefills of 225, 259 and 272 rows (q/k/v, gate/up and down_proj on the whole-M kernel: codes in the kernel
with the option, the bf16 expansion without), for a 32-row append and 8 greedy ids behind it, and for 273 rows and batches of 2
(other routes: the option changes nothing there).  A bf16 engine on the dequantised weights equals both in every hidden state and
both caches (its lm_head is another kernel -- bf16 instead of fp8 bytes -- so logits are compared between the MXFP4 engines only)."""
import functools

import pytest
import torch

from tests.test_gpu_mxfp4 import dequantised_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
HID, INTER, HQ, HKV, D = 4096, 14336, 32, 8, 128
QW = (HQ + 2 * HKV) * D
KW = dict(vit_hidden=64, vit_inter=176, vit_layers=2, vit_heads=4, image_size=42, patch_size=14, layers=2, vocab=4098,
          mask_token_id=4096, depth_token_id=4097, hidden=HID, inter=INTER, heads=HQ, kv_heads=HKV)


def _bits(t):
    return t.contiguous().view({BF16: torch.int16, torch.float32: torch.int32}[t.dtype])


@functools.lru_cache(maxsize=None)
def _engines():
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine
    from spatialrgpt_amd.weights import synth_state_dict

    sd = synth_state_dict(SrgptConfig(**KW), seed=5, dtype=BF16, device=DEV)
    on = SrgptEngine(SrgptConfig(**KW), dict(sd), device=DEV, dtype=BF16, rope_positions=512, llm_weight_format="mxfp4",
                     mxfp4_prefill_direct=True)
    off = SrgptEngine(SrgptConfig(**KW), dict(sd), device=DEV, dtype=BF16, rope_positions=512, llm_weight_format="mxfp4")
    assert on.mxfp4_prefill_direct is True and on.w.llm.mxfp4_direct == 1  # the option reached srgpt_llm_weights
    assert off.mxfp4_prefill_direct is False and off.w.llm.mxfp4_direct == 0
    for k in on.w.llm_q4:  # the same codes and scale bytes
        for (a, b) in zip(on.w.llm_q4[k][0] + on.w.llm_q4[k][1], off.w.llm_q4[k][0] + off.w.llm_q4[k][1]):
            assert torch.equal(a, b), k
    sdd = dequantised_state_dict(on, {k: v.cpu() for k, v in sd.items()})
    del sd
    bf = SrgptEngine(SrgptConfig(**KW), sdd, device=DEV, dtype=BF16, rope_positions=512)
    return on, off, bf


def _x(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, device=DEV, generator=g) * 0.5).to(BF16)


def _prefill(eng, x, cap, max_new=8):
    st = eng.new_state(x.shape[0], cap, max_new)
    _, al, hs = eng.prefill(x, max_new=max_new, all_logits=True, hidden_states=True, state=st)
    return st, al, hs


def _same_state(a, b, rows, what, logits=True):
    (sta, ala, hsa), (stb, alb, hsb) = a, b
    assert torch.equal(_bits(hsa), _bits(hsb)), what + ": hidden states"
    assert torch.equal(_bits(sta.kcache[:, :, :, rows]), _bits(stb.kcache[:, :, :, rows])), what + ": k cache"
    assert torch.equal(_bits(sta.vcache[:, :, :, rows]), _bits(stb.vcache[:, :, :, rows])), what + ": v cache"
    assert bool(torch.isfinite(hsa.float()).all()), what
    if logits:
        assert torch.equal(_bits(ala), _bits(alb)), what + ": all-position logits"
        assert torch.equal(_bits(sta.logits), _bits(stb.logits)), what + ": last-position logits"


def test_the_option_changes_which_products_read_codes_on_the_whole_m_kernel():
    from spatialrgpt_amd import _lib, ops

    if _lib.load().srgpt_device_cus() != 256:
        pytest.skip("the routes are recorded for 256 CUs")
    for T in (225, 259, 272):
        shapes = ((T, QW, HID, False), (T, HID, HQ * D, False), (T, INTER, HID, True), (T, HID, INTER, False))
        assert [ops.gemm_w4_in_kernel(M, N, K, swiglu=s) for M, N, K, s in shapes] == [False, True, False, False], T
        assert [ops.gemm_w4_in_kernel(M, N, K, swiglu=s, direct=True) for M, N, K, s in shapes] == [True] * 4, T


@pytest.mark.parametrize("T", [225, 259, 272])
def test_whole_m_prefill_equals_the_option_off_and_the_bf16_engine(T):
    on, off, bf = _engines()
    x = _x((1, T, HID), T)
    a, b, c = _prefill(on, x, 320), _prefill(off, x, 320), _prefill(bf, x, 320)
    _same_state(a, b, slice(0, T), "%d-row prefill, option on against off" % T)
    _same_state(a, c, slice(0, T), "%d-row prefill, option on against the bf16 engine" % T, logits=False)


def test_append_of_32_rows_then_8_greedy_ids():
    on, off, bf = _engines()
    x = _x((1, 259 + 32, HID), 7)
    head, tail = x[:, :259].contiguous(), x[:, 259:].contiguous()
    sts, outs = [], []
    for eng in (on, off, bf):
        st, _, _ = _prefill(eng, head, 320)
        _, al, hs = eng.append(st, tail, all_logits=True, hidden_states=True)
        sts.append(st)
        outs.append((st, al, hs))
    _same_state(outs[0], outs[1], slice(0, 291), "32-row append, option on against off")
    _same_state(outs[0], outs[2], slice(0, 291), "32-row append, option on against the bf16 engine", logits=False)
    ids = [eng.greedy_decode(st, 8) for eng, st in zip((on, off), sts[:2])]
    assert ids[0].shape == (1, 8) and torch.equal(ids[0], ids[1]), (ids[0].tolist(), ids[1].tolist())
    assert torch.equal(_bits(sts[0].kcache[:, :, :, :298]), _bits(sts[1].kcache[:, :, :, :298])), "k cache behind the greedy steps"


@pytest.mark.parametrize("B,T", [(1, 273), (2, 130), (2, 259)], ids=["1x273", "2x130", "2x259"])
def test_other_row_counts_and_batches(B, T):
    """273 rows leave the whole-M kernel; 2 x 130 = 260 rows stay on it with two sequences in the rotation; 2 x 259 rows take the
    256 x 256 tiles, which still expand"""
    on, off, bf = _engines()
    x = _x((B, T, HID), 11 * B + T)
    a, b, c = _prefill(on, x, 320), _prefill(off, x, 320), _prefill(bf, x, 320)
    _same_state(a, b, slice(0, T), "%d x %d rows, option on against off" % (B, T))
    _same_state(a, c, slice(0, T), "%d x %d rows, option on against the bf16 engine" % (B, T), logits=False)


def test_the_option_needs_the_mxfp4_format():
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.engine import SrgptEngine
    from spatialrgpt_amd.model import LlavaLlamaModel

    for cls in (SrgptEngine, LlavaLlamaModel):
        with pytest.raises(ValueError, match="mxfp4_prefill_direct"):
            cls(SrgptConfig(**KW), {}, device=DEV, dtype=BF16, rope_positions=512, llm_weight_format="native", mxfp4_prefill_direct=True)
    on, _, _ = _engines()
    with pytest.raises(AttributeError):
        on.mxfp4_prefill_direct = False  # read-only: set at construction
