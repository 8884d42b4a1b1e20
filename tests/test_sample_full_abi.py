"""CPU: the full sampler's C entry points (srgpt_sample_full, the _ex forms of the decode entry points) refuse bad arguments on the
host before any launch, its workspace follows the documented formula, and generate() routes every setting to a device sampler."""
import ctypes

from tests.util import ROOT  # noqa: F401  (puts the repository root on sys.path)


def _fake_llm(vocab):
    from spatialrgpt_amd import _lib

    w = _lib.LlmWeights()
    w.dtype, w.hidden, w.inter, w.layers, w.heads, w.kv_heads, w.head_dim, w.vocab = _lib.BF16, 64, 128, 1, 4, 2, 16, vocab
    st = _lib.LlmState()
    st.batch, st.max_pos, st.max_new, st.ws_tokens = 1, 8, 4, 8
    for f in ("kcache", "vcache", "pos", "tok", "out_ids", "step", "ws", "logits", "sampling"):
        setattr(st, f, 256)  # never dereferenced: every check below fails before a launch
    return w, st


def test_sample_full_refuses_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    V = 128 * 2048
    rc = lib.srgpt_sample_full(None, 16, 16, None, 16, 1, 1000, None)
    assert rc == _lib.ERR_ARG and b"null" in lib.srgpt_last_error()
    rc = lib.srgpt_sample_full(16, 16, None, None, 16, 1, 1000, None)
    assert rc == _lib.ERR_ARG and b"null" in lib.srgpt_last_error()
    rc = lib.srgpt_sample_full(16, 16, 16, None, None, 1, 1000, None)
    assert rc == _lib.ERR_ARG and b"null" in lib.srgpt_last_error()
    rc = lib.srgpt_sample_full(16, 16, 16, None, 16, 0, 1000, None)
    assert rc == _lib.ERR_ARG
    rc = lib.srgpt_sample_full(16, 16, 16, None, 16, 1, V + 1, None)
    assert rc == _lib.ERR_UNSUPPORTED and b"vocabulary" in lib.srgpt_last_error()


def test_sample_full_workspace_formula():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    # keys u32 [B][V] + threshold pair (4 u32) per row + 128 slice maxima (value + index) per row
    for B, V in ((1, 32000), (3, 128256), (16, 128258), (8, 128 * 2048)):
        assert lib.srgpt_sample_full_ws_bytes(B, V) == B * (4 * V + 16 + 128 * 8)
    assert lib.srgpt_sample_full_ws_bytes(0, 100) == -1 and lib.srgpt_sample_full_ws_bytes(2, 0) == -1


def test_ex_entry_points_refuse_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    P = ctypes.POINTER
    null_w, null_st = ctypes.cast(None, P(_lib.LlmWeights)), ctypes.cast(None, P(_lib.LlmState))
    for kind in (_lib.SAMPLER_TOPK64, _lib.SAMPLER_FULL):
        assert lib.srgpt_llm_decode_step_ex(null_w, null_st, kind, None) == _lib.ERR_ARG
        assert lib.srgpt_llm_sample_first_ex(null_w, null_st, kind, None) == _lib.ERR_ARG
        g = _lib.vp()
        assert lib.srgpt_llm_decode_graph_create_ex(null_w, null_st, kind, None, ctypes.byref(g)) == _lib.ERR_ARG
    w, st = _fake_llm(vocab=32000)
    assert lib.srgpt_llm_decode_graph_create_ex(ctypes.byref(w), ctypes.byref(st), 1, None, None) == _lib.ERR_ARG  # null out
    for kind in (2, -1):
        rc = lib.srgpt_llm_decode_step_ex(ctypes.byref(w), ctypes.byref(st), kind, None)
        assert rc == _lib.ERR_ARG and b"sampler kind" in lib.srgpt_last_error()
        rc = lib.srgpt_llm_sample_first_ex(ctypes.byref(w), ctypes.byref(st), kind, None)
        assert rc == _lib.ERR_ARG and b"sampler kind" in lib.srgpt_last_error()
        g = _lib.vp()
        rc = lib.srgpt_llm_decode_graph_create_ex(ctypes.byref(w), ctypes.byref(st), kind, None, ctypes.byref(g))
        assert rc == _lib.ERR_ARG and b"sampler kind" in lib.srgpt_last_error()
    w, st = _fake_llm(vocab=128 * 2048 + 1)
    rc = lib.srgpt_llm_decode_step_ex(ctypes.byref(w), ctypes.byref(st), _lib.SAMPLER_FULL, None)
    assert rc == _lib.ERR_UNSUPPORTED and b"vocabulary" in lib.srgpt_last_error()
    rc = lib.srgpt_llm_sample_first_ex(ctypes.byref(w), ctypes.byref(st), _lib.SAMPLER_FULL, None)
    assert rc == _lib.ERR_UNSUPPORTED and b"vocabulary" in lib.srgpt_last_error()
    g = _lib.vp()
    rc = lib.srgpt_llm_decode_graph_create_ex(ctypes.byref(w), ctypes.byref(st), _lib.SAMPLER_FULL, None, ctypes.byref(g))
    assert rc == _lib.ERR_UNSUPPORTED and b"vocabulary" in lib.srgpt_last_error()


def test_every_sampling_setting_has_a_device_sampler():
    from spatialrgpt_amd import _lib
    from spatialrgpt_amd.ops import SamplingParams

    V = 128256
    pick = SamplingParams.sampler
    assert pick(0.2, 50, None, V) == pick(0.7, 50, 0.9, V) == pick(1.0, 0, None, V) == pick(1.0, None, 1.0, V) == _lib.SAMPLER_TOPK64
    for k, p in ((0, 0.9), (None, 0.9), (65, None), (1000, None), (200, 0.5), (V + 5, 0.8), (0, 0.0)):
        assert pick(0.7, k, p, V) == _lib.SAMPLER_FULL, (k, p)
    assert pick(0.7, 1000, None, 128 * 2048 + 1) is None and pick(0.0, 50, None, V) is None and pick(None, 50, None, V) is None
    # the top-k-64 sampler's own predicate keeps its meaning
    assert not SamplingParams.supported(0.7, 0, 0.9, V) and not SamplingParams.supported(0.7, 65, None, V)


def test_sample_workspace_formula():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    # candidates (key + index: 8 bytes) of 64 slots x 128 slices per row + 128 slice maxima (value + index) per row + the error word
    for B in (1, 3, 16):
        assert lib.srgpt_sample_ws_bytes(B) == B * 128 * 64 * 8 + B * 128 * 8 + 256
    assert lib.srgpt_sample_ws_bytes(0) == -1


# srgpt_llm_ws_bytes(weights, batch, max_tokens) as the build before the samplers' layouts moved to csrc/pick.h returned it:
# (config, weight format, batch, max_tokens) -> bytes.  native: the config's dtype; fp8: bf16 activations; fp8_w8a8: fp8_act set.
LLM_WS_BYTES = {
    ("tiny", "native", 1, 32): 327424, ("tiny", "native", 8, 32): 2609408,
    ("tiny", "fp8", 1, 32): 275712, ("tiny", "fp8", 8, 32): 2192128,
    ("tiny", "fp8_w8a8", 1, 32): 281088, ("tiny", "fp8_w8a8", 8, 32): 2234112,
    ("vila15_8b", "native", 1, 259): 84463872, ("vila15_8b", "native", 8, 259): 675702784,
    ("vila15_8b", "fp8", 1, 259): 84463872, ("vila15_8b", "fp8", 8, 259): 675702784,
    ("vila15_8b", "fp8_w8a8", 1, 259): 88178176, ("vila15_8b", "fp8_w8a8", 8, 259): 705415424,
}


def test_llm_workspace_bytes_are_unchanged():
    from spatialrgpt_amd import _lib
    from spatialrgpt_amd.config import SrgptConfig
    from tests.util import load_tiny

    lib = _lib.load()
    cfgs = {"tiny": (SrgptConfig(**load_tiny("tiny_fp32.npz")[0]), _lib.F32), "vila15_8b": (SrgptConfig.vila15_8b(), _lib.BF16)}
    for (name, fmt, B, T), want in LLM_WS_BYTES.items():
        cfg, native = cfgs[name]
        w = _lib.LlmWeights()
        w.dtype, w.hidden, w.inter, w.layers = native if fmt == "native" else _lib.BF16, cfg.hidden, cfg.inter, cfg.layers
        w.heads, w.kv_heads, w.head_dim, w.vocab = cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.vocab
        w.fp8_act = 1 if fmt == "fp8_w8a8" else 0
        assert lib.srgpt_llm_ws_bytes(ctypes.byref(w), B, T) == want, (name, fmt, B, T)
