"""CPU: generation.plan_lookup, the pure decision behind LlavaLlamaModel._lookup_plan -- which requests with
`prompt_lookup_num_tokens=K` run lookup steps, with how many drafts, and what the others are told."""
from spatialrgpt_amd.generation import plan_lookup, resolve_generation

GEOM = dict(vocab=3002, heads=4, kv_heads=1, head_dim=128, bf16=True)  # tests/test_gpu_lookup.py's: G = 4, four rows per step
SAMPLED = dict(do_sample=True, temperature=0.2)  # the demo's call (top_k 50 from the transformers default)


def _plan(batch=1, processors=False, lookup_sampling=False, geom=None, **kw):
    g = resolve_generation({}, max_new_tokens=8, **kw)
    return plan_lookup(g, batch, processors, lookup_sampling, **dict(GEOM, **(geom or {})))


def test_greedy_requests_are_planned_as_before():
    assert _plan(prompt_lookup_num_tokens=3) == (3, "K = 3 drafts per step")
    assert _plan(prompt_lookup_num_tokens=2) == (2, "K = 2 drafts per step")
    assert _plan(prompt_lookup_num_tokens=10) == (3, "K = 3 drafts per step (asked for 10)")  # G = 4: 16 columns / 4 - 1
    # the switch does not matter to a greedy request, nor do sampling keywords without do_sample
    assert _plan(prompt_lookup_num_tokens=3, lookup_sampling=True) == (3, "K = 3 drafts per step")
    assert _plan(prompt_lookup_num_tokens=3, temperature=0.2, top_k=50) == (3, "K = 3 drafts per step")
    assert _plan(prompt_lookup_num_tokens=3, do_sample=True, temperature=0.0)[0] == 3  # temperature 0: the greedy loop
    for off in (dict(), dict(prompt_lookup_num_tokens=0), dict(prompt_lookup_num_tokens=None)):
        assert _plan(**off) == (None, "prompt_lookup_num_tokens not set")
    # other geometries: no grouped heads on the matrix-pipe route, and the composed route's 16 rows
    assert _plan(prompt_lookup_num_tokens=20, geom=dict(heads=4, kv_heads=4))[0] == 15
    assert _plan(prompt_lookup_num_tokens=20, geom=dict(bf16=False))[0] == 15
    assert _plan(prompt_lookup_num_tokens=20, geom=dict(heads=32, kv_heads=8))[0] == 3
    assert _plan(prompt_lookup_num_tokens=3, geom=dict(heads=8, kv_heads=1)) == (1, "K = 1 drafts per step (asked for 3)")
    assert _plan(prompt_lookup_num_tokens=20, geom=dict(heads=16, kv_heads=1))[0] == 15  # G = 16 is no matrix-pipe route


def test_sampling_with_the_switch_on_gives_k_clamped_as_today():
    assert _plan(prompt_lookup_num_tokens=3, lookup_sampling=True, **SAMPLED) == (3, "K = 3 drafts per step")
    assert _plan(prompt_lookup_num_tokens=10, lookup_sampling=True, **SAMPLED) == (3, "K = 3 drafts per step (asked for 10)")
    # settings of the full sampler are served too
    assert _plan(prompt_lookup_num_tokens=2, lookup_sampling=True, do_sample=True, temperature=0.7, top_k=0, top_p=0.9)[0] == 2
    assert _plan(prompt_lookup_num_tokens=2, lookup_sampling=True, do_sample=True, temperature=0.7, top_k=200)[0] == 2


def test_sampling_with_the_switch_off_says_so():
    k, why = _plan(prompt_lookup_num_tokens=3, **SAMPLED)
    assert k is None and "do_sample" in why and "lookup_sampling" in why
    k, why = _plan(prompt_lookup_num_tokens=3, do_sample=True, temperature=0.7, top_k=20, top_p=0.9)
    assert k is None and "do_sample" in why


def test_beams_batches_and_processors_keep_their_reasons():
    for on in (False, True):
        assert _plan(prompt_lookup_num_tokens=3, lookup_sampling=on, num_beams=2, **SAMPLED) == (None, "num_beams > 1")
        assert _plan(prompt_lookup_num_tokens=3, lookup_sampling=on, num_beams=2) == (None, "num_beams > 1")
        assert _plan(prompt_lookup_num_tokens=3, lookup_sampling=on, batch=2) == (None, "batch 2: the lookup step takes one sequence")
        assert _plan(prompt_lookup_num_tokens=3, lookup_sampling=on, processors=True) == (None, "logits processors are on")
    assert _plan(prompt_lookup_num_tokens=3, lookup_sampling=True, batch=2, **SAMPLED)[1] == "batch 2: the lookup step takes one sequence"
    assert _plan(prompt_lookup_num_tokens=3, lookup_sampling=True, processors=True, **SAMPLED) == (None, "logits processors are on")


def test_a_vocabulary_no_device_sampler_serves_stays_plain():
    k, why = _plan(prompt_lookup_num_tokens=3, lookup_sampling=True, geom=dict(vocab=262145), **SAMPLED)
    assert k is None and "do_sample" in why and "262145" in why
    assert _plan(prompt_lookup_num_tokens=3, lookup_sampling=True, geom=dict(vocab=262144), **SAMPLED)[0] == 3


def test_the_model_has_the_switch_and_it_is_off():
    import inspect

    from spatialrgpt_amd import builder
    from spatialrgpt_amd.model import LlavaLlamaModel

    assert inspect.signature(LlavaLlamaModel.__init__).parameters["lookup_sampling"].default is False
    assert inspect.signature(builder.load_pretrained_model).parameters["lookup_sampling"].default is False
