"""CPU: generation.plan_lookup with the `lookup_batch` switch -- which batches with `prompt_lookup_num_tokens=K` run batched lookup
steps, with how many drafts per row (the attention's columns and the 16-row weight pass both clamp K), what the others are told;
and, with the keyword left at its default, every answer of tests/test_host_lookup_plan.py as it was."""
import inspect

from spatialrgpt_amd.generation import plan_lookup, resolve_generation

GEOM = dict(vocab=3002, heads=4, kv_heads=1, head_dim=128, bf16=True)  # tests/test_gpu_lookup.py's: G = 4, four rows per sequence
G1 = dict(heads=4, kv_heads=4)   # G = 1: 16 attention columns per sequence
COMPOSED = dict(bf16=False)      # no matrix-pipe route: 16 rows per sequence
SAMPLED = dict(do_sample=True, temperature=0.2)


def _plan(batch=1, processors=False, lookup_sampling=False, geom=None, on=True, **kw):
    g = resolve_generation({}, max_new_tokens=8, **kw)
    extra = dict(lookup_batch=True) if on else {}
    return plan_lookup(g, batch, processors, lookup_sampling, **dict(GEOM, **(geom or {})), **extra)


def test_the_clamp_over_batch_sizes_and_geometries():
    # K = min(asked, attention cap - 1, 16 // batch - 1); asked for 20 everywhere
    want = {
        "G4": {2: 3, 4: 3, 5: 2, 8: 1},        # the attention's 16 / 4 columns cap K at 3; 16 // 5 - 1 = 2; 16 // 8 - 1 = 1
        "G1": {2: 7, 4: 3, 5: 2, 8: 1},        # 16 // 2 - 1 = 7
        "composed": {2: 7, 4: 3, 5: 2, 8: 1},
    }
    for name, geom in (("G4", None), ("G1", G1), ("composed", COMPOSED)):
        for batch, k in want[name].items():
            assert _plan(batch=batch, geom=geom, prompt_lookup_num_tokens=20) == (k, f"K = {k} drafts per step, batch {batch} (asked for 20)"), (name, batch)
            assert batch * (k + 1) <= 16
        # a K that fits is not remarked on
        assert _plan(batch=2, geom=geom, prompt_lookup_num_tokens=2) == (2, "K = 2 drafts per step, batch 2")
        assert _plan(batch=8, geom=geom, prompt_lookup_num_tokens=1) == (1, "K = 1 drafts per step, batch 8")
        # batch 9 and up: two rows per sequence do not fit one weight pass
        for batch in (9, 16, 17):
            k, why = _plan(batch=batch, geom=geom, prompt_lookup_num_tokens=3)
            assert k is None and why == f"batch {batch}: two rows per sequence exceed the 16-row weight pass of a step", (name, batch)
    # G = 8 leaves one draft per row whatever the batch (16 / 8 - 1), G = 16 is no matrix-pipe route
    assert _plan(batch=2, geom=dict(heads=8, kv_heads=1), prompt_lookup_num_tokens=3) == (1, "K = 1 drafts per step, batch 2 (asked for 3)")
    assert _plan(batch=2, geom=dict(heads=16, kv_heads=1), prompt_lookup_num_tokens=20)[0] == 7


def test_batch_one_with_the_switch_on_is_the_batch_one_plan():
    for kw in (dict(prompt_lookup_num_tokens=3), dict(prompt_lookup_num_tokens=10), dict(prompt_lookup_num_tokens=3, num_beams=2),
               dict(prompt_lookup_num_tokens=3, **SAMPLED), dict(prompt_lookup_num_tokens=0), dict()):
        for geom in (None, G1, COMPOSED):
            for ls in (False, True):
                assert _plan(batch=1, geom=geom, lookup_sampling=ls, **kw) == _plan(batch=1, geom=geom, lookup_sampling=ls, on=False, **kw)
    assert _plan(batch=1, prompt_lookup_num_tokens=3) == (3, "K = 3 drafts per step")
    assert _plan(batch=1, processors=True, prompt_lookup_num_tokens=3) == (None, "logits processors are on")


def test_what_a_batch_with_the_switch_on_still_runs_plain_and_why():
    for batch in (2, 4):
        assert _plan(batch=batch) == (None, "prompt_lookup_num_tokens not set")
        assert _plan(batch=batch, prompt_lookup_num_tokens=0) == (None, "prompt_lookup_num_tokens not set")
        assert _plan(batch=batch, prompt_lookup_num_tokens=3, num_beams=2) == (None, "num_beams > 1")
        assert _plan(batch=batch, prompt_lookup_num_tokens=3, num_beams=2, **SAMPLED) == (None, "num_beams > 1")
        assert _plan(batch=batch, prompt_lookup_num_tokens=3, processors=True) == (None, "logits processors are on")
        for ls in (False, True):  # the sampling switch does not serve a batch
            k, why = _plan(batch=batch, prompt_lookup_num_tokens=3, lookup_sampling=ls, **SAMPLED)
            assert k is None and why == (f"do_sample: batch {batch} draws from one Philox counter, rows that emit different numbers of ids "
                                         "would need one each")
        # do_sample at temperature 0 is the greedy loop, sampling keywords without do_sample do not matter
        assert _plan(batch=batch, prompt_lookup_num_tokens=3, do_sample=True, temperature=0.0)[0] == 3
        assert _plan(batch=batch, prompt_lookup_num_tokens=3, temperature=0.2, top_k=50)[0] == 3


def test_with_the_keyword_at_its_default_every_plan_is_as_before():
    """the calls of tests/test_host_lookup_plan.py, through the positional signature they use"""
    assert inspect.signature(plan_lookup).parameters["lookup_batch"].default is False
    assert list(inspect.signature(plan_lookup).parameters)[-1] == "lookup_batch"

    def old(batch=1, processors=False, lookup_sampling=False, geom=None, **kw):
        return _plan(batch, processors, lookup_sampling, geom, on=False, **kw)

    assert old(prompt_lookup_num_tokens=3) == (3, "K = 3 drafts per step")
    assert old(prompt_lookup_num_tokens=10) == (3, "K = 3 drafts per step (asked for 10)")
    assert old(prompt_lookup_num_tokens=20, geom=G1)[0] == 15 and old(prompt_lookup_num_tokens=20, geom=COMPOSED)[0] == 15
    assert old(prompt_lookup_num_tokens=3, geom=dict(heads=8, kv_heads=1)) == (1, "K = 1 drafts per step (asked for 3)")
    assert old() == (None, "prompt_lookup_num_tokens not set")
    assert old(prompt_lookup_num_tokens=3, lookup_sampling=True, **SAMPLED) == (3, "K = 3 drafts per step")
    assert old(prompt_lookup_num_tokens=3, **SAMPLED) == (None, "do_sample: the model's lookup_sampling switch is off")
    for ls in (False, True):
        assert old(prompt_lookup_num_tokens=3, lookup_sampling=ls, num_beams=2) == (None, "num_beams > 1")
        assert old(prompt_lookup_num_tokens=3, lookup_sampling=ls, processors=True) == (None, "logits processors are on")
        for batch in (2, 4, 9):
            assert old(prompt_lookup_num_tokens=3, lookup_sampling=ls, batch=batch) == (None, f"batch {batch}: the lookup step takes one sequence")
            assert old(prompt_lookup_num_tokens=3, lookup_sampling=ls, batch=batch, **SAMPLED)[1] == f"batch {batch}: the lookup step takes one sequence"
    k, why = old(prompt_lookup_num_tokens=3, lookup_sampling=True, geom=dict(vocab=262145), **SAMPLED)
    assert k is None and "262145" in why


def test_the_model_has_the_switch_and_it_is_off():
    from spatialrgpt_amd import builder
    from spatialrgpt_amd.model import LlavaLlamaModel

    assert inspect.signature(LlavaLlamaModel.__init__).parameters["lookup_batch"].default is False
    assert inspect.signature(builder.load_pretrained_model).parameters["lookup_batch"].default is False
