"""CPU: generation.plan_lookup with the third switch, `lookup_batch_sampling` -- which SAMPLED batches with
`prompt_lookup_num_tokens=K` run batched lookup steps (both batch switches on: the greedy batch's K), what the others are told, and
that with the switch off every answer is the one tests/test_host_lookup_plan_batch.py pins."""
import inspect
import itertools

from spatialrgpt_amd.generation import plan_lookup, resolve_generation

GEOM = dict(vocab=3002, heads=4, kv_heads=1, head_dim=128, bf16=True)  # tests/test_gpu_lookup.py's: G = 4, four rows per sequence
G1 = dict(heads=4, kv_heads=4)   # G = 1: 16 attention columns per sequence
COMPOSED = dict(bf16=False)      # no matrix-pipe route: 16 rows per sequence
DEMO = dict(do_sample=True, temperature=0.2, top_k=50)        # the demo's settings: the top-k-64 sampler
FULL = dict(do_sample=True, temperature=0.7, top_p=0.9)       # top-p without top-k: the full sampler
ONE_COUNTER = "do_sample: batch %d draws from one Philox counter, rows that emit different numbers of ids would need one each"


def _plan(batch=2, processors=False, lookup_sampling=False, geom=None, **kw):
    switches = {k: kw.pop(k) for k in ("lookup_batch", "lookup_batch_sampling") if k in kw}
    g = resolve_generation({}, max_new_tokens=8, **kw)
    return plan_lookup(g, batch, processors, lookup_sampling, **dict(GEOM, **(geom or {})), **switches)


BOTH = dict(lookup_batch=True, lookup_batch_sampling=True)


def test_both_switches_on_a_sampled_batch_gets_the_greedy_batchs_K():
    want = {
        "G4": {2: 3, 4: 3, 5: 2, 8: 1},        # the attention's 16 / 4 columns cap K at 3; 16 // 5 - 1 = 2; 16 // 8 - 1 = 1
        "G1": {2: 7, 4: 3, 5: 2, 8: 1},        # 16 // 2 - 1 = 7
        "composed": {2: 7, 4: 3, 5: 2, 8: 1},
    }
    for name, geom in (("G4", None), ("G1", G1), ("composed", COMPOSED)):
        for batch, k in want[name].items():
            for settings in (DEMO, FULL):
                got = _plan(batch=batch, geom=geom, prompt_lookup_num_tokens=20, **settings, **BOTH)
                assert got == (k, f"K = {k} drafts per step, batch {batch}, sampled (asked for 20)"), (name, batch)
                # the greedy batch's K at the same batch and geometry
                assert got[0] == _plan(batch=batch, geom=geom, prompt_lookup_num_tokens=20, lookup_batch=True)[0]
                assert batch * (k + 1) <= 16
        assert _plan(batch=2, geom=geom, prompt_lookup_num_tokens=2, **DEMO, **BOTH) == (2, "K = 2 drafts per step, batch 2, sampled")
        for batch in (9, 16):
            assert _plan(batch=batch, geom=geom, prompt_lookup_num_tokens=3, **DEMO, **BOTH) == (
                None, f"batch {batch}: two rows per sequence exceed the 16-row weight pass of a step")
    # lookup_sampling is the batch-1 switch: not consulted for a batch
    for ls in (False, True):
        assert _plan(batch=4, lookup_sampling=ls, prompt_lookup_num_tokens=3, **DEMO, **BOTH)[0] == 3
    # a greedy batch is told nothing new
    assert _plan(batch=4, prompt_lookup_num_tokens=3, **BOTH) == (3, "K = 3 drafts per step, batch 4")
    assert _plan(batch=4, prompt_lookup_num_tokens=3, do_sample=True, temperature=0.0, **BOTH) == (3, "K = 3 drafts per step, batch 4")


def test_no_device_sampler_for_the_vocabulary():
    for settings in (DEMO, FULL):
        assert _plan(batch=4, geom=dict(vocab=262145), prompt_lookup_num_tokens=3, **settings, **BOTH) == (
            None, "do_sample: no device sampler serves a vocabulary of 262145")
    assert _plan(batch=4, geom=dict(vocab=262144), prompt_lookup_num_tokens=3, **DEMO, **BOTH)[0] == 3


def test_beams_and_processors_keep_their_reasons():
    for batch in (2, 4):
        assert _plan(batch=batch, prompt_lookup_num_tokens=3, num_beams=2, **DEMO, **BOTH) == (None, "num_beams > 1")
        assert _plan(batch=batch, prompt_lookup_num_tokens=3, processors=True, **DEMO, **BOTH) == (None, "logits processors are on")
        assert _plan(batch=batch, **DEMO, **BOTH) == (None, "prompt_lookup_num_tokens not set")


def test_without_lookup_batch_the_third_switch_means_nothing():
    for batch, ls, settings in itertools.product((2, 4, 9), (False, True), ({}, DEMO, FULL)):
        got = _plan(batch=batch, lookup_sampling=ls, prompt_lookup_num_tokens=3, lookup_batch_sampling=True, **settings)
        assert got == (None, f"batch {batch}: the lookup step takes one sequence")


def test_with_the_switch_off_every_answer_is_todays():
    """every call with the new keyword absent, and with it False: the answers tests/test_host_lookup_plan_batch.py pins"""
    assert inspect.signature(plan_lookup).parameters["lookup_batch_sampling"].default is False
    cases = []
    for batch, ls, lb, geom in itertools.product((1, 2, 4, 5, 8, 9), (False, True), (False, True), (None, G1, COMPOSED, dict(vocab=262145))):
        for kw in (dict(), dict(prompt_lookup_num_tokens=3), dict(prompt_lookup_num_tokens=20), dict(prompt_lookup_num_tokens=3, num_beams=2),
                   dict(prompt_lookup_num_tokens=3, **DEMO), dict(prompt_lookup_num_tokens=3, **FULL),
                   dict(prompt_lookup_num_tokens=3, do_sample=True, temperature=0.0)):
            for proc in (False, True):
                cases.append(dict(batch=batch, lookup_sampling=ls, lookup_batch=lb, geom=geom, processors=proc, **kw))
    for c in cases:
        absent, off = _plan(**c), _plan(lookup_batch_sampling=False, **c)
        assert absent == off, c
        if c["batch"] == 1:  # the third switch never reaches a batch-1 request
            assert _plan(lookup_batch_sampling=True, **c) == absent, c
    # ... and they are today's: the sampled batch's reason, the greedy batch's K and words
    for batch in (2, 4):
        for ls in (False, True):
            assert _plan(batch=batch, lookup_sampling=ls, prompt_lookup_num_tokens=3, lookup_batch=True, **DEMO) == (None, ONE_COUNTER % batch)
            assert _plan(batch=batch, lookup_sampling=ls, prompt_lookup_num_tokens=3, lookup_batch=True, lookup_batch_sampling=False,
                         **DEMO) == (None, ONE_COUNTER % batch)
    assert _plan(batch=2, prompt_lookup_num_tokens=20, lookup_batch=True) == (3, "K = 3 drafts per step, batch 2 (asked for 20)")
    assert _plan(batch=8, prompt_lookup_num_tokens=1, lookup_batch=True) == (1, "K = 1 drafts per step, batch 8")
    assert _plan(batch=4, prompt_lookup_num_tokens=3) == (None, "batch 4: the lookup step takes one sequence")


def test_the_model_has_the_switch_and_it_is_off():
    from spatialrgpt_amd import builder
    from spatialrgpt_amd.model import LlavaLlamaModel

    assert inspect.signature(LlavaLlamaModel.__init__).parameters["lookup_batch_sampling"].default is False
    assert inspect.signature(builder.load_pretrained_model).parameters["lookup_batch_sampling"].default is False
