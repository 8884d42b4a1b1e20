"""Prefix reuse end to end on tiny_fp32.npz, through `model.generate(input_ids, images=..., depths=..., masks=...)` only -- what an
unchanged caller sends: the whole conversation every turn, the same media.  With `prefix_reuse = True` a follow-up continues the last
request's KV cache over the rows both prompts share and skips the towers (model.last_reuse says what happened); its ids are the
ORACLE's over the whole conversation, its teacher-forced logits lie within 2e-4 * max|logits| of a `prefix_reuse = False` model's on
the same call (rows served from the cache were multiplied at another M: the bar tests/test_gpu_append_generate.py holds a second
turn to), and what does not depend on M is bit for bit: the gathered inputs_embeds, and the turn against the hand-driven
truncate / append / greedy_decode.  A miss is the path of a model without the switch, bit for bit."""
import functools

import pytest
import torch

from tests.test_gpu_append_generate import SEG2, _probe
from tests.test_gpu_pipeline import _engine, _to_dev
from tests.util import assert_close, load_tiny, teacher_forced_decode_logits

pytestmark = pytest.mark.gpu
DEV = "cuda"
N1, N2 = 6, 5
T_IMG = 196  # rows an <image> sentinel becomes
GREEDY = dict(do_sample=False, eos_token_id=None)


def _pair():
    """(model with the switch on, model without it, the fixture's inputs on the device)"""
    on, cfg, dtype, w, inp, ref = _engine("tiny_fp32.npz")
    off = _engine("tiny_fp32.npz")[0]
    on.prefix_reuse = True
    return on, off, _to_dev(inp)


def _media(d, **over):
    return dict(dict(images=d["images"], depths=d["depths"], masks=d["masks"]), **over)


@functools.lru_cache(maxsize=None)
def _oracle(ids: tuple, n_masks: int, n: int):
    """greedy ids of the oracle (CPU) over a whole conversation on the fixture's media (its first n_masks masks); computed once"""
    from oracle import srgpt_oracle as so

    cfgd, dtype, w, inp, ref = load_tiny("tiny_fp32.npz")
    ocfg = so.SrgptConfig(**{k: v for k, v in cfgd.items() if k in so.SrgptConfig.__dataclass_fields__})
    return so.generate(w, ocfg, torch.tensor([list(ids)]), inp["images"], inp["depths"], [inp["masks"][0][:n_masks]], max_new_tokens=n)


def _follow_up(d, ids1, first=None):
    return torch.cat([d["input_ids"] if first is None else first, ids1, torch.tensor(SEG2, device=DEV)], 1)


def _check_against_off(on, off, ids2, media, got, n=N2, oracle_masks=2, probe=(7, 21, 3)):
    """the follow-up `got` of the reuse model against the same call on the model without the switch: the margin condition on the
    reuse-off logits, ids (the oracle's too), then the teacher-forced logits of both states"""
    t_off = off.generate(ids2, **media, **GREEDY, max_new_tokens=n, return_dict_in_generate=True)
    emb = off.engine.prepare_inputs(ids2, media["images"], media["depths"], media["masks"], None)[0]
    st = off.engine.prefill(emb, max_new=n + 1, fresh_state=True)[0]
    steps = teacher_forced_decode_logits(off.engine, st, t_off.sequences)[0]  # [n, V]: the reuse-off logits at every generated position
    bar = 2e-4 * float(steps.abs().max())
    top = steps.topk(2, -1).values
    margin = float((top[:, 0] - top[:, 1]).min())
    print(f"\nreuse-off top-2 margin {margin:.4e}, bar {bar:.4e}")
    assert margin > 2 * bar, "the segment puts a generated position inside the bar: choose another segment"
    assert torch.equal(got, t_off.sequences), (got.tolist(), t_off.sequences.tolist())
    if oracle_masks is not None:
        want = _oracle(tuple(ids2[0].tolist()), oracle_masks, n)
        assert torch.equal(got.cpu(), want), (got.tolist(), want.tolist())
    la, lb = _probe(on, on.reuse_record.state, list(probe)), _probe(off, t_off.past_key_values, list(probe))
    print(f"teacher-forced max |d| {float((la - lb).abs().max()):.4e}, bar {2e-4 * float(lb.abs().max()):.4e}")
    assert_close(la, lb, 2e-4 * float(lb.abs().max()), 0, "teacher-forced logits: prefix reuse vs the request without it")


def _check_bits(on, off, first_call, ids2, media, L, got, stages, n=N2):
    """what does not depend on M, bit for bit: the gathered inputs_embeds == prepare_inputs on the same arguments; ids and final
    logits == the hand-driven continuation (generate(return_dict_in_generate) -> truncate(L) -> append -> greedy_decode)"""
    emb = off.engine.prepare_inputs(ids2, media["images"], media["depths"], media["masks"], None)[0]
    assert torch.equal(stages["inputs_embeds"], emb)
    final = on.reuse_record.state.logits.clone()
    st = off.generate(**first_call, return_dict_in_generate=True).past_key_values
    st.truncate(L)
    off.engine.append(st, emb[:, L:])
    hand = off.engine.greedy_decode(st, n, eos_token_id=None)
    assert torch.equal(got, hand), (got.tolist(), hand.tolist())
    assert torch.equal(final, st.logits)


def test_switch_off_retains_nothing():
    model, cfg, dtype, w, inp, ref = _engine("tiny_fp32.npz")
    d = _to_dev(inp)
    assert model.prefix_reuse is False and model.last_reuse is None and model.reuse_record is None
    out = model.generate(d["input_ids"], **_media(d), **GREEDY, max_new_tokens=N1)
    assert torch.equal(out.cpu(), ref["new_ids"][:, :N1])
    assert model.last_reuse is None and model.reuse_record is None and model._reuse is None


def test_two_turns():
    on, off, d = _pair()
    T = d["input_ids"].shape[1] - 1 + T_IMG
    first = dict(input_ids=d["input_ids"], **_media(d), **GREEDY, max_new_tokens=N1)
    ids1 = on.generate(**first)
    assert on.last_reuse == dict(mode="fresh", rows_reused=0, rows_appended=T, towers_skipped=False, regions_common=0)
    assert torch.equal(ids1, off.generate(**first))  # the first request under the switch is the request without it
    rec = on.reuse_record
    assert rec.state is not on.engine._state and rec.n_rows == T and rec.n_gen == N1 and rec.live_len == T + N1 - 1
    assert rec.state.max_pos == min(T + N1 + on.cache_reserve, on.engine.w.rope_len)
    ids2 = _follow_up(d, ids1)
    on.reuse_stages = stages = {}
    got = on.generate(ids2, **_media(d), **GREEDY, max_new_tokens=N2)
    L = T + N1 - 1
    assert on.last_reuse == dict(mode="append", rows_reused=L, rows_appended=ids2.shape[1] - 1 + T_IMG - L, towers_skipped=True,
                                 regions_common=2)
    assert on.reuse_record.state is rec.state and on.reuse_record.n_rows == T + N1 + len(SEG2[0])
    _check_bits(on, off, first, ids2, _media(d), L, got, stages)
    _check_against_off(on, off, ids2, _media(d), got)


def test_the_demo_shape_a_second_region_joins():
    """turn 1: one <mask> <depth> pair and masks[:1]; turn 2's prompt adds the second pair and `masks` holds both"""
    on, off, d = _pair()
    ids_a, tail = d["input_ids"][:, :10], d["input_ids"][:, 10:]
    assert ids_a[0].tolist().count(120) == 1 and tail[0].tolist().count(120) == 1
    m1 = _media(d, masks=[d["masks"][0][:1].clone()])
    T = ids_a.shape[1] - 1 + T_IMG
    first = dict(input_ids=ids_a, **m1, **GREEDY, max_new_tokens=N1)
    ids1 = on.generate(**first)
    assert torch.equal(ids1.cpu(), _oracle(tuple(ids_a[0].tolist()), 1, N1))
    ids2 = torch.cat([ids_a, ids1, tail], 1)
    on.reuse_stages = stages = {}
    got = on.generate(ids2, **_media(d), **GREEDY, max_new_tokens=N2)
    L = T + N1 - 1
    assert on.last_reuse == dict(mode="append", rows_reused=L, rows_appended=tail.shape[1] + 1, towers_skipped=True, regions_common=1)
    _check_bits(on, off, first, ids2, _media(d), L, got, stages)
    _check_against_off(on, off, ids2, _media(d), got)


@pytest.mark.parametrize("what", ["images", "depths"])
def test_a_changed_medium_is_a_fresh_request(what):
    """one element of the image / of the depth changed: the path of a model without the switch, bit for bit"""
    on, off, d = _pair()
    ids1 = on.generate(d["input_ids"], **_media(d), **GREEDY, max_new_tokens=N1)
    ids2 = _follow_up(d, ids1)
    changed = d[what].clone()
    changed[0, 1, 200, 100] += 1 / 32
    media = _media(d, **{what: changed})
    got = on.generate(ids2, **media, **GREEDY, max_new_tokens=N2)
    assert on.last_reuse["mode"] == "fresh" and on.last_reuse["rows_reused"] == 0 and not on.last_reuse["towers_skipped"]
    t_off = off.generate(ids2, **media, **GREEDY, max_new_tokens=N2, return_dict_in_generate=True)
    assert torch.equal(got, t_off.sequences) and torch.equal(on.reuse_record.state.logits, t_off.past_key_values.logits)
    assert torch.equal(got, off.generate(ids2, **media, **GREEDY, max_new_tokens=N2))
    # the record was replaced: the unchanged medium is now the miss, the changed one the hit
    on.generate(ids2, **_media(d), **GREEDY, max_new_tokens=N2)
    assert on.last_reuse["mode"] == "fresh"
    on.generate(ids2, **media, **GREEDY, max_new_tokens=N2)
    assert on.last_reuse["mode"] == "fresh"  # (the request in between replaced it again)
    on.generate(ids2, **media, **GREEDY, max_new_tokens=N2)
    assert on.last_reuse["mode"] == "append" and on.last_reuse["rows_reused"] == ids2.shape[1] - 1 + T_IMG - 1
    # one medium absent where the other request had it counts as differing
    on.generate(ids2, **_media(d, depths=None), **GREEDY, max_new_tokens=N2)
    assert on.last_reuse["mode"] == "fresh"


def test_an_earlier_mask_changed_reuse_stops_at_the_first_region_row():
    """regions_common == 0: the rows in front of the first <mask> row are served from the cache, the towers still do not run; from
    there on the request is an append, held to the append's bar against the model without the switch"""
    on, off, d = _pair()
    ids1 = on.generate(d["input_ids"], **_media(d), **GREEDY, max_new_tokens=N1)
    ids2 = _follow_up(d, ids1)
    m = d["masks"][0].clone()
    m[0, 100:140, 100:140] = 1 - m[0, 100:140, 100:140]
    media = _media(d, masks=[m])
    got = on.generate(ids2, **media, **GREEDY, max_new_tokens=N2)
    row = d["input_ids"][0].tolist().index(120) - 1 + T_IMG  # the first <mask> id stands behind the <image> sentinel
    assert on.last_reuse == dict(mode="append", rows_reused=row, rows_appended=ids2.shape[1] - 1 + T_IMG - row, towers_skipped=True,
                                 regions_common=0)
    _check_against_off(on, off, ids2, media, got, oracle_masks=None)
    # a LATER mask changed: the first region's rows still serve
    on2, _, _ = _pair()
    on2.generate(d["input_ids"], **_media(d), **GREEDY, max_new_tokens=N1)
    m = d["masks"][0].clone()
    m[1, 0, 0] = 1 - m[1, 0, 0]
    on2.generate(ids2, **_media(d, masks=[m]), **GREEDY, max_new_tokens=N2)
    second = [i for i, t in enumerate(d["input_ids"][0].tolist()) if t == 120][1] - 1 + T_IMG
    assert on2.last_reuse["regions_common"] == 1 and on2.last_reuse["rows_reused"] == second and on2.last_reuse["mode"] == "append"


def test_partial_text_hits():
    on, off, d = _pair()
    T = d["input_ids"].shape[1] - 1 + T_IMG
    first = dict(input_ids=d["input_ids"], **_media(d), **GREEDY, max_new_tokens=N1)
    ids1 = on.generate(**first)
    # an id changed in the middle of turn 1's question
    ids2 = _follow_up(d, ids1)
    ids2[0, 8] = 14
    got = on.generate(ids2, **_media(d), **GREEDY, max_new_tokens=N2)
    assert on.last_reuse["mode"] == "append" and on.last_reuse["rows_reused"] == 8 - 1 + T_IMG and on.last_reuse["regions_common"] == 2
    _check_against_off(on, off, ids2, _media(d), got)
    # a generated id replaced in the re-sent answer (a re-tokenised answer)
    on, off, d = _pair()
    ids1 = on.generate(**first)
    k = 3
    ids2 = _follow_up(d, ids1)
    ids2[0, d["input_ids"].shape[1] + k] = 50
    got = on.generate(ids2, **_media(d), **GREEDY, max_new_tokens=N2)
    assert on.last_reuse["mode"] == "append" and on.last_reuse["rows_reused"] == T + k
    _check_against_off(on, off, ids2, _media(d), got)


def test_the_same_request_twice():
    on, off, d = _pair()
    T = d["input_ids"].shape[1] - 1 + T_IMG
    call = dict(input_ids=d["input_ids"], **_media(d), **GREEDY, max_new_tokens=N1)
    a = on.generate(**call)
    b = on.generate(**call)
    assert on.last_reuse == dict(mode="append", rows_reused=T - 1, rows_appended=1, towers_skipped=True, regions_common=2)
    assert torch.equal(a, b)
    c = on.generate(**call)  # and a third time, over the state the second one left
    assert on.last_reuse["rows_reused"] == T - 1 and torch.equal(a, c)
    _check_against_off(on, off, d["input_ids"], _media(d), c, n=N1)


def test_follow_up_after_a_turn_cut_by_eos():
    """turn 1 ends in an EOS id: the device position ran one step ahead of the kept ids (the setup of _two_turns(eos_at=2))"""
    on, off, d = _pair()
    T = d["input_ids"].shape[1] - 1 + T_IMG
    free = off.generate(d["input_ids"], **_media(d), **GREEDY, max_new_tokens=N1)[0].tolist()
    eos = free[2]
    keep = free.index(eos) + 1
    assert keep < N1
    ids1 = on.generate(d["input_ids"], **_media(d), do_sample=False, max_new_tokens=N1, eos_token_id=eos, pad_token_id=0)
    st = on.reuse_record.state
    assert ids1.shape[1] == keep and int(ids1[0, -1]) == eos and on.reuse_record.n_gen == keep
    assert int(st.pos[0]) > st.seq_len(), "the device position did not run ahead: the rollback is not exercised"
    ids2 = _follow_up(d, ids1)
    got = on.generate(ids2, **_media(d), **GREEDY, max_new_tokens=N2)
    assert on.last_reuse["mode"] == "append" and on.last_reuse["rows_reused"] == T + keep - 1
    assert int(st.pos[0]) == st.seq_len() == ids2.shape[1] - 1 + T_IMG + N2 - 1
    _check_against_off(on, off, ids2, _media(d), got)


def test_a_follow_up_that_does_not_fit_the_cache_is_a_fresh_request():
    on, off, d = _pair()
    on.cache_reserve = off.cache_reserve = 8
    n = 4
    ids1 = on.generate(d["input_ids"], **_media(d), **GREEDY, max_new_tokens=n)
    small = on.reuse_record.state
    ids2 = _follow_up(d, ids1)  # T + 4 + 7 rows + 4 new tokens against T + 4 + 8 positions
    got = on.generate(ids2, **_media(d), **GREEDY, max_new_tokens=n)
    assert on.last_reuse["mode"] == "fresh" and on.last_reuse["rows_reused"] == 0 and on.reuse_record.state is not small
    t_off = off.generate(ids2, **_media(d), **GREEDY, max_new_tokens=n, return_dict_in_generate=True)
    assert torch.equal(got, t_off.sequences) and torch.equal(on.reuse_record.state.logits, t_off.past_key_values.logits)
    ids3 = torch.cat([ids2, got, torch.tensor([[9, 4]], device=DEV)], 1)
    got3 = on.generate(ids3, **_media(d), **GREEDY, max_new_tokens=n)  # the next request reuses the new state
    assert on.last_reuse["mode"] == "append" and on.last_reuse["rows_reused"] == ids2.shape[1] - 1 + T_IMG + n - 1
    _check_against_off(on, off, ids3, _media(d), got3, n=n, probe=(7, 21))  # 3 spare positions: the pending id + 2
    # more new tokens than the retained state was built for: fresh as well
    on, off, d = _pair()
    on.generate(d["input_ids"], **_media(d), **GREEDY, max_new_tokens=n)
    on.generate(d["input_ids"], **_media(d), **GREEDY, max_new_tokens=on.reuse_record.state.max_new + 1)
    assert on.last_reuse["mode"] == "fresh" and on.reuse_record.n_gen == on.cache_reserve + 1


def test_sampling_with_top_k_1_under_reuse_equals_greedy():
    on, off, d = _pair()
    ids1 = on.generate(d["input_ids"], **_media(d), **GREEDY, max_new_tokens=N1)
    ids2 = _follow_up(d, ids1)
    greedy = on.generate(ids2, **_media(d), **GREEDY, max_new_tokens=N2)
    assert on.last_reuse["mode"] == "append"
    drawn = on.generate(ids2, **_media(d), do_sample=True, temperature=0.7, top_k=1, eos_token_id=None, max_new_tokens=N2)
    assert on.last_reuse["mode"] == "append" and on.last_reuse["rows_reused"] == ids2.shape[1] - 1 + T_IMG - 1
    assert torch.equal(drawn, greedy)
    # the logits processors see the turn's own ids, as on every other path
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    assert torch.equal(on.generate(ids2, **_media(d), **GREEDY, max_new_tokens=N2, **kw),
                       off.generate(ids2, **_media(d), **GREEDY, max_new_tokens=N2, **kw))
    assert on.last_reuse["mode"] == "append"


def test_what_the_reuse_path_does_not_serve_leaves_the_record_alone():
    on, off, d = _pair()
    ids1 = on.generate(d["input_ids"], **_media(d), **GREEDY, max_new_tokens=N1)
    rec, last = on.reuse_record, dict(on.last_reuse)
    ids2 = _follow_up(d, ids1)
    on.generate(ids2, **_media(d), do_sample=False, num_beams=2, max_new_tokens=3, eos_token_id=None)
    on.generate(ids2.repeat(2, 1), images=d["images"].repeat(2, 1, 1, 1), depths=d["depths"].repeat(2, 1, 1, 1), masks=d["masks"] * 2,
                **GREEDY, max_new_tokens=3)
    on.generate(ids2, **_media(d), **GREEDY, max_new_tokens=3, return_dict_in_generate=True)
    assert on.reuse_record is rec and on.last_reuse == last
    on.generate(ids2, **_media(d), **GREEDY, max_new_tokens=N2)
    assert on.last_reuse["mode"] == "append"
    # the caller's tensors are not the record's: writing into them afterwards cannot fake a hit
    d["images"][0, 0, 0, 0] += 1.0
    on.generate(ids2, **_media(d), **GREEDY, max_new_tokens=N2)
    assert on.last_reuse["mode"] == "fresh"
    # replacing weights drops the record
    on.resize_token_embeddings(on.engine.w.vocab + 2)
    assert on.reuse_record is None
