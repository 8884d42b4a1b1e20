"""The Python surface of the append prefill on tiny_fp32.npz: generate(return_dict_in_generate=True) hands the state back,
generate(past_key_values=state) continues it turn by turn (truncate to the true live length, the pending token first, then the
segment), DecodeState.truncate + LlavaLlamaModel.append reuse a shared prefix, SrgptEngine.append chunks a long segment.  The
one-shot reference of a conversation is `_generate_from_embeds` over [spliced prompt | embed(ids of turn 1) | embed(segment 2)]:
what the reference's callers do today, re-sending the whole conversation."""
import pytest
import torch

from tests.test_gpu_pipeline import _engine, _to_dev
from tests.util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEG2 = [[5, 9, 33, 2, 17, 44, 8]]


def _setup():
    model, cfg, dtype, w, inp, ref = _engine("tiny_fp32.npz")
    d = _to_dev(inp)
    emb = model.engine.prepare_inputs(d["input_ids"], d["images"], d["depths"], d["masks"], None)[0]  # [1, T, H]
    return model, d, emb


def _probe(model, st, ids):
    """teacher-forced logits over a live handle: its pending token and `ids` appended, all positions' logits [1, 1 + len, V]"""
    pend = st.pending_ids()
    st.truncate(list(st.host_len))
    seg = torch.cat([pend[:, None], torch.tensor([ids], device=DEV)], 1)
    return model.engine.append(st, model.engine.embed_tokens(seg), all_logits=True)[1]


def test_return_dict_in_generate_returns_the_ids_and_the_state():
    model, d, emb = _setup()
    n, T = 6, emb.shape[1]
    plain = model.generate(**d, do_sample=False, max_new_tokens=n, eos_token_id=None)
    out = model.generate(**d, do_sample=False, max_new_tokens=n, eos_token_id=None, return_dict_in_generate=True)
    assert torch.equal(out.sequences, plain) and out["sequences"] is out.sequences
    st = out.past_key_values
    assert st.seq_len() == T + n - 1 and st is not model.engine._state  # the caller's own state, never the pooled one
    assert st.max_pos >= T + n + model.cache_reserve or st.max_pos == model.engine.w.rope_len
    assert int(st.pending_ids()[0]) == int(plain[0, -1])
    # the plain call still returns a tensor, and the keyword set to False changes nothing
    again = model.generate(**d, do_sample=False, max_new_tokens=n, eos_token_id=None, return_dict_in_generate=False)
    assert isinstance(again, torch.Tensor) and torch.equal(again, plain)


def _two_turns(eos_at=None, **gen_kw):
    """turn 1 (n1 = 6 tokens, or cut by an EOS id taken from its own greedy ids at index eos_at), turn 2 = SEG2 over the returned
    state -> its ids against the one-shot request over the whole conversation, and both handles' teacher-forced logits"""
    model, d, emb = _setup()
    eng = model.engine
    n1, n2, T = 6, 5, emb.shape[1]
    kw1 = dict(do_sample=False, max_new_tokens=n1, eos_token_id=None)
    if eos_at is not None:
        free = model.generate(**d, **kw1)[0].tolist()
        eos = free[eos_at]
        keep = free.index(eos) + 1
        assert keep < n1, "the EOS must cut the turn short, so that the run-ahead step has written past the kept tokens"
        kw1 = dict(do_sample=False, max_new_tokens=n1, eos_token_id=eos, pad_token_id=0)
    t1 = model.generate(**d, **kw1, return_dict_in_generate=True)
    ids1, st = t1.sequences, t1.past_key_values
    if eos_at is not None:
        assert ids1.shape[1] == keep and int(ids1[0, -1]) == eos
        assert int(st.pos[0]) > st.seq_len(), "the device position did not run ahead: the rollback is not exercised"
    assert st.seq_len() == T + ids1.shape[1] - 1
    seg2 = torch.tensor(SEG2, device=DEV)
    kw2 = dict(dict(do_sample=False, max_new_tokens=n2, eos_token_id=None), **gen_kw)
    t2 = model.generate(input_ids=seg2, past_key_values=st, return_dict_in_generate=True, **kw2)
    assert t2.past_key_values is st and st.seq_len() == T + ids1.shape[1] + seg2.shape[1] + n2 - 1 == int(st.pos[0])
    whole = torch.cat([emb, eng.embed_tokens(ids1), eng.embed_tokens(seg2)], 1)
    one = model.llm.generate(inputs_embeds=whole, return_dict_in_generate=True, **kw2)
    # teacher-forced: the same continuation through both handles, every position's logits (an id flipped inside the margin
    # would otherwise hide everything behind it)
    la, lb = _probe(model, st, [7, 21, 3]), _probe(model, one.past_key_values, [7, 21, 3])
    assert_close(la, lb, 2e-4 * float(lb.abs().max()), 0, "teacher-forced logits: two turns vs the one-shot request")
    assert torch.equal(t2.sequences, one.sequences), (t2.sequences.tolist(), one.sequences.tolist())
    return model, t2.sequences


def test_second_turn_over_the_returned_state_equals_the_one_shot_request():
    _two_turns()


def test_second_turn_after_a_turn_that_ended_in_eos():
    _two_turns(eos_at=2)


def test_second_turn_sampling_and_logits_processors():
    """the handle path runs the decode loop the pooled path runs: a draw with top_k = 1 is the argmax, and the logits processors
    see the turn's own ids -- two turns equal the one-shot request under repetition_penalty and no_repeat_ngram_size too"""
    model, greedy = _two_turns()
    _, drawn = _two_turns(do_sample=True, temperature=0.7, top_k=1)
    assert torch.equal(drawn, greedy)
    _two_turns(repetition_penalty=1.3, no_repeat_ngram_size=2)


def test_generate_over_a_state_refuses_what_it_does_not_serve():
    model, d, emb = _setup()
    t1 = model.generate(**d, do_sample=False, max_new_tokens=4, eos_token_id=None, return_dict_in_generate=True)
    st = t1.past_key_values
    seg = torch.tensor(SEG2, device=DEV)
    with pytest.raises(NotImplementedError):
        model.generate(input_ids=seg, past_key_values=st, num_beams=2, do_sample=False, max_new_tokens=4, eos_token_id=None)
    with pytest.raises(NotImplementedError):
        model.generate(input_ids=seg.repeat(2, 1), past_key_values=st, do_sample=False, max_new_tokens=4, eos_token_id=None)
    with pytest.raises(ValueError, match="cache_reserve"):
        model.generate(input_ids=seg, past_key_values=st, do_sample=False, max_new_tokens=st.max_new + 1, eos_token_id=None)
    model.cache_reserve = 8  # a state with 8 spare positions cannot take a 7-row segment + the pending token + 4 new tokens
    small = model.generate(**d, do_sample=False, max_new_tokens=4, eos_token_id=None, return_dict_in_generate=True).past_key_values
    with pytest.raises(ValueError, match="cache_reserve"):
        model.generate(input_ids=seg, past_key_values=small, do_sample=False, max_new_tokens=4, eos_token_id=None)
    assert small.seq_len() == emb.shape[1] + 3  # refused before anything was appended
    with pytest.raises(ValueError):
        small.truncate([small.seq_len() + 1])


def test_shared_prefix_truncate_then_append_equals_forward_over_the_concatenation():
    """st from forward(use_cache=True) on a prefix; per question: truncate to the prefix, append the question -> the logits of
    forward() over [prefix | question] at the bar of test_forward_surface_and_text_only; a question is unaffected by the one
    asked before it"""
    model, d, emb = _setup()
    am = torch.ones_like(d["input_ids"])
    vis = dict(images=d["images"], depths=d["depths"], masks=d["masks"])
    st = model.forward(input_ids=d["input_ids"], attention_mask=am, use_cache=True, **vis).past_key_values
    P = st.seq_len()
    assert P == emb.shape[1]
    questions = [torch.tensor([[11, 4, 27, 9, 30]], device=DEV), torch.tensor([[8, 8, 15, 2, 41, 6, 19, 3, 12]], device=DEV)]
    first = None
    for q in questions + questions[:1]:
        out = model.append(st.truncate(P), input_ids=q)
        assert out.past_key_values is st and st.seq_len() == P + q.shape[1] and out.logits.shape[:2] == (1, q.shape[1])
        ids = torch.cat([d["input_ids"], q], 1)
        ref = model.forward(input_ids=ids, attention_mask=torch.ones_like(ids), use_cache=False, **vis).logits
        assert_close(out.logits, ref[:, P:], 2e-4 * float(ref.abs().max()) * 2, 0, f"append of a {q.shape[1]}-token question vs forward()")
        if first is None:
            first = out.logits.clone()
    assert torch.equal(out.logits, first), "the first question, asked again after the second, gives other logits"
    # a padded segment appends the valid positions only; padded positions come back as zeros
    q = questions[0]
    padded = torch.cat([q, torch.zeros((1, 3), dtype=q.dtype, device=DEV)], 1)
    mask = torch.cat([torch.ones_like(q), torch.zeros((1, 3), dtype=q.dtype, device=DEV)], 1)
    out = model.append(st.truncate(P), input_ids=padded, attention_mask=mask)
    assert st.seq_len() == P + q.shape[1] and bool((out.logits[:, q.shape[1]:] == 0).all())
    assert_close(out.logits[:, :q.shape[1]], first, 2e-4 * float(first.abs().max()) * 2, 0, "padded segment: the valid positions")
    with pytest.raises(NotImplementedError):  # forward() keeps refusing a multi-token segment over a cache
        model(input_ids=q, past_key_values=st, attention_mask=torch.ones_like(q))


def test_chunked_append_equals_the_unchunked_one():
    """ws_tokens = 16: a 37-row segment runs as appends of 16 + 16 + 5 rows"""
    model, d, emb = _setup()
    eng = model.engine
    g = torch.Generator().manual_seed(9)
    x = (torch.randn((1, 47, emb.shape[2]), generator=g) * 0.5).to(emb.dtype).to(DEV)
    got = []
    for ws_tokens in (16, 64):
        st = eng.new_state(1, 128, 1, ws_tokens=ws_tokens)
        eng.prefill(x[:, :10], max_new=1, state=st)
        _, al, hs = eng.append(st, x[:, 10:], all_logits=True, hidden_states=True)
        assert al.shape[:2] == (1, 37) and hs.shape[1:3] == (1, 37) and st.host_len == [47] == st.pos.tolist()
        got.append((al, st.logits.clone()))
    tol = 2e-4 * float(got[1][0].abs().max()) * 2
    assert_close(got[0][0], got[1][0], tol, 0, "chunked append vs one append: all rows' logits")
    assert_close(got[0][1], got[1][1], tol, 0, "chunked append vs one append: st.logits")
    with pytest.raises(ValueError):  # a ragged long segment is not chunked
        eng.append(eng.new_state(1, 128, 1, ws_tokens=16), x[:, :20], lens=torch.tensor([20]))
    with pytest.raises(ValueError, match="KV cache full"):
        eng.append(eng.new_state(1, 32, 1), x[:, :40])
