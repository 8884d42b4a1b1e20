"""GPU: the full device sampler (csrc/sample.hip, srgpt_sample_full): every temperature / top_k / top_p over the whole vocabulary,
inside the captured decode step -- the settings the top-k-64 sampler does not serve (top_k > 64, top-p without top-k).

Parity is stated as in tests/test_gpu_sampling.py: the KEPT SET against HF's warper chain (`generation.warp_logits`) -- exact for
top-k, exact for top-p outside a 1e-5 band around the cut (the softmax mass is summed in another order than torch's) -- and the DRAWN
DISTRIBUTION by chi-square; plus determinism, graph replay == eager steps, and `model.generate` on the device."""
import pytest
import torch

from tests.draw_ref import warp_stable as _warp_stable
from tests.test_gpu_sampling import _chi2_crit, _logits, _peaked_model, _request

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAND = 1e-5


def _ops():
    from spatialrgpt_amd import ops

    return ops


def _check_kept(lg, temperature, top_k, top_p, seed=1, stable_oracle=False):
    from spatialrgpt_amd.generation import warp_logits
    ops = _ops()
    B, V = lg.shape
    sp = ops.SamplingParams(DEV, B).set(temperature, top_k, top_p, seed=seed)
    tok, kept = ops.sample_full(lg, sp, kept_mask=True)
    kept, tok = kept.cpu(), tok.cpu()
    scores = lg.cpu() / temperature
    want, cp = _warp_stable(scores, top_k, top_p)
    if not stable_oracle:
        want = warp_logits(lg.cpu(), temperature, top_k, top_p) > float("-inf")
    diff = kept ^ want
    p_on = top_p is not None and top_p < 1.0
    if not p_on:
        assert not bool(diff.any()), ("top-k kept set differs", int(diff.sum()))
    elif bool(diff.any()):
        # only entries whose oracle cumulative probability lies within the band around the cut may differ
        off = (cp[diff] - (1 - top_p)).abs()
        assert bool((off <= BAND).all()), ("top-p kept set differs outside the band", int(diff.sum()), float(off.max()))
    for b in range(B):
        assert bool(kept[b, tok[b]]), (b, int(tok[b]))  # the draw comes from the kept set
    return kept


SETTINGS = [(0.7, 0, 0.9), (1.0, 65, None), (1.3, 1000, 0.95), (0.5, 0, 0.5), (1.0, 0, 0.0), (1.0, "V+5", 0.8), (2.0, 128256, 0.99)]


@pytest.mark.parametrize("V", [32000, 128256, 128258])
@pytest.mark.parametrize("si", range(len(SETTINGS)))
def test_kept_set_equals_hf_warpers(V, si):
    temperature, top_k, top_p = SETTINGS[si]
    top_k = V + 5 if top_k == "V+5" else top_k
    B = (1, 3, 16)[(si + V) % 3]
    kept = _check_kept(_logits(B, V, seed=V + si), temperature, top_k, top_p)
    if top_p == 0.0:
        assert kept.sum(dim=1).tolist() == [1] * B


def test_planted_ties_at_the_kth_score():
    V, k = 128256, 1000
    lg = _logits(2, V, seed=11)
    for b in range(2):
        vals = lg[b].sort(descending=True).values
        c = vals[850]
        below = torch.nonzero(lg[b] < c).flatten()
        pick = below[torch.randperm(below.numel(), generator=torch.Generator().manual_seed(b))[:300].to(below.device)]
        lg[b, pick] = c  # 850 entries above c, 301 at c: the 1000-th largest is c, every tie is kept
    kept = _check_kept(lg, 1.0, k, None)
    assert kept.sum(dim=1).tolist() == [1151, 1151]
    _check_kept(lg, 0.8, k, 0.95)


def test_planted_ties_straddling_the_top_p_cut():
    V = 32000
    lg = torch.full((3, V), -30.0)
    ties = torch.tensor([5, 700, 701, 9000, 12000, 12001, 20000, 25000, 31000, 31999])
    lg[:, ties] = 0.0
    lg[:, 15000] = float(torch.log(torch.tensor(10.0)))
    # ascending: the -30 entries (mass ~3e-9), the 10 ties at 1/20 each (cumulative 0.05 .. 0.5), the top entry at 1/2.
    # top_p = 0.77: the cut 0.23 removes the 4 lowest-index ties (cumulative 0.20; the next is 0.25 -- far outside the band)
    kept = _check_kept(lg.to(DEV), 1.0, 0, 0.77, stable_oracle=True)
    want = torch.zeros(V, dtype=torch.bool)
    want[ties[4:]] = True
    want[15000] = True
    assert all(torch.equal(kept[b], want) for b in range(3))
    # top_p = 0 keeps exactly one entry: the highest index among tied maxima
    lg2 = _logits(2, V, seed=4).cpu()
    lg2[:, [3, 77, 30001]] = lg2.max() + 1.0
    kept = _check_kept(lg2.to(DEV), 1.0, 0, 0.0, stable_oracle=True)
    assert all(torch.nonzero(kept[b]).flatten().tolist() == [30001] for b in range(2))


def test_all_equal_row():
    V = 128256
    lg = torch.zeros((2, V), device=DEV)
    kept = _check_kept(lg, 1.0, 50, None)  # top-k keeps every tie
    assert bool(kept.all())
    kept = _check_kept(lg, 1.0, 0, 0.0, stable_oracle=True)
    assert all(torch.nonzero(kept[b]).flatten().tolist() == [V - 1] for b in range(2))
    kept = _check_kept(lg, 1.0, 0, 0.5, stable_oracle=True)  # the highest-index half survives (the cut lies in the band)
    assert abs(int(kept[0].sum()) - V // 2) <= 2 and bool(kept[0, V // 2 + 2:].all()) and not bool(kept[0, :V // 2 - 2].any())


@pytest.mark.parametrize("temperature,top_k,top_p", [(0.7, 50, 0.9), (1.3, 64, 0.95), (0.2, 50, None)])
def test_agrees_with_the_top_k_64_sampler(temperature, top_k, top_p):
    ops = _ops()
    B, V = 3, 128258
    lg = _logits(B, V, seed=21)
    sp = ops.SamplingParams(DEV, B, keep_kept_sets=True).set(temperature, top_k, top_p, seed=1)
    ops.sample(lg, sp)
    ref = sp.kept.cpu()
    _, kept = ops.sample_full(lg, ops.SamplingParams(DEV, B).set(temperature, top_k, top_p, seed=1), kept_mask=True)
    for b in range(B):
        n = int(ref[b, 0])
        assert sorted(ref[b, 1:1 + n].tolist()) == torch.nonzero(kept[b].cpu()).flatten().tolist(), b


@pytest.mark.parametrize("top_k,top_p", [(0, 0.9), (500, None)])
def test_draws_follow_the_kept_softmax(top_k, top_p):
    from spatialrgpt_amd.generation import warp_logits
    ops = _ops()
    V, B, CALLS, T = 128256, 512, 100, 1.0
    row = _logits(1, V, seed=3, scale=4.0)
    lg = row.expand(B, V).contiguous()
    sp = ops.SamplingParams(DEV, B).set(T, top_k, top_p, seed=4321)
    draws = torch.stack([ops.sample_full(lg, sp) for _ in range(CALLS)]).flatten().cpu()
    probs = warp_logits(row.cpu(), T, top_k, top_p).softmax(-1)[0].double()
    keep = torch.nonzero(probs > 0).flatten()
    N = draws.numel()
    counts = torch.bincount(draws, minlength=V).double()
    assert float(counts[probs == 0].sum()) == 0, "a filtered token was drawn"
    exp = probs[keep] * N
    big = exp >= 5  # pool the tail cells
    obs = torch.cat([counts[keep][big], counts[keep][~big].sum()[None]])
    ex = torch.cat([exp[big], exp[~big].sum()[None]])
    if float(ex[-1]) == 0:
        obs, ex = obs[:-1], ex[:-1]
    assert len(ex) >= 10, len(ex)
    chi2 = float(((obs - ex) ** 2 / ex).sum())
    assert chi2 < _chi2_crit(len(ex) - 1), (chi2, len(ex) - 1, _chi2_crit(len(ex) - 1))


def test_draws_are_a_function_of_seed_and_counter():
    ops = _ops()
    lg = _logits(4, 128258, seed=8, scale=1.0)
    for k, p in ((0, 0.9), (200, None)):
        a = ops.SamplingParams(DEV, 4).set(1.0, k, p, seed=7)
        b = ops.SamplingParams(DEV, 4).set(1.0, k, p, seed=7)
        c = ops.SamplingParams(DEV, 4).set(1.0, k, p, seed=8)
        s1 = [ops.sample_full(lg, a) for _ in range(6)]
        s2 = [ops.sample_full(lg, b) for _ in range(6)]
        s3 = [ops.sample_full(lg, c) for _ in range(6)]
        assert all(torch.equal(x, y) for x, y in zip(s1, s2))          # same seed, same counters
        assert not all(torch.equal(x, y) for x, y in zip(s1, s3))      # another seed
        assert not all(torch.equal(s1[0], x) for x in s1[1:])          # the counter advances
        b.set(1.0, k, p, seed=7, counter=3)
        assert torch.equal(ops.sample_full(lg, b), s1[3])              # a draw is addressed by (seed, counter)


# ------------------------------------------------------------------------------------------------ decode step and model.generate
@pytest.fixture(scope="module")
def peaked():
    return _peaked_model()


@pytest.fixture(scope="module")
def plain():
    """random (not peaked) weights: the draws at T = 1.5 really vary"""
    from spatialrgpt_amd.config import SrgptConfig
    from spatialrgpt_amd.model import LlavaLlamaModel
    from spatialrgpt_amd.weights import synth_state_dict

    cfg = SrgptConfig(vit_hidden=64, vit_inter=176, vit_layers=3, vit_heads=4, image_size=378, patch_size=14, hidden=1024, inter=2816,
                      layers=2, heads=8, kv_heads=2, vocab=32002, mask_token_id=32000, depth_token_id=32001,
                      max_position_embeddings=1024)
    sd = synth_state_dict(cfg, seed=1, dtype=torch.bfloat16, device=DEV)
    return cfg, LlavaLlamaModel(cfg, sd, device=DEV, dtype=torch.bfloat16, consume_state_dict=True)


@pytest.mark.parametrize("batch", [1, 4])
def test_graph_replay_equals_eager_steps(plain, batch):
    cfg, model = plain
    req = _request(cfg, batch=batch)
    eng = model.engine
    kw = dict(do_sample=True, temperature=1.5, top_k=0, top_p=0.9, max_new_tokens=24, eos_token_id=None)
    use = eng.use_graph
    try:
        eng.use_graph = False
        torch.manual_seed(5)
        eager = model.generate(**req, **kw)
        eng.use_graph = True
        torch.manual_seed(5)
        graph = model.generate(**req, **kw)  # greedy_decode checks srgpt_llm_decode_sync_state after the loop
    finally:
        eng.use_graph = use
    st = eng._state
    assert "sample_full" in st.graphs and st.c.sampling is None
    assert torch.equal(eager, graph)
    torch.manual_seed(6)
    assert not torch.equal(model.generate(**req, **kw), graph)  # another seed draws other ids


def test_generate_runs_every_setting_on_the_device(peaked, plain, monkeypatch):
    from spatialrgpt_amd.model import LlavaLlamaModel

    def no_torch_loop(*a, **k):
        raise AssertionError("the torch sampling loop ran")

    monkeypatch.setattr(LlavaLlamaModel, "_sample_loop", no_torch_loop)
    cfg, model = plain
    req = _request(cfg, batch=2)
    for kw in (dict(top_k=0, top_p=0.9), dict(top_k=200), dict(top_k=None, top_p=0.9)):
        torch.manual_seed(0)
        a = model.generate(**req, do_sample=True, temperature=1.5, max_new_tokens=16, eos_token_id=None, **kw)
        torch.manual_seed(0)
        b = model.generate(**req, do_sample=True, temperature=1.5, max_new_tokens=16, eos_token_id=None, **kw)
        assert a.shape == (2, 16) and torch.equal(a, b), kw
    # at T = 0.2 on peaked weights every other token has probability ~e^-50: the draws are the greedy ids
    cfg, model = peaked
    req = _request(cfg, batch=2)
    G = 32
    greedy = model.generate(**req, do_sample=False, max_new_tokens=G, eos_token_id=None)
    for kw in (dict(top_k=0, top_p=0.9), dict(top_k=200)):
        torch.manual_seed(1)
        assert torch.equal(model.generate(**req, do_sample=True, temperature=0.2, max_new_tokens=G, eos_token_id=None, **kw), greedy)
    # EOS: a row that draws an EOS id is padded after it, exactly as on the greedy path
    eos = int(greedy[0, 5])
    want = model.generate(**req, do_sample=False, max_new_tokens=G, eos_token_id=eos, pad_token_id=7)
    got = model.generate(**req, do_sample=True, temperature=0.2, top_k=200, max_new_tokens=G, eos_token_id=eos, pad_token_id=7)
    assert torch.equal(got, want)


def test_stopping_criteria_run_ahead_returns_the_serial_loops_prefix(peaked):
    cfg, model = peaked
    req = _request(cfg)
    G = 32
    kw = dict(do_sample=True, temperature=0.2, top_k=0, top_p=0.9)
    torch.manual_seed(0)
    full = model.generate(**req, **kw, max_new_tokens=G, eos_token_id=None)
    for stop_at in (0, 7, G - 1):
        target = int(full[0, stop_at])

        def crit(ids, scores, target=target):
            return bool((ids[0] == target).any())

        torch.manual_seed(0)
        out = model.generate(**req, **kw, max_new_tokens=G, eos_token_id=None, stopping_criteria=[crit])
        first = int(torch.nonzero(full[0] == target).flatten()[0])
        assert torch.equal(out, full[:, :first + 1]), (stop_at, out.shape)
