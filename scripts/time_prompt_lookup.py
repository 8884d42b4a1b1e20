"""What prompt-lookup decoding costs and gains.  -> profiles/prompt_lookup.txt, profiles/prompt_lookup_sampling.txt (--sampling),
profiles/prompt_lookup_batch.txt (--batch), profiles/prompt_lookup_batch_sampling.txt (--sampling with --batch)

    python scripts/time_prompt_lookup.py step     [--weights bf16|fp8] [--rows 259] [--tree DIR] [--sampling demo|full|demo,full]
                                                  [--batch 2,4,8] [--only-plain]
    python scripts/time_prompt_lookup.py requests [--new 128] [--sampling demo] [--batch 4]

step: VILA1.5-8B geometry (bench.make_cfg, synth_state_dict seed 0), batch 1, `rows` cached rows.  The captured plain decode step
against the captured lookup step at T = 2, 3, 4 rows: per call the state's position and step counter are put back outside the window,
then device synchronise, an event, ONE graph launch, an event, synchronise.  Per repetition 4 blocks of 10 calls per line, the lines
alternating block by block (one untimed call in front of every block); three repetitions, the median of each is printed.  --tree DIR
imports the package from another checkout (the parent commit: it has no lookup step, only the plain line is timed).

requests: the same geometry with PEAKED weights (tests.util.make_peaked: the greedy continuation walks a permutation), text-only
prompts, `new` tokens per request, K = 3: the full-acceptance prompt (the walk itself, then its first id) and the zero-acceptance
prompt (every id of the walk followed by an id the model does not pick), each with and without the keyword; wall clock from the call
to the synchronise behind it, 2 warm-up requests, 5 timed ones per line and repetition, three repetitions.

--sampling: the SAMPLED leg.  step: every line draws its tokens on the device -- the captured plain sampled step against the captured
sampled lookup step (srgpt_llm_lookup_step_ex) at T = 2, 3, 4, at the demo's settings (`demo`: temperature 0.2, top-k 50, the
top-k-64 sampler) or at a setting of the full sampler (`full`: temperature 0.7, top-p 0.9, no top-k); on a tree without the sampled
lookup step (the parent commit) only the plain sampled line is timed.  requests: do_sample at the demo's settings -- on the peaked
weights every draw is its row's argmax (the ids are asserted to be the walk), so the two prompts keep their acceptance rates -- with
the model's lookup_sampling switch off and on; the keyword is passed on both sides.

--batch B (step takes a list B1,B2,...): the BATCHED leg, greedy unless --sampling is given too (below).  step: B sequences of `rows` cached rows each -- the captured plain batched step against the
captured batched lookup step (srgpt_llm_lookup_step_batch) at every T of 2, 3, 4 with B * T <= 16; per call the rows' positions, the
step counter and the rows' emission counts are put back outside the window.  On a tree without the batched step (the parent commit)
only the plain line is timed: that is the baseline the ratios are taken against.  requests: B rows with the model's lookup_batch
switch on, every row on a walk of its own -- every row the full-acceptance prompt, every row the zero-acceptance prompt, and mixed
(row 0 zero acceptance among full-acceptance rows, which hold all their ids early and ride along frozen) --, each against the same
call without the keyword; both must return the walks.

--sampling with --batch: the SAMPLED BATCHED leg.  step (--sampling takes a list: one engine, a state per setting and batch size): the
captured plain sampled batched step against the captured sampled batched lookup step (srgpt_llm_lookup_step_batch_ex) at every (B, T)
and, in the same process and the same alternation, the captured GREEDY batched lookup step on the same state -- the difference of the
two lookup lines is what the sampler's B * T rows add.  --only-plain times the plain line alone (the switch-off comparison with the
parent commit: the same work in both trees).  requests: B rows at the demo's settings with the model's lookup_batch switch on and
lookup_batch_sampling off / on, the keyword passed on both sides; every row full acceptance and every row zero acceptance; both sides
must return the walks (on the peaked weights every draw is its row's argmax)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# the sampled leg's settings: the demo's (the top-k-64 sampler) and one only the full sampler serves
SAMPLING = {"demo": dict(temperature=0.2, top_k=50, top_p=1.0), "full": dict(temperature=0.7, top_k=0, top_p=0.9)}


def med3(reps):
    return "  ".join("%7.3f" % statistics.median(r) for r in reps) + "    %7.3f .. %7.3f" % (min(min(r) for r in reps), max(max(r) for r in reps))


def step_cost(args):
    import bench
    from spatialrgpt_amd import _lib as L, ops
    from spatialrgpt_amd.engine import SrgptEngine
    from spatialrgpt_amd.weights import synth_state_dict

    dev, dt = torch.device("cuda:0"), torch.bfloat16
    cfg = bench.make_cfg("vila15_8b")
    sd = synth_state_dict(cfg, seed=0, dtype=dt, device=dev)
    eng = SrgptEngine(cfg, sd, device=dev, dtype=dt, rope_positions=1024, consume_state_dict=True,
                      llm_weight_format="native" if args.weights == "bf16" else "fp8")
    del sd
    lib, w = L.load(), eng.w
    for name, B in ((name, B) for name in args.sampling.split(",") for B in args.batches):  # one engine, one state per setting and batch size
        sampling = SAMPLING.get(name)
        entry = ("srgpt_llm_lookup_step_batch_ex" if sampling else "srgpt_llm_lookup_step_batch") if B > 1 else \
            "srgpt_llm_lookup_step_ex" if sampling else "srgpt_llm_lookup_step"
        have_lookup = hasattr(lib, entry) and not args.only_plain
        g = torch.Generator(device=dev).manual_seed(3)
        x = (torch.randn((B, args.rows, cfg.hidden), device=dev, generator=g) * 0.5).to(dt)
        st, _, _ = eng.prefill(x, max_new=64)
        lines = ["plain"] + ([f"lookup T={t}" for t in (2, 3, 4) if B * t <= 16] if have_lookup else [])
        if have_lookup and sampling and B > 1:  # the greedy batched lookup step on the same state: what the sampler's rows add
            lines += [f"greedy T={t}" for t in (2, 3, 4) if B * t <= 16]
        reps = {k: [[] for _ in range(args.reps)] for k in lines}
        with torch.cuda.stream(eng.stream):
            eng.stream.wait_stream(torch.cuda.default_stream())
            if sampling:  # the block stays set: every graph below is captured, and replays, as a sampled step
                kind = ops.SamplingParams.sampler(sampling["temperature"], sampling["top_k"], sampling["top_p"], cfg.vocab)
                st.set_sampling(dict(sampling, seed=1, sampler=kind))
            L.check(lib.srgpt_llm_sample_first_ex(C.byref(w.llm), C.byref(st.c), st.sampler, ops._stream()))

            def graph_of(line):
                if line == "plain":
                    return st.ensure_graph()
                if B > 1:
                    st.ensure_lookup_batch(int(line.split("=")[1]) - 1, 2, None)
                    if line.startswith("greedy"):  # captured with the block taken off the state: a graph key of its own
                        block, st.c.sampling = st.c.sampling, None
                        try:
                            return st.ensure_lookup_batch_graph()
                        finally:
                            st.c.sampling = block
                    return st.ensure_lookup_batch_graph()
                st.ensure_lookup(int(line.split("=")[1]) - 1, 2, None)  # a change of T drops the captured graph: captured again per block
                return st.ensure_lookup_graph()

            def once(graph, timed=True):
                st.pos.fill_(args.rows)
                st.step.fill_(1)
                if B > 1 and getattr(st, "lookup_b", None) is not None:
                    st.lookup_b["steps"].fill_(1)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                L.check(lib.srgpt_graph_launch(graph, 1, ops._stream()))
                b.record()
                torch.cuda.synchronize()
                return a.elapsed_time(b)

            for line in lines:  # warm-up
                gr = graph_of(line)
                for _ in range(5):
                    once(gr)
            for r in range(args.reps):
                for _ in range(args.blocks):
                    for line in lines:
                        gr = graph_of(line)
                        once(gr)
                        reps[line][r] += [once(gr) for _ in range(args.per_block)]
        rc = lib.srgpt_llm_decode_sync_state(C.byref(w.llm), C.byref(st.c), ops._stream())
        assert rc == 0, L.last_error()
        print(f"step cost, batch {B}, {args.weights}, sampling {name} {sampling}, {args.rows} cached rows, tree {args.tree}: events ms, median of {args.blocks * args.per_block} "
              f"({args.reps} repetitions)   min .. max of all")
        base = statistics.median([statistics.median(r) for r in reps["plain"]])
        for line in lines:
            m = statistics.median([statistics.median(r) for r in reps[line]])
            print("  %-12s %s    ratio to plain %.3f" % (line, med3(reps[line]), m / base))
        for line in (ln for ln in lines if ln.startswith("greedy")):  # sampled minus greedy lookup step at the same (B, T)
            t = line.split("=")[1]
            d = [statistics.median(a) - statistics.median(b) for a, b in zip(reps[f"lookup T={t}"], reps[line])]
            print("  sampler's rows at T=%s: %+.3f ms (median of the repetitions' differences; %+.3f .. %+.3f)" % (t, statistics.median(d), min(d), max(d)))


def requests_batch(args):
    import bench
    from spatialrgpt_amd.model import LlavaLlamaModel
    from spatialrgpt_amd.weights import synth_state_dict
    from tests.util import make_peaked

    dev, dt = torch.device("cuda:0"), torch.bfloat16
    cfg = bench.make_cfg("vila15_8b")
    sd = synth_state_dict(cfg, seed=0, dtype=dt, device=dev)
    perm = make_peaked(sd, cfg)
    model = LlavaLlamaModel(cfg, sd, device=dev, dtype=dt, rope_positions=1024, consume_state_dict=True, lookup_batch=True)
    del sd
    n, K, B = args.new, 3, args.batch
    sampling = SAMPLING.get(args.sampling)
    chains = []
    for a in range(17, 17 + 12 * B, 12):  # one walk per row
        chain = [a]
        for _ in range(n):
            chain.append(int(perm[chain[-1]]))
        assert len(set(chain)) == len(chain)
        chains.append(chain)
    used = {t for c in chains for t in c}
    z = next(t for t in range(100, cfg.vocab) if t not in used and all(int(perm[c]) != t for c in used))
    full = [c + [c[0]] for c in chains]
    zero = [[t for h in c for t in (h, z)] + [c[0]] for c in chains]
    cases = {"every row full acceptance": full, "every row zero acceptance": zero, "mixed: row 0 zero, the others full acceptance": zero[:1] + full[1:]}
    print(f"whole requests, batch {B}, bf16, peaked weights, {'sampling ' + args.sampling + ' ' + str(sampling) if sampling else 'greedy'}, {n} new tokens per row, K = {K}: tokens/s over the batch, "
          f"median of {args.per_rep} ({args.reps} repetitions)")
    for name, rows in cases.items():
        P = max(len(r) for r in rows)
        ids = torch.tensor([r + [0] * (P - len(r)) for r in rows], dtype=torch.int64, device=dev)
        mask = torch.tensor([[1] * len(r) + [0] * (P - len(r)) for r in rows], dtype=torch.int64, device=dev)
        kw = dict(attention_mask=mask, do_sample=False, max_new_tokens=n, eos_token_id=None)
        if sampling:  # the keyword on both sides: the lookup_batch_sampling switch decides
            kw = dict(attention_mask=mask, do_sample=True, max_new_tokens=n, eos_token_id=None, prompt_lookup_num_tokens=K, **sampling)
        outs, reps, stats = {}, {}, None
        for side, extra in (("plain", {}), ("lookup", {} if sampling else dict(prompt_lookup_num_tokens=K))):
            model.lookup_batch_sampling = bool(sampling) and side == "lookup"
            reps[side] = [[] for _ in range(args.reps)]
            for r in range(-1, args.reps):
                for i in range(2 if r < 0 else args.per_rep):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = model.generate(ids, **kw, **extra)
                    torch.cuda.synchronize()
                    if r >= 0:
                        reps[side][r].append(B * n / (time.perf_counter() - t0))
            outs[side] = out
            assert model.last_lookup["mode"] == side, model.last_lookup
            if side == "lookup":
                stats = dict(model.last_lookup)
        assert torch.equal(outs["plain"], outs["lookup"]) and outs["plain"].tolist() == [c[1:] for c in chains], name
        print(f"  {name}: prompts of {[len(r) for r in rows]} ids, {stats}")
        for side in ("plain", "lookup"):
            print("    %-7s %s" % (side, med3(reps[side])))


def requests(args):
    import bench
    from spatialrgpt_amd.model import LlavaLlamaModel
    from spatialrgpt_amd.weights import synth_state_dict
    from tests.util import make_peaked

    dev, dt = torch.device("cuda:0"), torch.bfloat16
    cfg = bench.make_cfg("vila15_8b")
    sd = synth_state_dict(cfg, seed=0, dtype=dt, device=dev)
    perm = make_peaked(sd, cfg)
    model = LlavaLlamaModel(cfg, sd, device=dev, dtype=dt, rope_positions=1024, consume_state_dict=True)
    del sd
    n, K = args.new, 3
    sampling = SAMPLING.get(args.sampling)
    chain = [17]
    for _ in range(n):
        chain.append(int(perm[chain[-1]]))
    assert len(set(chain)) == len(chain)
    z = next(t for t in range(100, cfg.vocab) if t not in chain and all(int(perm[c]) != t for c in chain))
    prompts = {"full acceptance": chain + [chain[0]], "zero acceptance": [t for c in chain for t in (c, z)] + [chain[0]]}
    print(f"whole requests, bf16, peaked weights, sampling {args.sampling} {sampling}, {n} new tokens, K = {K}: tokens/s, median of {args.per_rep} ({args.reps} repetitions)")
    for name, prompt in prompts.items():
        ids = torch.tensor([prompt], dtype=torch.int64, device=dev)
        kw = dict(do_sample=False, max_new_tokens=n, eos_token_id=None)
        if sampling:  # the keyword on both sides: the switch decides
            kw = dict(do_sample=True, max_new_tokens=n, eos_token_id=None, prompt_lookup_num_tokens=K, **sampling)
        outs, reps, stats = {}, {}, None
        for side, extra in (("plain", {}), ("lookup", {} if sampling else dict(prompt_lookup_num_tokens=K))):
            model.lookup_sampling = bool(sampling) and side == "lookup"
            reps[side] = [[] for _ in range(args.reps)]
            for r in range(-1, args.reps):
                for i in range(2 if r < 0 else args.per_rep):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = model.generate(ids, **kw, **extra)
                    torch.cuda.synchronize()
                    if r >= 0:
                        reps[side][r].append(n / (time.perf_counter() - t0))
            outs[side] = out
            assert model.last_lookup["mode"] == side, model.last_lookup
            if side == "lookup":
                stats = dict(model.last_lookup)
        assert torch.equal(outs["plain"], outs["lookup"]) and outs["plain"][0].tolist() == chain[1:], name
        print(f"  {name}: prompt of {len(prompt)} ids, {stats}")
        for side in ("plain", "lookup"):
            print("    %-7s %s" % (side, med3(reps[side])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["step", "requests"])
    ap.add_argument("--weights", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--rows", type=int, default=259)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--per-block", type=int, default=10)
    ap.add_argument("--per-rep", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sampling", default="off", help="time the sampled steps / requests: off, demo or full; step takes a list: demo,full")
    ap.add_argument("--batch", default="1", help="sequences per step / request (> 1: the batched lookup step); step takes a list: 2,4,8")
    ap.add_argument("--only-plain", action="store_true", help="step: time the plain line alone")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is timed")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    assert torch.cuda.is_available(), "a timing needs the MI355X"
    args.batches = [int(b) for b in args.batch.split(",")]
    args.batch = args.batches[0]
    assert all(name == "off" or name in SAMPLING for name in args.sampling.split(",")), "--sampling: off, demo or full"
    assert args.what == "step" or "," not in args.sampling, "requests take one setting"
    step_cost(args) if args.what == "step" else requests_batch(args) if args.batch > 1 else requests(args)


if __name__ == "__main__":
    main()
