"""What prompt-lookup decoding costs and gains.  -> profiles/prompt_lookup.txt, profiles/prompt_lookup_sampling.txt (--sampling)

    python scripts/time_prompt_lookup.py step     [--weights bf16|fp8] [--rows 259] [--tree DIR] [--sampling demo|full]
    python scripts/time_prompt_lookup.py requests [--new 128] [--sampling demo]

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
the model's lookup_sampling switch off and on; the keyword is passed on both sides."""
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
    sampling = SAMPLING.get(args.sampling)
    have_lookup = hasattr(lib, "srgpt_llm_lookup_step_ex" if sampling else "srgpt_llm_lookup_step")
    g = torch.Generator(device=dev).manual_seed(3)
    x = (torch.randn((1, args.rows, cfg.hidden), device=dev, generator=g) * 0.5).to(dt)
    st, _, _ = eng.prefill(x, max_new=64)
    lines = ["plain"] + ([f"lookup T={t}" for t in (2, 3, 4)] if have_lookup else [])
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
            st.ensure_lookup(int(line.split("=")[1]) - 1, 2, None)  # a change of T drops the captured graph: captured again per block
            return st.ensure_lookup_graph()

        def once(graph, timed=True):
            st.pos.fill_(args.rows)
            st.step.fill_(1)
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
    print(f"step cost, {args.weights}, sampling {args.sampling} {sampling}, {args.rows} cached rows, tree {args.tree}: events ms, median of {args.blocks * args.per_block} "
          f"({args.reps} repetitions)   min .. max of all")
    base = statistics.median([statistics.median(r) for r in reps["plain"]])
    for line in lines:
        m = statistics.median([statistics.median(r) for r in reps[line]])
        print("  %-12s %s    ratio to plain %.3f" % (line, med3(reps[line]), m / base))


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
    ap.add_argument("--sampling", default="off", choices=["off"] + sorted(SAMPLING), help="time the sampled steps / requests")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is timed")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    assert torch.cuda.is_available(), "a timing needs the MI355X"
    step_cost(args) if args.what == "step" else requests(args)


if __name__ == "__main__":
    main()
