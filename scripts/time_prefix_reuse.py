"""Time to the first token of a follow-up request with `prefix_reuse` off (the whole conversation runs again: two ViT passes,
refinement, pooling, projector, full prefill) and on (the last request's cache is continued; spatialrgpt_amd/reuse.py), and of a
FIRST request with the switch on against off (what retaining costs).  -> profiles/prefix_reuse.txt

    python scripts/time_prefix_reuse.py [--model vila15_8b] [--regions 8] [--prompt-len 64] [--turn 32] [--out FILE]

Geometry and data: bench.py's (make_cfg, synth_state_dict seed 0, synth_request seed 1), bf16, batch 1.  Turn 1 is the bench request
with max_new_tokens = 1: `spliced_len` cached rows and one pending id.  The follow-up re-sends turn 1's ids, its one generated id and
`turn - 1` new ids: a `turn`-row new turn over the cached rows.  Every timed call is generate(..., max_new_tokens=1) from the call to
the synchronise behind it -- the time to the first token, host work included.  One process, profiler off; warm-up, then per
repetition 4 blocks of 10 calls per side, the sides alternating block by block; three repetitions, the median of each is listed and
their spread is the run-to-run spread.  With the switch on, an untimed re-send of turn 1 in front of every timed follow-up puts the
retained state back to turn 1's rows (itself a reuse hit: 1 row appended)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    from spatialrgpt_amd.model import LlavaLlamaModel
    from spatialrgpt_amd.weights import synth_state_dict

    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="vila15_8b")
    ap.add_argument("--regions", type=int, default=8)
    ap.add_argument("--prompt-len", type=int, default=64)
    ap.add_argument("--turn", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--per-block", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the MI355X"
    device, dtype = torch.device("cuda:0"), torch.bfloat16
    cfg = bench.make_cfg(args.model)
    sd = synth_state_dict(cfg, seed=0, dtype=dtype, device=device)
    model = LlavaLlamaModel(cfg, sd, device=device, dtype=dtype, rope_positions=1024, consume_state_dict=True)
    del sd
    ids, images, depths, masks = bench.synth_request(cfg, args.regions, args.prompt_len, 1, device, dtype)
    media = dict(images=images, depths=depths, masks=masks)
    kw = dict(do_sample=False, max_new_tokens=1, eos_token_id=None)
    T = bench.spliced_len(cfg, args.prompt_len)

    model.prefix_reuse = False
    gen1 = model.generate(ids, **media, **kw)
    g = torch.Generator().manual_seed(7)
    hi = min(cfg.mask_token_id, cfg.depth_token_id, cfg.vocab)
    seg = torch.randint(3, hi, (1, args.turn - 1), generator=g).to(device)
    follow = torch.cat([ids, gen1, seg], 1)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def follow_off():
        model.prefix_reuse = False
        return timed(lambda: model.generate(follow, **media, **kw))

    def follow_on():
        model.prefix_reuse = True
        model.generate(ids, **media, **kw)  # untimed: the retained state back to turn 1 (T cached rows, one pending id)
        ms, out = timed(lambda: model.generate(follow, **media, **kw))
        assert model.last_reuse["mode"] == "append" and model.last_reuse["rows_reused"] == T, model.last_reuse
        assert model.last_reuse["rows_appended"] == args.turn and model.last_reuse["towers_skipped"]
        return ms, out

    def first_off():
        model.prefix_reuse = False
        return timed(lambda: model.generate(ids, **media, **kw))

    def first_on():
        model.prefix_reuse = True
        model.drop_reuse()  # untimed: no retained request, the call is a first request
        ms, out = timed(lambda: model.generate(ids, **media, **kw))
        assert model.last_reuse["mode"] == "fresh"
        return ms, out

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"model {args.model}, bf16, bs 1, {args.regions} regions, {args.prompt_len}-id prompt -> {T} spliced rows; follow-up: {T} cached rows "
        f"+ a {args.turn}-row new turn = {T + args.turn} rows; every call generate(max_new_tokens=1), host clock around call + synchronise")
    same = {}
    for name, off, on in (("follow-up", follow_off, follow_on), ("first request", first_off, first_on)):
        for _ in range(5):  # warm-up of both sides: code objects, the pooled and the retained state's geometry, allocator
            off()
            on()
        meds = {"off": [], "on": []}
        allv = {"off": [], "on": []}
        for rep in range(args.reps):
            v = {"off": [], "on": []}
            for b in range(args.blocks):
                for side, fn in (("off", off), ("on", on)):
                    for _ in range(args.per_block):
                        ms, out = fn()
                        v[side].append(ms)
                        same.setdefault(name, {})[side] = out
            for side in ("off", "on"):
                meds[side].append(statistics.median(v[side]))
                allv[side] += v[side]
        n = args.blocks * args.per_block
        for side in ("off", "on"):
            say(f"{name:14s} prefix_reuse {side:3s}: median of {n} ms, {args.reps} repetitions: "
                + "  ".join(f"{m:7.3f}" for m in meds[side]) + f"   spread of the medians {max(meds[side]) - min(meds[side]):.3f}"
                + f"   min .. max of all {min(allv[side]):.3f} .. {max(allv[side]):.3f}")
        d = [a - b for a, b in zip(meds["off"], meds["on"])]
        say(f"{name:14s} off - on per repetition: " + "  ".join(f"{x:+.3f}" for x in d) + " ms;  on / off = "
            + "  ".join(f"{b / a:.3f}" for a, b in zip(meds["off"], meds["on"])))
        say(f"{name:14s} first token on == off: {bool(torch.equal(same[name]['off'], same[name]['on']))}")
    model.prefix_reuse = True
    model.drop_reuse()
    model.generate(ids, **media, **kw)
    say(f"retained by one request: {model.reuse_record.nbytes() / 2 ** 20:.1f} MiB (media, tower features, splice table, KV cache of "
        f"{model.reuse_record.state.max_pos} positions, workspace, logits)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
