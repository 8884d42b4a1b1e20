"""generate() tok/s of the sampling settings at BASELINE configs[1] geometry (VILA1.5-8B, bf16, bs 1, 8 regions, 128 new tokens),
each with and without a stopping criterion: the full device sampler against the torch-ops loop it replaced (`_sample_loop`, forced
by routing the setting away from the device), and the top-k-64 sampler's (0.7, 50) as the yardstick.

  python scripts/sampling_full_timing.py             # tok/s table (best of --reps whole requests)
  python scripts/sampling_full_timing.py --trace     # decode only, full sampler at B = 1 and B = 8 (run under rocprofv3 --kernel-trace)
  python scripts/sampling_full_timing.py --batch 1 4 --device-only   # the device samplers alone (no torch loop, no criterion), plus
                                                     # the top-k-64 sampler's Gumbel path (0.7, 0): every rep's tok/s, for a spread
SRGPT_LIB=<path of a libsrgpt_hip*.so build> selects the library, as for ubench_decode_step.py.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from spatialrgpt_amd import _lib as L  # noqa: E402

if os.environ.get("SRGPT_LIB"):
    L.LIB_PATH = os.path.abspath(os.environ["SRGPT_LIB"])
from spatialrgpt_amd import ops  # noqa: E402
from spatialrgpt_amd.model import LlavaLlamaModel  # noqa: E402
from spatialrgpt_amd.weights import synth_state_dict  # noqa: E402

SETTINGS = [(0.7, 50, None), (0.7, 0, 0.9), (0.7, 1000, None)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-new-tokens", type=int, default=128)
    ap.add_argument("--batch", type=int, nargs="+", default=[1])
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    cfg = bench.make_cfg("vila15_8b")
    G, dev, dt = args.max_new_tokens, torch.device("cuda"), torch.bfloat16
    sd = synth_state_dict(cfg, seed=0, dtype=dt, device=dev)
    model = LlavaLlamaModel(cfg, sd, device=dev, dtype=dt, rope_positions=1024, consume_state_dict=True)
    del sd
    if args.trace:
        eng = model.engine
        for B in (1, 8):
            x = torch.randn((B, 259, cfg.hidden), device=dev).to(dt)
            for T, k, p in SETTINGS[1:]:
                st, _, _ = eng.prefill(x, max_new=G)
                eng.greedy_decode(st, G, sampling=dict(temperature=T, top_k=k, top_p=p, seed=1, sampler=L.SAMPLER_FULL))
            torch.cuda.synchronize()
            print(f"traced: B = {B}, {len(SETTINGS) - 1} settings x {G} steps, full sampler", flush=True)
        return
    for batch in args.batch:
        timed(args, cfg, model, batch, G, dev, dt)


def timed(args, cfg, model, batch, G, dev, dt):
    ids, images, depths, masks = bench.synth_request(cfg, 8, 64, batch, dev, dt)
    req = dict(input_ids=ids, images=images, depths=depths, masks=masks, max_new_tokens=G, eos_token_id=None, do_sample=True)
    never = [lambda ids_, scores: False]
    orig = ops.SamplingParams.sampler

    def run(T, k, p, crit, torch_loop):
        ops.SamplingParams.sampler = staticmethod(
            lambda *a: (None if orig(*a) == L.SAMPLER_FULL else orig(*a)) if torch_loop else orig(*a))
        try:
            times = []
            for _ in range(args.reps + 1):  # + 1 warm-up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = model.generate(**req, temperature=T, top_k=k, top_p=p, stopping_criteria=crit)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            assert out.shape[1] == G
            if args.device_only:
                print(f"  B={batch} T={T} top_k={k} top_p={p} tok/s per rep after the warm-up: " + " ".join(f"{batch * G / t:.1f}" for t in times[1:]))
            return batch * G / min(times)
        finally:
            ops.SamplingParams.sampler = staticmethod(orig)

    base = None
    print(f"{os.path.basename(L.LIB_PATH)}: configs[1] geometry (vila15_8b, bf16, bs {batch}, 8 regions, prompt 64, {G} new tokens), whole request, best of {args.reps}")
    for T, k, p in SETTINGS + ([(0.7, 0, None)] if args.device_only else []):
        for crit in (None,) if args.device_only else (None, never):
            legs = [("device", False)] + ([("torch loop (before)", True)] if (k == 0 or k > 64) and not args.device_only else [])
            for name, tl in legs:
                r = run(T, k, p, crit, tl)
                if base is None:
                    base = r
                print(f"T={T} top_k={k} top_p={p} {'+ stopping criterion' if crit else '                    '} {name:20s} "
                      f"{r:7.1f} tok/s  {r / base:.3f} x (0.7, 50, no criterion)", flush=True)


if __name__ == "__main__":
    main()
