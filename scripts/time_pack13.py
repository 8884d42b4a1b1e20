#!/usr/bin/env python
"""The batch-1 bf16 decode products, raw bf16 weights (srgpt_gemv) against their lossless 13-bit packed copies (srgpt_gemv_p13).

    python scripts/time_pack13.py [--out profiles/pack13_products.txt] [--config vila15_8b] [--layers 32]

q/k/v, gate/up and down_proj: one launch per layer (--layers distinct matrices, so that no replay finds a weight in a cache) in a
captured graph; lm_head: --heads distinct matrices.  Both kernels in the same process, alternating (raw, packed, raw, ...), events
on the stream the graphs run on: per product the median and min .. max of all replays in us per launch, the rate in weights / s and
bytes / s.  Before it is timed every packed product is compared with the raw one bit for bit.  The matrices come from the device
generator, which returns an exact 0.0 about once in 1e7 draws, so about one row in a thousand is an exception row and runs the raw
loop inside the packed launch, as in a model from synth_state_dict; their count is printed with every product, and more than 2e-3
of the rows stops the script (a packed kernel mostly on its raw fallback would time the wrong loop).  A product keeps its packed route only where its
packed median is below the raw kernel's minimum of the same visit."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = []


def say(s=""):
    print(s, flush=True)
    OUT.append(s)


def timed(replay, stream):
    with torch.cuda.stream(stream):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        replay()
        b.record()
        torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--config", default="vila15_8b")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--heads", type=int, default=3, help="distinct lm_head matrices in its chain")
    ap.add_argument("--calls", type=int, default=40, help="timed replays per kernel")
    ap.add_argument("--only", default="", help="comma-separated product names: qkv, gu, down, lm_head")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from spatialrgpt_amd import _lib as L
    if os.environ.get("SRGPT_LIB"):  # another build of the library (a compile-time variant of the batch sizes), as ubench_decode_step.py
        L.LIB_PATH = os.path.abspath(os.environ["SRGPT_LIB"])
    from spatialrgpt_amd import ops
    from spatialrgpt_amd.config import SrgptConfig

    cfg = getattr(SrgptConfig, args.config)()
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    Hd, I, QW = cfg.hidden, cfg.inter, (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim
    # name -> (title, matrix rows, N, K, norm, residual, swiglu, fp32 out, matrices in the chain)
    products = {"qkv": ("q/k/v   [%d, %d] norm" % (QW, Hd), QW, QW, Hd, True, False, False, False, args.layers),
                "gu": ("gate/up [2 x %d, %d] norm, SwiGLU" % (I, Hd), 2 * I, I, Hd, True, False, True, False, args.layers),
                "down": ("down    [%d, %d] residual" % (Hd, I), Hd, Hd, I, False, True, False, False, args.layers),
                "lm_head": ("lm_head [%d, %d] norm, fp32" % (cfg.vocab, Hd), cfg.vocab, cfg.vocab, Hd, True, False, False, True, args.heads)}
    only = [s for s in args.only.split(",") if s]
    stream = torch.cuda.Stream()
    say("batch-1 bf16 decode products, raw (srgpt_gemv) against 13-bit packed (srgpt_gemv_p13): %s, %d CUs, us per launch" % (
        args.config, L.load().srgpt_device_cus()))
    say("  %-38s %-28s %-28s %s" % ("product", "raw median (min .. max)", "packed median (min .. max)", "packed median / raw min   keep?"))
    with torch.cuda.stream(stream):
        for name, (title, rows, N, K, norm, res, sw, f32, n) in products.items():
            if only and name not in only:
                continue
            if not ops.pack13_eligible(torch.empty((1, K), dtype=dt)):
                say("  %-38s K = %d is not a multiple of 512: stays raw" % (title, K))
                continue
            ws = [(torch.randn((rows, K), device=dev, generator=g) * 0.02).to(dt) for _ in range(n)]
            pk, exc = [], 0
            for w in ws:
                packed, flags, n_exc = ops.pack13(w)
                exc += n_exc
                pk.append((packed, flags))
            # (the device generator returns an exact 0.0 about once in 1e7 draws: a few rows per matrix, as in synth_state_dict's)
            assert exc <= 2e-3 * rows * n, "%s: %d exception rows of %d in gaussian matrices" % (name, exc, rows * n)
            x = (torch.randn((1, K), device=dev, generator=g) * 0.5).to(dt)
            nw = (1.0 + 0.02 * torch.randn((K,), device=dev, generator=g)).to(dt) if norm else None
            r = (torch.randn((1, N), device=dev, generator=g) * 0.5).to(dt) if res else None
            out = torch.empty((1, N), device=dev, dtype=torch.float32 if f32 else dt)
            ref = ops.gemv(x, ws[0], nw, 1e-5, r, sw, out_f32=f32)
            got = ops.gemv_p13(x, pk[0][0], pk[0][1], ws[0], nw, 1e-5, r, sw, out_f32=f32)
            assert torch.equal(ref, got), "%s: the packed product differs from the raw one" % name

            def launches(kind):
                for w, (packed, flags) in zip(ws, pk):
                    if kind == "raw":
                        ops.gemv(x, w, nw, 1e-5, r, sw, out=out, out_f32=f32)
                    else:
                        ops.gemv_p13(x, packed, flags, w, nw, 1e-5, r, sw, out=out, out_f32=f32)

            graphs = {}
            for kind in ("raw", "packed"):
                launches(kind)
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=stream):
                    launches(kind)
                graphs[kind] = gr
            t = {"raw": [], "packed": []}
            for _ in range(5):
                for kind in t:
                    timed(graphs[kind].replay, stream)
            for _ in range(args.calls):
                for kind in t:
                    t[kind].append(timed(graphs[kind].replay, stream) * 1e3 / n)
            med = {k: statistics.median(v) for k, v in t.items()}
            keep = med["packed"] < min(t["raw"])
            say("  %-38s %7.2f (%7.2f .. %7.2f)    %7.2f (%7.2f .. %7.2f)    %.3f  %s" % (
                title, med["raw"], min(t["raw"]), max(t["raw"]), med["packed"], min(t["packed"]), max(t["packed"]),
                med["packed"] / min(t["raw"]), "packed" if keep else "raw"))
            say("  %-38s raw %.2f TB/s, %.2fe12 weights/s; packed %.2f TB/s, %.2fe12 weights/s; %d exception rows of %d" % (
                "", rows * K * 2 / med["raw"] * 1e-6, rows * K / med["raw"] * 1e-6,
                pk[0][0].numel() / med["packed"] * 1e-6, rows * K / med["packed"] * 1e-6, exc, rows * n))
            del graphs, ws, pk
            torch.cuda.empty_cache()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
            fh.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
