"""What the wide weight pass (decode_pass_rows = 32) gains over two passes of 16 rows.  -> profiles/wide_decode.txt

    python scripts/time_wide_decode.py [--out profiles/wide_decode.txt] [--only products|steps] [--formats bf16,fp8,mxfp4]

VILA1.5-8B geometry (bench.make_cfg, synth_state_dict seed 0), one process, one card.  Every timed call is: device synchronise, an
event, the work, an event, synchronise; the two lines of a comparison alternate block by block (one untimed call in front of every
block); three repetitions, the median of each is printed with the min .. max of all calls -- the spread a difference has to clear.

  products  q/k/v, o_proj, gate/up, down_proj and lm_head alone at 17, 24 and 32 rows, per format as the step launches them (bf16
            row-major; fp8 packed copies, lm_head row-major; MXFP4 packed copies): the `wide=True` entry against the 16-row entry (two
            passes) on the same rows, a captured graph of one launch per layer (32 different matrices: nothing is served from a cache;
            lm_head: 4 launches of the one matrix, 0.5 - 1 GB), us per launch
  steps     the captured decode step over 259 cached rows at 20, 24 and 32 sequences, an engine with the option on against one with it
            off, ms per step and tokens/s per GPU
The resource table of the wide instances comes from scripts/kernel_resources.py."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = []


def say(s=""):
    print(s, flush=True)
    OUT.append(s)


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def interleaved(lines, args):
    """lines: name -> fn.  -> name -> [reps][calls] ms"""
    for fn in lines.values():
        for _ in range(3):
            timed(fn)
    reps = {k: [[] for _ in range(args.reps)] for k in lines}
    for r in range(args.reps):
        for _ in range(args.blocks):
            for k, fn in lines.items():
                timed(fn)
                reps[k][r] += [timed(fn) for _ in range(args.per_block)]
    return reps


def line(reps, unit):
    return "  ".join("%8.2f" % (statistics.median(r) * unit) for r in reps) + "   %8.2f .. %8.2f" % (
        min(min(r) for r in reps) * unit, max(max(r) for r in reps) * unit)


def mid(reps):
    return statistics.median([statistics.median(r) for r in reps])


def captured(fn, stream):
    """fn's launches as a graph on `stream` -> a callable that replays it"""
    with torch.cuda.stream(stream):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            fn()
    return g.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_decode.txt"))
    ap.add_argument("--only", default="all", choices=["all", "products", "steps"])
    ap.add_argument("--formats", default="bf16,fp8,mxfp4")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--per-block", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=259)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the MI355X"
    import bench
    from spatialrgpt_amd import _lib as L, ops
    from spatialrgpt_amd.engine import SrgptEngine
    from spatialrgpt_amd.weights import synth_state_dict

    dev, dt = torch.device("cuda:0"), torch.bfloat16
    cfg = bench.make_cfg("vila15_8b")
    lib = L.load()
    kws = {"bf16": {}, "fp8": dict(llm_weight_format="fp8"), "mxfp4": dict(llm_weight_format="mxfp4", mxfp4_packed=True)}
    say("scripts/time_wide_decode.py --only %s: VILA1.5-8B geometry (hidden %d, inter %d, %d layers, heads %d / %d, vocab %d), synthetic "
        "weights, %s, %d CUs" % (args.only, cfg.hidden, cfg.inter, cfg.layers, cfg.heads, cfg.kv_heads, cfg.vocab,
                                 torch.cuda.get_device_name(0), lib.srgpt_device_cus()))
    say()
    g = torch.Generator(device=dev).manual_seed(3)
    stream = torch.cuda.Stream(device=dev)
    Hd, I, QW = cfg.hidden, cfg.inter, (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim
    for fmt in args.formats.split(","):
        engs = {}
        for pr in ((16, 32) if args.only in ("all", "steps") else (32,)):
            sd = synth_state_dict(cfg, seed=0, dtype=dt, device=dev)
            engs[pr] = SrgptEngine(cfg, sd, device=dev, dtype=dt, rope_positions=1024, consume_state_dict=True, decode_pass_rows=pr, **kws[fmt])
            del sd
        w = engs[32].w
        if args.only in ("all", "products"):
            say("%s products: events us per launch, median of each of %d repetitions    min .. max of all calls" % (fmt, args.reps))

            def mats(name):
                if fmt == "mxfp4":
                    return [dict(packed=w.p4[name][i][1], n_rows=w.llm_q4[name][0][i].shape[0]) for i in range(cfg.layers)]
                if fmt == "fp8":
                    return [dict(w8=w.llm_pk[name][i], wscale=w.llm_q[name][1][i], packed_rows=w.pk_rows[name],
                                 n_rows=w.llm_q[name][0][i].shape[0]) for i in range(cfg.layers)]
                return [dict(w=w.llm_t[name][i]) for i in range(cfg.layers)]

            head = [dict(w=w.lm_head) if fmt == "bf16" else dict(w8=w.lm_head8, wscale=w.lm_head_scale)] * 4
            # product -> (matrices, N, K, fusion): the step's fusions (norm with the table of the product before, residual in place + table)
            products = {"q/k/v": (mats("wqkv"), QW, Hd, "norm"), "o_proj": (mats("wo"), Hd, cfg.heads * cfg.head_dim, "res"),
                        "gate/up": (mats("wgu"), I, Hd, "swiglu"), "down_proj": (mats("wdown"), Hd, I, "res"), "lm_head": (head, cfg.vocab, Hd, "f32")}
            for pname, (ms, N, K, fusion) in products.items():
                for R in (17, 24, 32):
                    x = (torch.randn((R, K), device=dev, generator=g) * 0.5).to(dt)
                    gains = torch.ones((K,), device=dev, dtype=dt)
                    tab_in = torch.rand((R, L.ROWSS_STRIDE), device=dev, generator=g) * (K / 512.0)
                    h = (torch.randn((R, N), device=dev, generator=g) * 0.5).to(dt)
                    tab = torch.empty((R, L.ROWSS_STRIDE), device=dev, dtype=torch.float32)
                    out = torch.empty((R, N), device=dev, dtype=torch.float32 if fusion == "f32" else dt)
                    w4 = fmt == "mxfp4" and pname != "lm_head"
                    is_fp8 = fmt != "bf16" and not w4
                    pk = ms[0].get("packed_rows", 16 if w4 else 0)
                    chunk = ops.gemv_wide_pass_rows(R, N, K, fp8=is_fp8, packed_rows=pk, w4=w4, norm=fusion != "res", swiglu=fusion == "swiglu")

                    def run(wide):
                        for m in ms:
                            kw = dict(wide=wide)
                            if fusion == "res":
                                kw.update(residual=h, out=h, publish=True, table=tab)
                            else:
                                kw.update(norm_w=gains, eps=1e-5, rowss_in=tab_in, out=out, swiglu=fusion == "swiglu", out_f32=fusion == "f32")
                            if w4:
                                ops.gemv_w4p(x, m["packed"], m["n_rows"], **kw)
                            else:
                                ops.gemv_rowss(x, **m, **kw)

                    lines = {"two passes": captured(lambda: run(False), stream), "wide": captured(lambda: run(True), stream)}
                    reps = interleaved(lines, args)
                    u = 1e3 / len(ms)
                    say("  %-9s %2d rows  two passes %s   |  wide %s   |  wide / two passes %.3f  (route: %d rows per pass)" % (
                        pname, R, line(reps["two passes"], u), line(reps["wide"], u), mid(reps["wide"]) / mid(reps["two passes"]), chunk))
            say()
        if args.only in ("all", "steps"):
            say("%s steps over %d cached rows: captured step, events ms per step, median of each of %d repetitions    min .. max of all calls" % (
                fmt, args.rows, args.reps))
            G = 64
            for B in (20, 24, 32):
                x = (torch.randn((B, args.rows, Hd), device=dev, generator=g) * 0.5).to(dt)
                lines = {}
                for pr, e in engs.items():
                    def fn(e=e):
                        e._state = None
                        st = e.prefill(x, max_new=G + 2)[0]
                        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        t0.record(e.stream)
                        e.greedy_decode(st, G)
                        t1.record(e.stream)
                        torch.cuda.synchronize()
                        return t0.elapsed_time(t1) / G

                    lines[pr] = fn
                for fn in lines.values():
                    fn()
                reps = {pr: [[] for _ in range(args.reps)] for pr in lines}
                for r in range(args.reps):
                    for _ in range(args.blocks):
                        for pr, fn in lines.items():
                            fn()
                            reps[pr][r] += [fn() for _ in range(2)]
                say("  batch %2d  option off %s = %6.0f tok/s   |  option on %s = %6.0f tok/s   |  on / off %.3f" % (
                    B, line(reps[16], 1.0), B / mid(reps[16]) * 1e3, line(reps[32], 1.0), B / mid(reps[32]) * 1e3, mid(reps[32]) / mid(reps[16])))
            say()
        for e in engs.values():
            if fmt == "mxfp4":
                e.w.mxfp4_unbind()
        del engs, w
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
