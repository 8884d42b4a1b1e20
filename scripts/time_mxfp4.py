"""What llm_weight_format="mxfp4" costs and gains against fp8 and bf16.  -> profiles/mxfp4.txt

    python scripts/time_mxfp4.py [--out profiles/mxfp4.txt] [--rows 259] [--only steps|products|packed|prefill|whole_m|w4a8] [--tree DIR]

VILA1.5-8B geometry (bench.make_cfg, synth_state_dict seed 0), one process, three engines (bf16, fp8, mxfp4) on one card.  Every
timed call is: the state put back outside the window, device synchronise, an event, the work, an event, synchronise.  The lines of a
section alternate block by block (one untimed call in front of every block); three repetitions, the median of each is printed with
the min .. max of all calls -- the run-to-run spread a ratio has to clear.

  steps     the captured batch-1 decode step over `rows` cached rows: bf16, fp8, mxfp4
  lookup    the captured lookup step at K = 3 (T = 4 rows): fp8, mxfp4
  batch 8   the captured batch-8 step: fp8 (the MFMA kernel, one pass of 8 rows) against mxfp4 (two passes of 4 rows)
  products  q/k/v, o_proj, gate/up and down_proj alone at 1 .. 4 rows, srgpt_gemv_w8 against srgpt_gemv_w4: a captured graph of one
            launch per layer (32 different matrices: nothing is served from a cache), us per launch
  prefill   the 259-row prefill and a 32-row append over it, eager calls: fp8 against mxfp4 (srgpt_gemm_w4 and its composites: the
            direct-to-LDS kernels multiply the codes, the whole-M and 256 x 256 routes expand the matrix to bf16 first)
  bytes     llm_weight_bytes() of the three engines

--only packed  (-> profiles/mxfp4_mfma.txt) the packed MXFP4 copies (mxfp4_packed=True: srgpt_gemv_w4p, the MFMA product) against the
default mxfp4 engine and fp8, three engines in one process:
  one row   the captured batch-1 step: the packed engine takes the default engine's launches
  steps     the captured lookup step at K = 1 / 2 / 3, the batch-4 and batch-8 step, the batched lookup step at (2, 4) and (4, 4)
  products  the four products at 1 .. 4, 8 and 16 rows: srgpt_gemv_w4 (VALU), srgpt_gemv_w4p, fp8 srgpt_gemv_rowss over its packed copy
  HBM       what the engines hold, and mxfp4_packed_bytes()

--only prefill  (-> profiles/mxfp4_prefill.txt) the prefill leg for all three formats: the captured batch-1 decode steps, then the
259-row prefill and the 32-row append over 259 cached rows, eager, bf16 / fp8 / mxfp4.  Run on this tree and, with --tree, on the
parent commit's checkout in alternating fresh processes: a change of the mxfp4 lines counts when it clears the min .. max of one
process's calls, and the bf16 / fp8 lines and the decode steps have to stay inside it.

--only whole_m  (-> profiles/mxfp4_whole_m.txt) --only prefill's lines with a fourth engine, "mxfp4 direct" (mxfp4_prefill_direct=True:
the whole-M kernel multiplies the codes of q/k/v, gate/up and down_proj itself), where the timed tree has the option; then those
three products alone at `rows` rows, one launch per layer (32 different matrices) in a captured graph, us per launch: the W4 instance
(direct=True), the expansion plus the bf16 launch (the plain entry) and the bf16 launch alone (the bf16 engine's matrix).  Same
protocol as --only prefill: this tree and, with --tree, the parent commit's checkout (three engines, no products section) in
alternating fresh processes of one job.

--only w4a8  (-> profiles/mxfp4_w4a8.txt) llm_weight_format="mxfp4_w4a8" (per-token e4m3 activations x the codes on the block-scaled
MFMA, srgpt_gemm_w4a8) next to bf16, "fp8_w8a8" and "mxfp4" with mxfp4_prefill_direct=True, four engines in one process (three where
the timed tree does not have the format): the captured batch-1 decode step; the prefill at 1 x, 4 x and 8 x `rows` rows; the 32-row
append over `rows` cached rows; then the four layer products alone at 8 x `rows` rows, one launch per layer (32 different matrices)
in a captured graph, us per launch: srgpt_gemm_w4a8, srgpt_gemm_w8a8 and the expansion + srgpt_gemm (srgpt_gemm_w4).  Same protocol
as --only whole_m; with --tree the parent commit's checkout gives the lines that must not move.

--only steps: the bf16 and fp8 steps alone -- what a tree without the format has; --tree DIR imports the package from another
checkout (the parent commit), so the same lines can be taken on both in turn.  --only products: the fp8 and mxfp4 steps and the
products section alone (how a build with another W4_UNIT_COLS in csrc/gemv_route.h was compared)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = []


def say(s=""):
    print(s, flush=True)
    OUT.append(s)


def med3(reps, unit=1.0):
    return "  ".join("%8.3f" % (statistics.median(r) * unit) for r in reps) + "    %8.3f .. %8.3f" % (
        min(min(r) for r in reps) * unit, max(max(r) for r in reps) * unit)


def mid(reps):
    return statistics.median([statistics.median(r) for r in reps])


def timed(fn, reset, stream):
    """ms of fn() on `stream`: the events sit on the stream the work runs on"""
    with torch.cuda.stream(stream):
        if reset:
            reset()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
    return a.elapsed_time(b)


def interleaved(lines, args, warm=5):
    """lines: name -> (fn, reset, stream).  -> name -> [reps][calls] ms"""
    for line in lines.values():
        for _ in range(warm):
            timed(*line)
    reps = {k: [[] for _ in range(args.reps)] for k in lines}
    for r in range(args.reps):
        for _ in range(args.blocks):
            for k, line in lines.items():
                timed(*line)
                reps[k][r] += [timed(*line) for _ in range(args.per_block)]
    return reps


def report(title, reps, base, unit=1.0, what="ms"):
    say(title + ": events %s, median of each of %d repetitions    min .. max of all calls" % (what, len(next(iter(reps.values())))))
    for k, r in reps.items():
        say("  %-28s %s    ratio to %s %.3f" % (k, med3(r, unit), base, mid(r) / mid(reps[base])))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/mxfp4.txt (--only packed: profiles/mxfp4_mfma.txt)")
    ap.add_argument("--rows", type=int, default=259)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--per-block", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="all", choices=["all", "steps", "products", "packed", "prefill", "whole_m", "w4a8"])
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is timed")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", {"packed": "mxfp4_mfma.txt", "prefill": "mxfp4_prefill.txt", "whole_m": "mxfp4_whole_m.txt", "w4a8": "mxfp4_w4a8.txt"}.get(args.only, "mxfp4.txt"))
    sys.path.insert(0, os.path.abspath(args.tree))
    sys.path.insert(1, ROOT)
    assert torch.cuda.is_available(), "a timing needs the MI355X"
    import bench
    from spatialrgpt_amd import _lib as L, ops
    from spatialrgpt_amd.engine import SrgptEngine
    from spatialrgpt_amd.weights import synth_state_dict

    dev, dt = torch.device("cuda:0"), torch.bfloat16
    cfg = bench.make_cfg("vila15_8b")
    lib = L.load()
    have4 = hasattr(lib, "srgpt_gemv_w4")
    have_direct = hasattr(lib, "srgpt_gemm_w4_direct")  # (the parent commit's tree has neither the entries nor the engine's option)
    formats = ["fp8", "mxfp4", "mxfp4p"] if args.only == "packed" else ["fp8", "mxfp4"] if args.only == "products" else ["native", "fp8"] + (["mxfp4"] if have4 and args.only in ("all", "prefill", "whole_m") else [])
    if args.only == "whole_m" and have_direct:
        formats.append("mxfp4d")
    have_w4a8 = hasattr(lib, "srgpt_gemm_w4a8")
    if args.only == "w4a8":
        formats = ["native", "fp8_w8a8", "mxfp4d"] + (["mxfp4_w4a8"] if have_w4a8 else [])
    name = {"native": "bf16", "fp8": "fp8", "mxfp4": "mxfp4", "mxfp4p": "mxfp4 packed", "mxfp4d": "mxfp4 direct", "fp8_w8a8": "fp8_w8a8",
            "mxfp4_w4a8": "mxfp4_w4a8"}
    base_fmt = "fp8_w8a8" if args.only == "w4a8" else "fp8"
    eng, held = {}, {}
    for f in formats:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        sd = synth_state_dict(cfg, seed=0, dtype=dt, device=dev)
        kw = dict(llm_weight_format="mxfp4", mxfp4_packed=True) if f == "mxfp4p" else \
            dict(llm_weight_format="mxfp4", mxfp4_prefill_direct=True) if f == "mxfp4d" else dict(llm_weight_format=f)
        eng[f] = SrgptEngine(cfg, sd, device=dev, dtype=dt, rope_positions=1024, consume_state_dict=True, **kw)
        del sd
        torch.cuda.synchronize()
        held[f] = torch.cuda.memory_allocated() - before
    say("scripts/time_mxfp4.py --only %s, tree %s: VILA1.5-8B geometry (hidden %d, inter %d, %d layers, heads %d / %d, vocab %d), "
        "synthetic weights, %s, %d CUs" % (args.only, os.path.relpath(os.path.abspath(args.tree), ROOT), cfg.hidden, cfg.inter, cfg.layers, cfg.heads, cfg.kv_heads,
                                           cfg.vocab, torch.cuda.get_device_name(0), lib.srgpt_device_cus()))
    say()
    g = torch.Generator(device=dev).manual_seed(3)

    def step_line(f, B, T=None):
        """a fresh state of B sequences over `rows` cached rows and its captured plain (T None) or lookup (T rows) step"""
        e = eng[f]
        x = (torch.randn((B, args.rows, cfg.hidden), device=dev, generator=g) * 0.5).to(dt)
        st, _, _ = e.prefill(x, max_new=64, fresh_state=True)
        with torch.cuda.stream(e.stream):
            e.stream.wait_stream(torch.cuda.default_stream())
            L.check(lib.srgpt_llm_sample_first(C.byref(e.w.llm), C.byref(st.c), ops._stream()))
            if T is None:
                graph = st.ensure_graph()
            else:
                if B == 1:
                    st.ensure_lookup(T - 1, 2, None)
                    graph = st.ensure_lookup_graph()
                else:  # the batched lookup step: B sequences of T rows
                    st.ensure_lookup_batch(T - 1, 2, None)
                    st.lookup_b["steps"].fill_(1)
                    graph = st.ensure_lookup_batch_graph()
        torch.cuda.synchronize()

        def reset():
            st.pos.fill_(args.rows)
            st.step.fill_(1)
            if T is not None and B > 1:
                st.lookup_b["steps"].fill_(1)

        def fn():
            L.check(lib.srgpt_graph_launch(graph, 1, ops._stream()))

        def check():
            rc = lib.srgpt_llm_decode_sync_state(C.byref(e.w.llm), C.byref(st.c), ops._stream())
            assert rc == 0, L.last_error()

        return (fn, reset, e.stream), check, st

    checks, keep = [], []

    def section(title, specs, base):
        lines = {}
        for label, (f, B, T) in specs.items():
            line, check, st = step_line(f, B, T)
            lines[label] = line
            checks.append(check)
            keep.append(st)
        reps = interleaved(lines, args)
        report(title, reps, base)
        return reps

    shared = torch.cuda.Stream()  # the product graphs' stream

    section("captured batch-1 decode step, %d cached rows" % args.rows, {name[f]: (f, 1, None) for f in formats}, base_fmt)
    if args.only == "packed":
        assert eng["mxfp4p"].w.mxfp4_packed
        three = lambda B, T: {name[f]: (f, B, T) for f in ("mxfp4", "mxfp4p", "fp8")}
        for K in (1, 2, 3):
            section("captured lookup step, K = %d (T = %d rows), batch 1" % (K, K + 1), three(1, K + 1), "mxfp4")
        for B in (4, 8):
            section("captured batch-%d decode step" % B, three(B, None), "mxfp4")
        for B in (2, 4):
            section("captured batched lookup step, (%d, 4): %d rows" % (B, 4 * B), three(B, 4), "mxfp4")
    if args.only == "all" and have4:
        section("captured lookup step, K = 3 (T = 4 rows), batch 1", {"fp8": ("fp8", 1, 4), "mxfp4": ("mxfp4", 1, 4)}, "fp8")
        section("captured batch-8 decode step (fp8: one MFMA pass of 8 rows; mxfp4: two VALU passes of 4)",
                {"fp8": ("fp8", 8, None), "mxfp4": ("mxfp4", 8, None)}, "fp8")
    for c in checks:
        c()
    keep.clear()
    if args.only == "packed":
        # ---- the four products alone: the VALU kernel, the MFMA product over the packed copy, fp8 on the MFMA kernel (its packed copy)
        w8, w4 = eng["fp8"].w, eng["mxfp4p"].w
        Hd, I, HqD, QW = cfg.hidden, cfg.inter, cfg.heads * cfg.head_dim, (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim
        shapes = {"q/k/v   [%d, %d] norm" % (QW, Hd): ("wqkv", QW, Hd, True, False, False),
                  "o_proj  [%d, %d] residual" % (Hd, HqD): ("wo", Hd, HqD, False, True, False),
                  "gate/up [2 x %d, %d] norm, SwiGLU" % (I, Hd): ("wgu", I, Hd, True, False, True),
                  "down    [%d, %d] residual" % (Hd, I): ("wdown", Hd, I, False, True, False)}
        say("the four products alone, one launch per layer (%d matrices) in a captured graph: us per launch (min .. max of all calls)" % cfg.layers)
        with torch.cuda.stream(shared):
            for title, (k, N, K, norm, res, sw) in shapes.items():
                for rows in (1, 2, 3, 4, 8, 16):
                    x = (torch.randn((rows, K), device=dev, generator=g) * 0.5).to(dt)
                    nw = torch.ones((K,), device=dev, dtype=dt) if norm else None
                    r = (torch.randn((rows, N), device=dev, generator=g) * 0.5).to(dt) if res else None
                    out = torch.empty((rows, N), device=dev, dtype=dt)
                    R = 2 * N if sw else N

                    def launches(fmt):
                        for i in range(cfg.layers):
                            if fmt == "w4":
                                ops.gemv_w4(x, w4.llm_q4[k][0][i], w4.llm_q4[k][1][i], nw, 1e-5, r, sw, out=out)
                            elif fmt == "w4p":
                                ops.gemv_w4p(x, w4.p4[k][i][1], R, nw, 1e-5, r, sw, out=out)
                            elif k in w8.llm_pk:
                                ops.gemv_rowss(x, w8=w8.llm_pk[k][i], wscale=w8.llm_q[k][1][i], norm_w=nw, eps=1e-5, residual=r, swiglu=sw,
                                               out=out, packed_rows=w8.pk_rows[k], n_rows=R)
                            else:
                                ops.gemv_rowss(x, w8=w8.llm_q[k][0][i], wscale=w8.llm_q[k][1][i], norm_w=nw, eps=1e-5, residual=r, swiglu=sw, out=out)

                    lines = {}
                    for fmt in ("w4", "w4p") + (("fp8",) if rows >= 2 else ()):  # (one fp8 row takes a kernel without the hand-off)
                        launches(fmt)  # first use of an instance outside the capture
                        torch.cuda.synchronize()
                        gr = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(gr, stream=shared):
                            launches(fmt)
                        lines[fmt] = (gr.replay, None, shared)
                    reps = interleaved(lines, args)
                    us = lambda f: "%7.2f (%7.2f .. %7.2f)" % (mid(reps[f]) * 1e3 / cfg.layers, min(map(min, reps[f])) * 1e3 / cfg.layers,
                                                             max(map(max, reps[f])) * 1e3 / cfg.layers)
                    say("  %-36s %2d row%s   gemv_w4 %s   gemv_w4p %s   fp8 %s   w4p / w4 %.3f" % (
                        title, rows, " " if rows == 1 else "s", us("w4"), us("w4p"), us("fp8") if "fp8" in reps else "      -" + " " * 21,
                        mid(reps["w4p"]) / mid(reps["w4"])))
        say()
        say("HBM held per engine (torch.cuda.memory_allocated around its construction):")
        for f in formats:
            say("  %-13s %7.3f GB" % (name[f], held[f] / 1e9))
        say("  mxfp4_packed_bytes() %.3f GB: the packed copies, on top of the row-major codes and scales" % (eng["mxfp4p"].w.mxfp4_packed_bytes() / 1e9))
        say()

    if args.only in ("all", "products") and have4:
        # ---- the four products alone
        w8, w4 = eng["fp8"].w, eng["mxfp4"].w
        Hd, I, HqD, QW = cfg.hidden, cfg.inter, cfg.heads * cfg.head_dim, (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim
        shapes = {"q/k/v   [%d, %d] norm" % (QW, Hd): ("wqkv", QW, Hd, True, False, False),
                  "o_proj  [%d, %d] residual" % (Hd, HqD): ("wo", Hd, HqD, False, True, False),
                  "gate/up [2 x %d, %d] norm, SwiGLU" % (I, Hd): ("wgu", I, Hd, True, False, True),
                  "down    [%d, %d] residual" % (Hd, I): ("wdown", Hd, I, False, True, False)}
        say("the four products alone, one launch per layer (%d matrices) in a captured graph: us per launch" % cfg.layers)
        with torch.cuda.stream(shared):
            for title, (k, N, K, norm, res, sw) in shapes.items():
                for rows in (1, 2, 3, 4):
                    x = (torch.randn((rows, K), device=dev, generator=g) * 0.5).to(dt)
                    nw = torch.ones((K,), device=dev, dtype=dt) if norm else None
                    r = (torch.randn((rows, N), device=dev, generator=g) * 0.5).to(dt) if res else None
                    out = torch.empty((rows, N), device=dev, dtype=dt)

                    def launches(fmt):
                        for i in range(cfg.layers):
                            if fmt == "fp8":
                                ops.gemv_w8(x, w8.llm_q[k][0][i], w8.llm_q[k][1][i], nw, 1e-5, r, sw, out=out)
                            else:
                                ops.gemv_w4(x, w4.llm_q4[k][0][i], w4.llm_q4[k][1][i], nw, 1e-5, r, sw, out=out)

                    lines = {}
                    for fmt in ("fp8", "mxfp4"):
                        launches(fmt)  # first use of an instance outside the capture
                        torch.cuda.synchronize()
                        gr = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(gr, stream=shared):
                            launches(fmt)
                        lines[fmt] = (gr.replay, None, shared)
                    reps = interleaved(lines, args)
                    say("  %-36s %d row%s   fp8 %7.2f (%7.2f .. %7.2f)   mxfp4 %7.2f (%7.2f .. %7.2f)   mxfp4 / fp8 %.3f" % (
                        title, rows, " " if rows == 1 else "s",
                        mid(reps["fp8"]) * 1e3 / cfg.layers, min(map(min, reps["fp8"])) * 1e3 / cfg.layers, max(map(max, reps["fp8"])) * 1e3 / cfg.layers,
                        mid(reps["mxfp4"]) * 1e3 / cfg.layers, min(map(min, reps["mxfp4"])) * 1e3 / cfg.layers, max(map(max, reps["mxfp4"])) * 1e3 / cfg.layers,
                        mid(reps["mxfp4"]) / mid(reps["fp8"])))
        say()

    if args.only in ("all", "prefill", "whole_m") and have4:
        # ---- prefill and append
        x = (torch.randn((1, args.rows + 32, cfg.hidden), device=dev, generator=g) * 0.5).to(dt)
        head, tail = x[:, :args.rows].contiguous(), x[:, args.rows:].contiguous()
        lines_p, lines_a = {}, {}
        for f in (formats if args.only in ("prefill", "whole_m") else ("fp8", "mxfp4")):
            e = eng[f]
            st = e.new_state(1, 512, 4)
            keep.append(st)

            def prefill(e=e, st=st):
                e.prefill(head, max_new=4, state=st)

            def append(e=e, st=st):
                e.append(st, tail)

            def back(st=st):
                st.pos.fill_(args.rows)
                st.host_len = [args.rows]

            with torch.cuda.stream(e.stream):
                prefill()
            torch.cuda.synchronize()
            lines_p[name[f]] = (prefill, None, e.stream)
            lines_a[name[f]] = (append, back, e.stream)
        report("%d-row prefill, eager" % args.rows, interleaved(lines_p, args), "fp8")
        report("32-row append over %d cached rows, eager" % args.rows, interleaved(lines_a, args), "fp8")

    if args.only == "w4a8":
        # ---- prefill at 1 x, 4 x and 8 x rows; the append
        for B in (1, 4, 8):
            x = (torch.randn((B, args.rows, cfg.hidden), device=dev, generator=g) * 0.5).to(dt)
            lines_p = {}
            for f in formats:
                e = eng[f]
                st = e.new_state(B, args.rows + 8, 4, ws_tokens=args.rows)

                def prefill(e=e, st=st, x=x):
                    e.prefill(x, max_new=4, state=st)

                with torch.cuda.stream(e.stream):
                    prefill()
                torch.cuda.synchronize()
                lines_p[name[f]] = (prefill, None, e.stream)
            report("%d x %d-row prefill (%d rows), eager" % (B, args.rows, B * args.rows), interleaved(lines_p, args), base_fmt)
            del lines_p, st
        x = (torch.randn((1, args.rows + 32, cfg.hidden), device=dev, generator=g) * 0.5).to(dt)
        head, tail = x[:, :args.rows].contiguous(), x[:, args.rows:].contiguous()
        lines_a = {}
        for f in formats:
            e = eng[f]
            st = e.new_state(1, 512, 4)
            keep.append(st)

            def append(e=e, st=st):
                e.append(st, tail)

            def back(st=st):
                st.pos.fill_(args.rows)
                st.host_len = [args.rows]

            with torch.cuda.stream(e.stream):
                e.prefill(head, max_new=4, state=st)
            torch.cuda.synchronize()
            lines_a[name[f]] = (append, back, e.stream)
        report("32-row append over %d cached rows, eager" % args.rows, interleaved(lines_a, args), base_fmt)

    if args.only == "w4a8" and have_w4a8:
        # ---- the four layer products alone at 8 x rows: W4A8, W8A8, expansion + bf16
        w4, w8 = eng["mxfp4_w4a8"].w, eng["fp8_w8a8"].w
        Hd, I, HqD, QW, M = cfg.hidden, cfg.inter, cfg.heads * cfg.head_dim, (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim, 8 * args.rows
        shapes = {"q/k/v   [%d, %d]" % (QW, Hd): ("wqkv", QW, Hd, False), "o_proj  [%d, %d] residual" % (Hd, HqD): ("wo", Hd, HqD, True),
                  "gate/up [%d, %d]" % (2 * I, Hd): ("wgu", 2 * I, Hd, False), "down    [%d, %d] residual" % (Hd, I): ("wdown", Hd, I, True)}
        say("the four layer products alone at %d rows, one launch per layer (%d matrices) in a captured graph: us per launch, median "
            "(min .. max of all calls)" % (M, cfg.layers))
        with torch.cuda.stream(shared):
            for title, (k, N, K, res) in shapes.items():
                x = (torch.randn((M, K), device=dev, generator=g) * 0.5).to(dt)
                a8, asc = ops.quant_rows_e4m3(x)
                r = (torch.randn((M, N), device=dev, generator=g) * 0.5).to(dt) if res else None
                out = torch.empty((M, N), device=dev, dtype=dt)
                expand = torch.empty((N, K), device=dev, dtype=dt)
                assert not ops.gemm_w4_in_kernel(M, N, K)

                def launches(fmt):
                    for i in range(cfg.layers):
                        if fmt == "w4a8":
                            ops.gemm_w4a8(a8, asc, w4.llm_q4[k][0][i], w4.llm_q4[k][1][i], residual=r, out=out)
                        elif fmt == "w8a8":
                            ops.gemm_w8a8(a8, asc, w8.llm_q[k][0][i], w8.llm_q[k][1][i], residual=r, out=out)
                        else:
                            ops.gemm_w4(x, w4.llm_q4[k][0][i], w4.llm_q4[k][1][i], residual=r, out=out, expand=expand)

                lines = {}
                for fmt in ("w4a8", "w8a8", "expand"):
                    launches(fmt)  # first use of an instance outside the capture
                    torch.cuda.synchronize()
                    gr = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gr, stream=shared):
                        launches(fmt)
                    lines[fmt] = (gr.replay, None, shared)
                reps = interleaved(lines, args)
                us = lambda f: "%7.2f (%7.2f .. %7.2f)" % (mid(reps[f]) * 1e3 / cfg.layers, min(map(min, reps[f])) * 1e3 / cfg.layers,
                                                         max(map(max, reps[f])) * 1e3 / cfg.layers)
                say("  %-34s gemm_w4a8 %s   gemm_w8a8 %s   expansion + bf16 gemm %s   w4a8 / w8a8 %.3f   w4a8 / expansion %.3f" % (
                    title, us("w4a8"), us("w8a8"), us("expand"), mid(reps["w4a8"]) / mid(reps["w8a8"]), mid(reps["w4a8"]) / mid(reps["expand"])))
        say()

    if args.only == "whole_m" and have_direct:
        # ---- the three whole-M products alone: codes in the kernel, expansion + bf16 launch, bf16 launch alone
        w4, wn = eng["mxfp4"].w, eng["native"].w
        Hd, I, QW, M = cfg.hidden, cfg.inter, (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim, args.rows
        shapes = {"q/k/v   [%d, %d]" % (QW, Hd): ("wqkv", QW, Hd, False, False),
                  "gate/up [2 x %d, %d] SwiGLU" % (I, Hd): ("wgu", I, Hd, False, True),
                  "down    [%d, %d] residual" % (Hd, I): ("wdown", Hd, I, True, False)}
        say("the whole-M products alone at %d rows, one launch per layer (%d matrices) in a captured graph: us per launch, median "
            "(min .. max of all calls)" % (M, cfg.layers))
        with torch.cuda.stream(shared):
            for title, (k, N, K, res, sw) in shapes.items():
                x = (torch.randn((M, K), device=dev, generator=g) * 0.5).to(dt)
                r = (torch.randn((M, N), device=dev, generator=g) * 0.5).to(dt) if res else None
                out = torch.empty((M, N), device=dev, dtype=dt)
                expand = torch.empty(((2 * N if sw else N), K), device=dev, dtype=dt)
                assert ops.gemm_w4_in_kernel(M, N, K, swiglu=sw, direct=True) and not ops.gemm_w4_in_kernel(M, N, K, swiglu=sw)

                def launches(fmt):
                    for i in range(cfg.layers):
                        c, s = w4.llm_q4[k][0][i], w4.llm_q4[k][1][i]
                        if fmt == "bf16":
                            ops.gemm_swiglu(x, wn.llm_t[k][i], out=out) if sw else ops.gemm(x, wn.llm_t[k][i], residual=r, out=out)
                        elif sw:
                            ops.gemm_w4_swiglu(x, c, s, out=out, expand=expand, direct=fmt == "w4")
                        else:
                            ops.gemm_w4(x, c, s, residual=r, out=out, expand=expand, direct=fmt == "w4")

                lines = {}
                for fmt in ("w4", "expand", "bf16"):
                    launches(fmt)  # first use of an instance outside the capture
                    torch.cuda.synchronize()
                    gr = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gr, stream=shared):
                        launches(fmt)
                    lines[fmt] = (gr.replay, None, shared)
                reps = interleaved(lines, args)
                us = lambda f: "%7.2f (%7.2f .. %7.2f)" % (mid(reps[f]) * 1e3 / cfg.layers, min(map(min, reps[f])) * 1e3 / cfg.layers,
                                                         max(map(max, reps[f])) * 1e3 / cfg.layers)
                say("  %-34s W4 instance %s   expansion + bf16 %s   bf16 alone %s   W4 / expansion %.3f   W4 / bf16 %.3f" % (
                    title, us("w4"), us("expand"), us("bf16"), mid(reps["w4"]) / mid(reps["expand"]), mid(reps["w4"]) / mid(reps["bf16"])))
        say()

    say("llm_weight_bytes() (streamed per decoded token at batch 1):")
    base = eng[formats[0]].w.llm_weight_bytes()
    for f in formats:
        n = eng[f].w.llm_weight_bytes()
        say("  %-6s %12d bytes   %.3f of %s" % (name[f], n, n / base, name[formats[0]]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
