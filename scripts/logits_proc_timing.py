"""What the device logits processors cost (profiles/logits_processors.txt): ms per graph-captured decode step of the flagship geometry
(VILA1.5-8B, bf16, bs = 1, T = 259) with the processors off -- the entry points and graph every other request takes -- and with
repetition_penalty + no_repeat_ngram_size = 3 on, at 128 and 1024 generated tokens, alternating, three rounds each; then the
processor launch alone (device events around 200 back-to-back launches) at histories of 128 and 1024 ids.
  python scripts/logits_proc_timing.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from spatialrgpt_amd import ops
from spatialrgpt_amd.config import SrgptConfig
from spatialrgpt_amd.engine import SrgptEngine
from spatialrgpt_amd.weights import synth_state_dict

cfg = SrgptConfig.vila15_8b()
T = 259
PROC = dict(repetition_penalty=1.5, no_repeat_ngram_size=3, min_new_tokens=0, eos_token_ids=None)
sd = synth_state_dict(cfg, seed=0, dtype=torch.bfloat16, device="cuda")
eng = SrgptEngine(cfg, sd, device="cuda", dtype=torch.bfloat16, rope_positions=2048, consume_state_dict=True)
del sd
x = torch.randn((1, T, cfg.hidden), device="cuda").to(torch.bfloat16)


def step_ms(G, proc):
    st, _, _ = eng.prefill(x, max_new=1024)  # one pooled state (and one pair of graphs) for both lengths
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    eng.greedy_decode(st, G, logits_proc=proc)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / G


for G in (128, 1024):
    step_ms(G, None), step_ms(G, PROC)  # warm-up: both graphs captured, code objects loaded
    rows = {"off": [], "on": []}
    for rep in range(3):
        rows["off"].append(step_ms(G, None))
        rows["on"].append(step_ms(G, PROC))
    for k, v in rows.items():
        print(f"decode step, {G} new tokens, processors {k}: " + " ".join(f"{t:.4f}" for t in v) + f" ms/step (min {min(v):.4f} = "
              f"{1e3 / min(v):.1f} tok/s decode-only)", flush=True)
    print(f"  on - off (min): {(min(rows['on']) - min(rows['off'])) * 1e3:.1f} us per step; spread of off: "
          f"{(max(rows['off']) - min(rows['off'])) * 1e3:.1f} us", flush=True)

V = cfg.vocab
params = ops.LogitsProcParams("cuda").set(**PROC)
scores = torch.randn((1, V), device="cuda")
for n in (128, 1024):
    ids = torch.randint(0, V, (1, 1024), device="cuda")
    ids[0, 1::2] = ids[0, 0]  # repeated ids and repeated 2-gram prefixes: the n-gram phase compares all three ids
    for rep in range(2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(200):
            ops.logits_process(scores, params, ids, n)
        e1.record()
        torch.cuda.synchronize()
    print(f"srgpt_logits_process alone, V = {V}, history {n} ids: {e0.elapsed_time(e1) / 200 * 1e3:.1f} us per launch "
          "(200 back-to-back launches, launch overhead included)", flush=True)
