"""The known-answer cases of tests/golden/pick_kat.npz: the draws of both device samplers (ops.sample, ops.sample_full) on fixed
logits, seeds and counters.  scripts/mint_pick_kat.py records them with one build of the library, tests/test_gpu_pick.py asserts
that the build under test draws the same ids -- the cases are enumerated here, once, for both."""
import zlib

import numpy as np
import torch

STORED_V = (70, 1000)          # logits kept in the fixture (rows [3, V])
HASHED_V = (32002, 128258)     # logits regenerated from an integer hash of the index
BATCHES = (1, 3)
COUNTERS = (0, 5)
SAMPLE = ((1.0, 0, None), (0.7, 50, 0.9), (0.2, 1, None))            # ops.sample: (temperature, top_k, top_p)
SAMPLE_FULL = ((0.7, 0, 0.9), (0.7, 1000, None), (1.3, 64, 0.95))    # ops.sample_full


def hashed_logits(V):
    """fp32 [3, V] in [-8, 8): a 32-bit integer hash of the flat index (numpy: the same bits wherever it runs)"""
    x = np.arange(3 * V, dtype=np.uint32)
    with np.errstate(over="ignore"):
        x = (x + np.uint32(0x9E3779B9)) * np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(13)
    return ((x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -20) - np.float32(8.0)).reshape(3, V)


def stored_logits():
    """what the mint stores for STORED_V: fp32 [3, V] normal scores x 3 from a seeded numpy generator"""
    return {V: (np.random.RandomState(V).standard_normal((3, V)) * 3).astype(np.float32) for V in STORED_V}


def cases():
    """-> (name, V, B, counter, sampler name, (temperature, top_k, top_p), seed)"""
    n = 0
    for V in STORED_V + HASHED_V:
        for B in BATCHES:
            for counter in COUNTERS:
                for which, settings in (("sample", SAMPLE), ("sample_full", SAMPLE_FULL)):
                    for si, setting in enumerate(settings):
                        n += 1
                        yield f"{which}{si}.V{V}.B{B}.c{counter}", V, B, counter, which, setting, 1000 + n


def run_cases(ops, L, stored, device="cuda"):
    """every case on the loaded library -> {name + ".ids": int64 [B], ".counter": the block's counter after the call, and for the
    full sampler ".kept_count": int64 [B], ".kept_crc": CRC-32 of the kept mask's 32-bit words (bit i % 32 of word i / 32)}"""
    out, logits = {}, {}
    for V in STORED_V + HASHED_V:
        logits[V] = torch.from_numpy(np.ascontiguousarray(stored[V]) if V in STORED_V else hashed_logits(V)).to(device)
    for name, V, B, counter, which, (temperature, top_k, top_p), seed in cases():
        lg = logits[V][:B].contiguous()
        sp = ops.SamplingParams(device, B).set(temperature, top_k, top_p, seed=seed, counter=counter)
        if which == "sample":
            ids = ops.sample(lg, sp, check=True)
        else:
            ids, kept = ops.sample_full(lg, sp, kept_mask=True)
            kept = kept.cpu().numpy()
            bits = np.zeros((B, (V + 31) // 32 * 32), dtype=np.uint8)
            bits[:, :V] = kept
            words = np.packbits(bits, axis=1, bitorder="little")  # little-endian bytes of the uint32 words
            out[name + ".kept_count"] = kept.sum(axis=1).astype(np.int64)
            out[name + ".kept_crc"] = np.array(zlib.crc32(words.tobytes()), dtype=np.int64)
        out[name + ".ids"] = ids.cpu().numpy().astype(np.int64)
        out[name + ".counter"] = np.array(L.Sampling.from_buffer_copy(sp.buf.cpu().numpy().tobytes()).counter, dtype=np.int64)
    return out
