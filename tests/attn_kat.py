"""The known-answer cases of tests/golden/attn_kat.npz: one launch of every reachable attention kernel instance (the decode kernels
through ops.decode_attention, the prefill kernels through ops.attention) on inputs that an integer hash generates -- the same bits
wherever it runs, none stored.  scripts/mint_attn_kat.py records the results with one build of the library,
tests/test_gpu_attn_kat.py asserts that the build under test reproduces them bit for bit -- the cases are enumerated here, once, for
both.  Which instance a case runs on is pinned on the CPU (tests/test_host_attn_route.py, tests/golden/attn_routes.json)."""
import zlib

import numpy as np
import torch

BF16, F32 = torch.bfloat16, torch.float32
DTYPE_NAME = {BF16: "bf16", F32: "f32"}

# decode: B = 2 sequences, one kv head, Hq = G
DECODE_POS = {512: [5, 300], 8192: [5000, 100]}
# prefill: B = 3, Tq = Tk = 130 (three 64-row tiles, the last one partial), Hq = 4, Hkv = 2
PREFILL_B, PREFILL_T, PREFILL_HQ, PREFILL_HKV = 3, 130, 4, 2
PREFILL_LENS = [130, 64, 7]
PREFILL_ROWS = (0, 129)  # query rows stored in full; every batch row also as a CRC-32


def hashed(shape, salt, dtype, scale=64):
    """a tensor of k / scale, k in [-128, 127] from a 32-bit integer hash of (salt, flat index): exact in bf16 and fp32"""
    n = int(np.prod(shape))
    x = np.arange(n, dtype=np.uint32)
    with np.errstate(over="ignore"):
        x = (x + np.uint32(0x9E3779B9) * np.uint32(salt + 1)) * np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(13)
    v = ((x >> np.uint32(24)).astype(np.int32) - 128).astype(np.float32) / np.float32(scale)
    if dtype == F32:
        return torch.from_numpy(v.reshape(shape))
    return torch.from_numpy((v.view(np.uint32) >> np.uint32(16)).astype(np.uint16).view(np.int16).reshape(shape)).view(BF16)


def bits(t):
    """the tensor's bits, on the host, as unsigned integers"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == BF16 else t.view(torch.int32).numpy().view(np.uint32)


def decode_cases():
    """-> (name, dtype, D, G, max_pos): every decode_split_kernel<T, D, G> that can be reached, the four decode_mfma_kernel<G> (bf16,
    head_dim 128), and one of those with 128 keys per block"""
    for dtype in (BF16, F32):
        for D in (16, 32, 64, 128):
            for G in (1, 2, 4, 8):
                yield f"decode.{DTYPE_NAME[dtype]}.D{D}.G{G}.P512", dtype, D, G, 512
    yield "decode.bf16.D128.G2.P8192", BF16, 128, 2, 8192


def prefill_cases():
    """-> (name, dtype, D, causal): the eight flash_bf16_kernel<HDP, CAUSAL> (padded widths 32 / 64 / 96 / 128) and the one-wave
    kernel in bf16 (head_dim 20: not a multiple of 8) and fp32"""
    for causal in (False, True):
        for dtype, D in ((BF16, 32), (BF16, 64), (BF16, 80), (BF16, 128), (BF16, 20), (F32, 64)):
            yield f"prefill.{DTYPE_NAME[dtype]}.D{D}.causal{int(causal)}", dtype, D, causal


def run_cases(ops, device="cuda"):
    """every case on the loaded library -> {name + ".out": output bits, and for decode ".k" / ".v": the appended cache rows' bits,
    ".tickets": the arrival tickets after the launch; for prefill ".crc": CRC-32 of every batch row's output bits}"""
    out = {}
    for name, dtype, D, G, max_pos in decode_cases():
        pos = DECODE_POS[max_pos]
        B, Hq, Hkv = len(pos), G, 1
        qkv = hashed((B, (Hq + 2 * Hkv) * D), 1, dtype).to(device)
        kc = hashed((B, Hkv, max_pos, D), 2, dtype).to(device)
        vc = hashed((B, Hkv, max_pos, D), 3, dtype).to(device)
        cos_t, sin_t = hashed((max_pos, D // 2), 4, dtype, 128).to(device), hashed((max_pos, D // 2), 5, dtype, 128).to(device)
        ws, tickets = ops.decode_attention_ws(B, Hq, D, device)
        o = ops.decode_attention(qkv, kc, vc, torch.tensor(pos, dtype=torch.int32, device=device), cos_t, sin_t, Hq, Hkv, D, ws=ws)
        torch.cuda.synchronize()
        out[name + ".out"] = bits(o)
        out[name + ".k"] = bits(torch.stack([kc[b, 0, p] for b, p in enumerate(pos)]))
        out[name + ".v"] = bits(torch.stack([vc[b, 0, p] for b, p in enumerate(pos)]))
        out[name + ".tickets"] = tickets.cpu().numpy().astype(np.int32)
    B, T, Hq, Hkv = PREFILL_B, PREFILL_T, PREFILL_HQ, PREFILL_HKV
    kv_len = torch.tensor(PREFILL_LENS, dtype=torch.int32, device=device)
    for name, dtype, D, causal in prefill_cases():
        q, k, v = (hashed((B, T, h, D), 6 + i, dtype).to(device) for i, h in enumerate((Hq, Hkv, Hkv)))
        o = bits(ops.attention(q, k, v, causal=causal, kv_len=kv_len))
        out[name + ".out"] = np.ascontiguousarray(o[:, list(PREFILL_ROWS)])
        out[name + ".crc"] = np.array([zlib.crc32(o[b].tobytes()) for b in range(B)], dtype=np.int64)
    return out
