// The 13-bit lossless code of a bf16 weight matrix that the batch-1 decode products stream (gemv_p13.hip), as plain C++ usable from
// host and device: tests/test_host_pack13.py compiles this header alone and round-trips every bf16 bit pattern through it.
//
// A bf16 weight is s | e8 | m7.  In a weight row the exponent takes a few dozen values, all close below the row's largest, so a
// row stores a BASE exponent b and each weight the 5-bit code c = e - b, c in [0, 31]:  s | c5 | m7 = 13 bits = 0.8125 of the
// bytes, every weight reconstructed bit for bit.
//   * The base is PER ROW (the rows of an embedding-shaped matrix such as lm_head differ in scale by more than a window; a row's
//     base costs the kernel one scalar register) and EVEN: then bit 0 of e is bit 0 of c, the low byte (e0 | m7) of the weight is
//     stored as it is, and the high byte is s << 7 | (b / 2 + (c >> 1)) -- one 32-bit add of b / 2 replicated into four bytes
//     restores four weights' high bytes, with no carry between bytes because e <= 254.  An even base makes the window 31 or 32
//     exponents wide: b = max(emax - 31, 1) rounded up to even.
//   * e = 0 (zeros, denormals) and e = 255 (Inf, NaN) are never coded (the cheap form of the decode: no special case for c = 0).
//     A row that holds one of them, or a value below its window, is an EXCEPTION ROW: its meta word is P13_EXCEPTION, its packed
//     bytes are zeros, and the product streams it from the raw matrix, which stays resident for the prefill anyway.  So the code is
//     lossless for every possible bf16 input.
//
// Storage.  A row is cut into GROUPS of 4 chunk iterations = 2048 weights (a row of K % 512 == 0 weights is padded to whole groups;
// padded weights are stored as zeros and multiply activations the kernel zero-fills).  In iteration t of group g, lane l owns the 8
// weights k = ((4 g + t) * 64 + l) * 8 + i, i = 0 .. 7 -- exactly what the raw kernel's 16-byte load number 4 g + t gives lane l.
// A group is three planes, each one contiguous wave load, in the order the kernel issues and consumes them:
//   sign  [64 lanes][ 4 B]   256 B   bit 8 j + 7 - (2 t + h) = sign of weight i = 4 h + j of iteration t
//   nib   [64 lanes][16 B]  1024 B   dword t: nibble 2 j + h = c >> 1 of weight i = 4 h + j
//   low   [2][64 lanes][16 B] 2048 B load t / 2, dword 2 (t % 2) + h: byte j = low byte of weight i = 4 h + j
// = 3328 bytes per group; a K = 4096 row is 6656 bytes against 8192.  The placement makes the decode of four weights
//   H = (((sign << (2 t + h)) & 0x80808080) | ((nib >> 4 h) & 0x0f0f0f0f)) + bb4        (the four high bytes)
//   fp32 bits of weight j = H.byte[j] << 24 | low.byte[j] << 16                          (one v_perm_b32 each)
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define P13_HD __host__ __device__ inline
#else
#define P13_HD inline
#endif

constexpr int P13_GROUP_ITS = 4;                      // chunk iterations (64 lanes x 8 weights) per group
constexpr int P13_GROUP_WEIGHTS = P13_GROUP_ITS * 512;
constexpr int P13_SIGN_OFF = 0, P13_NIB_OFF = 256, P13_LOW_OFF = 1280;
constexpr int P13_GROUP_BYTES = 3328;
constexpr uint32_t P13_EXCEPTION = 0xffffffffu;       // meta word of an exception row (a base byte is at most 0x7f)

P13_HD bool p13_eligible(long long N, long long K) { return N > 0 && K > 0 && K % 512 == 0; }
P13_HD int p13_groups(int K) { return (K + P13_GROUP_WEIGHTS - 1) / P13_GROUP_WEIGHTS; }
P13_HD size_t p13_row_bytes(int K) { return (size_t)p13_groups(K) * P13_GROUP_BYTES; }
P13_HD size_t p13_packed_bytes(int N, int K) { return (size_t)N * p13_row_bytes(K); }
// one meta word per row, and one more word: the exception-row count the pack kernel leaves behind
P13_HD size_t p13_meta_bytes(int N) { return ((size_t)N + 1) * sizeof(uint32_t); }

// The meta word of a row from what a scan of its exponents found: the largest and smallest exponent field, and whether a 0 or a
// 255 occurred.  b / 2 replicated into four bytes, or P13_EXCEPTION.
P13_HD uint32_t p13_meta(int emax, int emin, bool zero_or_special) {
  if (zero_or_special) return P13_EXCEPTION;
  int b = emax - 31 < 1 ? 1 : emax - 31;
  b += b & 1;
  if (emin < b) return P13_EXCEPTION;
  return (uint32_t)(b >> 1) * 0x01010101u;
}
P13_HD int p13_meta_base(uint32_t meta) { return (int)(meta & 0xffu) * 2; }

P13_HD uint32_t p13_row_meta(const uint16_t* row, int K) {
  int emax = 0, emin = 255;
  bool bad = false;
  for (int k = 0; k < K; ++k) {
    const int e = (row[k] >> 7) & 0xff;
    emax = e > emax ? e : emax;
    emin = e < emin ? e : emin;
    bad = bad || e == 0 || e == 255;
  }
  return p13_meta(emax, emin, bad);
}

// what lane `lane` stores for group g of a coded row: one sign dword, the four nibble dwords, the eight low-byte dwords (two loads)
struct P13Lane {
  uint32_t sign, nib[4], low[8];
};
P13_HD P13Lane p13_encode_lane(const uint16_t* row, int K, uint32_t meta, int g, int lane) {
  P13Lane o{};
  const int b = p13_meta_base(meta);
  for (int t = 0; t < P13_GROUP_ITS; ++t)
    for (int i = 0; i < 8; ++i) {
      const long long k = ((long long)(P13_GROUP_ITS * g + t) * 64 + lane) * 8 + i;
      if (k >= K) continue;  // padding: zeros
      const uint32_t v = row[k], c = ((v >> 7) & 0xffu) - (uint32_t)b, h = (uint32_t)i >> 2, j = (uint32_t)i & 3;
      o.sign |= (v >> 15) << (8 * j + 7 - (2 * t + h));
      o.nib[t] |= (c >> 1) << (8 * j + 4 * h);
      o.low[2 * t + h] |= (v & 0xffu) << (8 * j);
    }
  return o;
}

// the four high bytes (s << 7 | e >> 1) of weights i = 4 h .. 4 h + 3 of iteration t
P13_HD uint32_t p13_high4(uint32_t sign, uint32_t nib, uint32_t bb4, int t, int h) {
  return (((sign << (2 * t + h)) & 0x80808080u) | ((nib >> (4 * h)) & 0x0f0f0f0fu)) + bb4;
}
// fp32 bits of weight j of four: its bf16 bits in the upper half
P13_HD uint32_t p13_f32_bits(uint32_t high4, uint32_t low4, int j) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(high4, low4, ((4u + j) << 24) | ((uint32_t)j << 16) | 0x0c0cu);
#else
  return ((high4 >> (8 * j)) & 0xffu) << 24 | ((low4 >> (8 * j)) & 0xffu) << 16;
#endif
}

// byte offsets of a lane's pieces inside a row's packed bytes
P13_HD size_t p13_sign_off(int g, int lane) { return (size_t)g * P13_GROUP_BYTES + P13_SIGN_OFF + (size_t)lane * 4; }
P13_HD size_t p13_nib_off(int g, int lane) { return (size_t)g * P13_GROUP_BYTES + P13_NIB_OFF + (size_t)lane * 16; }
P13_HD size_t p13_low_off(int g, int load, int lane) {
  return (size_t)g * P13_GROUP_BYTES + P13_LOW_OFF + (size_t)load * 1024 + (size_t)lane * 16;
}

// ---- whole rows on the host: the reference of the device kernels (pack13.hip) and the test program's subject ----
// `packed`: p13_row_bytes(K) bytes, 4-byte aligned.  Returns the row's meta word.
inline uint32_t p13_pack_row(const uint16_t* row, int K, unsigned char* packed) {
  const uint32_t meta = p13_row_meta(row, K);
  for (int g = 0; g < p13_groups(K); ++g)
    for (int lane = 0; lane < 64; ++lane) {
      const P13Lane o = meta == P13_EXCEPTION ? P13Lane{} : p13_encode_lane(row, K, meta, g, lane);
      *reinterpret_cast<uint32_t*>(packed + p13_sign_off(g, lane)) = o.sign;
      for (int t = 0; t < 4; ++t) reinterpret_cast<uint32_t*>(packed + p13_nib_off(g, lane))[t] = o.nib[t];
      for (int q = 0; q < 8; ++q) reinterpret_cast<uint32_t*>(packed + p13_low_off(g, q >> 2, lane))[q & 3] = o.low[q];
    }
  return meta;
}
// `raw`: the row of the raw matrix, read only for an exception row
inline void p13_unpack_row(const unsigned char* packed, uint32_t meta, const uint16_t* raw, int K, uint16_t* out) {
  if (meta == P13_EXCEPTION) {
    for (int k = 0; k < K; ++k) out[k] = raw[k];
    return;
  }
  for (int g = 0; g < p13_groups(K); ++g)
    for (int lane = 0; lane < 64; ++lane) {
      const uint32_t sign = *reinterpret_cast<const uint32_t*>(packed + p13_sign_off(g, lane));
      for (int t = 0; t < 4; ++t) {
        const uint32_t nib = reinterpret_cast<const uint32_t*>(packed + p13_nib_off(g, lane))[t];
        for (int h = 0; h < 2; ++h) {
          const uint32_t low = reinterpret_cast<const uint32_t*>(packed + p13_low_off(g, t >> 1, lane))[2 * (t & 1) + h];
          const uint32_t high = p13_high4(sign, nib, meta, t, h);
          for (int j = 0; j < 4; ++j) {
            const long long k = ((long long)(P13_GROUP_ITS * g + t) * 64 + lane) * 8 + 4 * h + j;
            if (k < K) out[k] = (uint16_t)(p13_f32_bits(high, low, j) >> 16);
          }
        }
      }
    }
}
