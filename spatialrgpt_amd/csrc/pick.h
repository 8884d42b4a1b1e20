// The token pick's contract: how st->logits become st->tok, for model.hip (argmax, the merge in advance_kernel) and sample.hip (both
// samplers, the stand-alone merge).  A row of V <= PICK_VOCAB_MAX scores is cut into PICK_SLICES contiguous slices; a producer kernel
// runs on a grid (PICK_SLICES, batch) of 256 threads and leaves ONE (value, index) pair per slice in pv / pi [batch][PICK_SLICES]
// (index PICK_NONE: the slice had no entry); a merge takes the best pair of the row.  "Best" is pick_better everywhere: the greater
// value, or the lower index among equal values (torch.argmax's first maximum).  Whoever produces partials elsewhere satisfies this
// header: pick_slice for the bounds, pick_gumbel_key for a draw, pick_store_slice to publish.
#pragma once
#include "common.h"
#include "draw_addr.h"

constexpr int PICK_SLICES = 128;                              // slices per row = blocks per row of a producer = partials per row
constexpr int PICK_SLICE_MAX = 2048;                          // entries of a slice (sample_partial_kernel holds one in LDS)
constexpr int PICK_VOCAB_MAX = PICK_SLICES * PICK_SLICE_MAX;  // 262144 = 2^18 (the full sampler's index digits rely on it)
constexpr int PICK_NONE = 0x7fffffff;                         // "no entry": loses every tie, merges to token 0
constexpr int SMP_K = 64;                                     // top-k-64 sampler: candidates per slice = the largest top_k it serves

// the one host check of the vocabulary limit; `who` = the caller's message prefix
static inline int pick_check_vocab(int V, const char* who) {
  SRGPT_CHECK(V <= PICK_VOCAB_MAX, SRGPT_ERR_UNSUPPORTED, "%s: vocabulary %d exceeds %d", who, V, PICK_VOCAB_MAX);
  return SRGPT_OK;
}

// ---- workspace layouts (ws == NULL: sizes only) ----
// top-k-64 sampler (srgpt_sample_ws_bytes): candidate keys u32 [B][128][64] | their indices i32 [B][128][64] | slice maxima f32
// [B][128] | their indices i32 [B][128] | error word (+ padding to 256 bytes)
struct SampleWs {
  unsigned* cand_key;
  int* cand_idx;
  float* pv;
  int* pi;
  int* err;
  int64_t bytes;
};
static inline SampleWs carve_sample_ws(const void* ws, int B) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(ws), cand = (uintptr_t)B * PICK_SLICES * SMP_K * 4, part = (uintptr_t)B * PICK_SLICES * 4;
  return SampleWs{reinterpret_cast<unsigned*>(p), reinterpret_cast<int*>(p + cand), reinterpret_cast<float*>(p + 2 * cand),
                  reinterpret_cast<int*>(p + 2 * cand + part), reinterpret_cast<int*>(p + 2 * cand + 2 * part),
                  (int64_t)(2 * cand + 2 * part + 256)};
}
// full sampler (srgpt_sample_full_ws_bytes): keys u32 [B][V] | thresholds u32 [B][4] | slice maxima f32 [B][128] | their indices i32
// [B][128].  head_bytes = keys + thresholds: what the decode step carves (its slice maxima are the argmax's)
struct SampleFullWs {
  unsigned *keys, *thr;
  float* pv;
  int* pi;
  size_t head_bytes;
  int64_t bytes;
};
static inline SampleFullWs carve_sample_full_ws(const void* ws, int B, int V) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(ws), keys = (uintptr_t)B * V * 4, head = keys + (uintptr_t)B * 16;
  const uintptr_t part = (uintptr_t)B * PICK_SLICES * 4;
  return SampleFullWs{reinterpret_cast<unsigned*>(p), reinterpret_cast<unsigned*>(p + keys), reinterpret_cast<float*>(p + head),
                      reinterpret_cast<int*>(p + head + part), (size_t)head, (int64_t)(head + 2 * part)};
}

// ---- device side ----
// is (v, i) a better pick than (ov, oi)?
__device__ __forceinline__ bool pick_better(float v, int i, float ov, int oi) { return v > ov || (v == ov && i < oi); }

// the slice [lo, hi) of a row of V entries that this block of a (slices, batch) grid scans
struct PickSlice {
  int lo, hi;
};
__device__ __forceinline__ PickSlice pick_slice(int V) {
  const int per = (V + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * per;
  return PickSlice{lo, min(lo + per, V)};
}

// the best pair of the wave, in every lane
__device__ __forceinline__ void pick_wave_reduce(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (pick_better(ov, oi, v, i)) {
      v = ov;
      i = oi;
    }
  }
}

// every thread of a 256-thread block of a (slices, batch) grid brings its best pair: the slice's goes to pv / pi
__device__ __forceinline__ void pick_store_slice(float v, int i, float* __restrict__ pv, int* __restrict__ pi) {
  __shared__ float sv[4];
  __shared__ int si[4];
  pick_wave_reduce(v, i);
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = v;
    si[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w)
      if (pick_better(sv[w], si[w], v, i)) {
        v = sv[w];
        i = si[w];
      }
    pv[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = v;
    pi[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = i;
  }
}

// one wave merges a row's nb partials: the row's token, in every lane
__device__ __forceinline__ int pick_merge_row(const float* __restrict__ pv, const int* __restrict__ pi, int nb, int lane) {
  float best = -INFINITY;
  int bi = PICK_NONE;
  for (int i = lane; i < nb; i += 64)
    if (pick_better(pv[i], pi[i], best, bi)) {
      best = pv[i];
      bi = pi[i];
    }
  pick_wave_reduce(best, bi);
  return bi == PICK_NONE ? 0 : bi;
}

// Philox4x32-10, keyed by the caller's seed; counter = (step counter, sequence, vocabulary index | ~0)
struct U4 {
  unsigned x, y, z, w;
};
__device__ __forceinline__ U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}
// Where row b of a sampler launch reads that stream.  The rows are the sequences of ONE step (PICK_ROWS_SEQS): (counter, b).  Or they
// are successive steps of ONE sequence (PICK_ROWS_STEPS, the lookup step's T rows): (counter + b, 0), the 64-bit sum carried into the
// high word -- exactly what B = 1 calls at counter, counter + 1, ... read, so a row's draw does not depend on which launch made it.
// Or they are B sequences x T successive steps (PICK_ROWS_SEQ_STEPS, the batched lookup step; row b * T + t): draw_addr.h's rule over
// the sequences' emission counts, which a kernel of that mode takes as one more argument (PickSeqs) -- the other two take none.
enum PickRows { PICK_ROWS_SEQS, PICK_ROWS_STEPS, PICK_ROWS_SEQ_STEPS };
struct PickDraw {
  unsigned long long ctr;
  int seq;
};
struct PickSeqs {
  const int* steps;  // device int [B]: ids every sequence has emitted; every block reads all B and takes the minimum itself
  int B, T;
};
template <PickRows MODE>
__device__ __forceinline__ PickDraw pick_draw(unsigned long long counter, int b) {
  static_assert(MODE != PICK_ROWS_SEQ_STEPS, "rows of several sequences are addressed over their counts");
  return MODE == PICK_ROWS_STEPS ? PickDraw{counter + (unsigned long long)b, 0} : PickDraw{counter, b};
}
template <PickRows MODE>
__device__ __forceinline__ PickDraw pick_draw(unsigned long long counter, int r, PickSeqs q) {
  static_assert(MODE == PICK_ROWS_SEQ_STEPS, "only rows of several sequences carry counts");
  const DrawAddr a = draw_addr(counter, q.steps, q.B, q.T, r);
  return PickDraw{a.ctr, a.seq};
}
// Gumbel-max: argmax_i (score_i + g_i), g_i = -log(-log(u_i)), u_i in (0, 1), is a draw from softmax(score).  The key of entry i of
// row b at step counter ctr (srgpt_sampling::counter / ::seed).  u = (n + 0.5) * 2^-24 over the 24 bits n = x >> 8; for n >= 2^23 the
// sum is no fp32 number and rounds half to even, and at n = 2^24 - 1 it rounds to 2^24: u = 1, g = +inf, the entry won whatever its
// score (2^-24 per entry and draw, one pure-temperature draw in 130 over 128258 entries).  The minimum keeps that one u at the
// largest fp32 below 1 and changes no other draw.  tests/draw_ref.py restates the key on the host, token for token.
__device__ __forceinline__ float pick_gumbel_key(float score, unsigned long long ctr, unsigned long long seed, int b, int i) {
  const U4 r = philox4x32_10(U4{(unsigned)ctr, (unsigned)(ctr >> 32), (unsigned)b, (unsigned)i}, (unsigned)seed, (unsigned)(seed >> 32));
  const float u = fminf(((float)(r.x >> 8) + 0.5f) * (1.0f / 16777216.0f), 0x1.fffffep-1f);
  return score - logf(-logf(u));
}
