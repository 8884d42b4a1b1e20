// Attention kernels.
//  1. flash_bf16_kernel  -- prefill / ViT: MFMA flash attention, in flash.hip (its own translation unit: it is compiled with
//     MFMA accumulators in arch VGPRs, this file is not); launched from srgpt_attention below.
//  2. simple_attn_kernel -- one wave per (query, head); any dtype / head_dim; fp32 parity path.
//  3. decode_split/combine -- single new token against the static KV cache, flash-decoding split over
//     keys, fused RoPE of the new q/k and cache append.  HBM/latency bound.
//  4. decode_mfma_multi  -- the same for T new tokens per sequence (prompt-lookup decoding): the drafted tokens' query heads in the
//     columns of the MFMA B operand the single-token kernel leaves empty.
#include <stdlib.h>

#include <type_traits>

#include "attn_route.h"
#include "common.h"
#include "internal.h"

namespace {

// ================================================================================================
// 2. simple attention: one wave per (query row, head)
// ================================================================================================
template <typename T>
__global__ __launch_bounds__(64) void simple_attn_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                         const T* __restrict__ v, T* __restrict__ o, int Tq, int Tk,
                                                         int Hq, int Hkv, int D, int64_t q_bs, int64_t q_ts,
                                                         int64_t q_hs, int64_t k_bs, int64_t k_ts, int64_t k_hs,
                                                         int64_t v_bs, int64_t v_ts, int64_t v_hs, float scale,
                                                         int causal, const int* __restrict__ kv_len,
                                                         const int* __restrict__ q_pos0) {
  __shared__ float qs[256];
  const int t = blockIdx.x, h = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  const int hk = h / (Hq / Hkv);
  const int klen = kv_len ? min(kv_len[b], Tk) : Tk;
  const T* qp = q + b * q_bs + (int64_t)t * q_ts + h * q_hs;
  for (int d = lane; d < D; d += 64) qs[d] = to_f(qp[d]);
  __syncthreads();
  const T* kb = k + b * k_bs + hk * k_hs;
  const T* vb = v + b * v_bs + hk * v_hs;
  // causal: query t sits at t + (Tk - Tq), or (srgpt_attention_append) at the row's own q_pos0[b] + t
  const int last = causal ? min(klen - 1, t + (q_pos0 ? q_pos0[b] : Tk - Tq)) : klen - 1;
  float m = -INFINITY, l = 0.f;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};  // d = lane + 64 * i, D <= 256
  for (int k0 = 0; k0 <= last; k0 += 64) {
    const int key = k0 + lane;
    float s = -INFINITY;
    if (key <= last) {
      const T* kr = kb + (int64_t)key * k_ts;
      float dot = 0.f;
      for (int d = 0; d < D; ++d) dot = fmaf(qs[d], to_f(kr[d]), dot);
      s = dot * scale;
    }
    const float m_new = fmaxf(m, wave_max(s));
    const float alpha = __expf(m - m_new);
    const float p = (key <= last) ? __expf(s - m_new) : 0.f;
    l = l * alpha + wave_sum(p);
    m = m_new;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] *= alpha;
    const int nk = min(64, last + 1 - k0);
    for (int j = 0; j < nk; ++j) {
      const float pj = __shfl(p, j);
      const T* vr = vb + (int64_t)(k0 + j) * v_ts;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int d = lane + 64 * i;
        if (d < D) acc[i] = fmaf(pj, to_f(vr[d]), acc[i]);
      }
    }
  }
  const float inv = l > 0.f ? 1.f / l : 0.f;
  T* op = o + (((int64_t)b * Tq + t) * Hq + h) * D;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = lane + 64 * i;
    if (d < D) op[d] = from_f<T>(acc[i] * inv);
  }
}

// ================================================================================================
// 3. decode attention: split over keys + combine
// ================================================================================================
constexpr int DEC_CHUNK_MAX = ATTN_DEC_CHUNK_MAX;  // attn_route.h: the routes, their thresholds and the workspace layout

typedef SrgptPrefetch DecodePrefetch;  // common.h: L2 prefetch blocks appended to the launch (here: o_proj's weights)

// Partials are published WRITE-THROUGH (agent-scope relaxed atomic stores = global_store ... sc1) and read back with agent-scope
// relaxed loads by whichever block of this (sequence, kv head) arrives last: no second launch for the merge.  One float, or a pair
// as one 8-byte store.  (A function object like the two lambdas it replaces: as a free function it renamed registers in
// decode_mfma_kernel<1> and <2>, profiles/NOTEBOOK.md.)
struct PublishPartial {
  __device__ void operator()(float* p, float v) const { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ void operator()(float* p, float a, float b) const {
    const unsigned long long u = (unsigned long long)__float_as_uint(a) | ((unsigned long long)__float_as_uint(b) << 32);
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// ---- the tail both decode kernels share: arrival ticket of the (sequence, kv head) group, merge by the last arriver ----
template <typename T, int D, int G, int SCLD>
__device__ __forceinline__ void decode_ticket_merge(float* __restrict__ wbase, int* __restrict__ ticket, int nsplit,
                                                    T* __restrict__ outp, float* __restrict__ sc, float* __restrict__ stat_m,
                                                    float* __restrict__ stat_l, int tid, int lane, int wave) {
  // ---- arrival ticket: every storing wave drains its write-through stores, one lane takes the ticket; the block that draws
  //      the last one merges the nsplit partials of its G query heads (fixed split order: the result does not depend on
  //      which block came last) and re-arms the ticket for the next launch on this stream ----
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    stat_l[0] = (t == nsplit - 1) ? 1.f : 0.f;  // stat_l is free again: broadcast "I am last" through the existing LDS
  }
  __syncthreads();
  if (stat_l[0] == 0.f) return;
  __syncthreads();
  // The first 16 splits' partials of this thread's pair of output dims AND the per-split statistics are requested back to
  // back: the merge pays one memory latency.  (G * D / 2 <= 256 * MAXW items; one or two per thread for the shipped shapes.)
  constexpr int PRE = 16;
  constexpr size_t HEAD = attn_ws_row(1, 0, D), ROW = attn_ws_row(0, 1, D);  // floats between two heads' rows, two splits' rows
  constexpr int MAXW = (G * (D / 2) + 255) / 256;
  unsigned long long v[MAXW][PRE];
#pragma unroll
  for (int wi = 0; wi < MAXW; ++wi) {
    const int w = min(tid + 256 * wi, G * (D / 2) - 1);
    const int gq = w / (D / 2), d = 2 * (w - gq * (D / 2));
    const float* wp = wbase + gq * HEAD + d;
#pragma unroll
    for (int j = 0; j < PRE; ++j)
      v[wi][j] = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(wp + min(j, nsplit - 1) * ROW),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // per-head merge weights: wave gq handles head gq (G <= 8 heads over 4 waves), one split per lane (nsplit <= 64)
  for (int gq = wave; gq < G; gq += 4) {
    const float* wp = wbase + gq * HEAD;
    const bool ok = lane < nsplit;
    const int sidx = ok ? lane : nsplit - 1;
    const unsigned long long ml = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(wp + sidx * ROW + D),
                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float ms_raw = __uint_as_float((unsigned)ml), ls_raw = __uint_as_float((unsigned)(ml >> 32));
    const float ms = ok ? ms_raw : -INFINITY;
    const float ls = ok ? ls_raw : 0.f;
    const float M = lanes_max<64>(ms);
    const float wv = (ms > -INFINITY) ? __expf(ms - M) : 0.f;
    const float den = lanes_sum<64>(wv * ls);
    sc[gq * SCLD + lane] = wv;
    if (lane == 0) stat_m[gq] = den > 0.f ? 1.f / den : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int wi = 0; wi < MAXW; ++wi) {
    const int w = tid + 256 * wi;
    if (w < G * (D / 2)) {
      const int gq = w / (D / 2), d = 2 * (w - gq * (D / 2));
      const float* wp = wbase + gq * HEAD + d;
      float n0 = 0.f, n1 = 0.f;
#pragma unroll
      for (int j = 0; j < PRE; ++j)
        if (j < nsplit) {
          n0 = fmaf(sc[gq * SCLD + j], __uint_as_float((unsigned)v[wi][j]), n0);
          n1 = fmaf(sc[gq * SCLD + j], __uint_as_float((unsigned)(v[wi][j] >> 32)), n1);
        }
      // long contexts (> 16 live splits = > 1024 keys on the MFMA kernel): the remaining partials in batches of 16 loads in flight,
      // consumed in split order -- the same fma chain as one load at a time (48 dependent L2 round trips at 4096 keys before)
      for (int s0 = PRE; s0 < nsplit; s0 += PRE) {
        unsigned long long u[PRE];
#pragma unroll
        for (int j = 0; j < PRE; ++j)
          u[j] = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(wp + min(s0 + j, nsplit - 1) * ROW),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int j = 0; j < PRE; ++j)
          if (s0 + j < nsplit) {
            n0 = fmaf(sc[gq * SCLD + s0 + j], __uint_as_float((unsigned)u[j]), n0);
            n1 = fmaf(sc[gq * SCLD + s0 + j], __uint_as_float((unsigned)(u[j] >> 32)), n1);
          }
      }
      T* op = outp + (size_t)gq * D + d;
      op[0] = from_f<T>(n0 * stat_m[gq]);
      op[1] = from_f<T>(n1 * stat_m[gq]);
    }
  }
  if (tid == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename T, int D, int G>
__global__ __launch_bounds__(256) void decode_split_kernel(const T* __restrict__ qkv, T* __restrict__ kcache,
                                                           T* __restrict__ vcache, const int* __restrict__ pos,
                                                           const T* __restrict__ cos_tab, const T* __restrict__ sin_tab,
                                                           float* __restrict__ ws, int* __restrict__ tickets,
                                                           T* __restrict__ out, int Hq, int Hkv, int max_pos,
                                                           int nsplit, float scale, int n_attn, DecodePrefetch pf) {
  constexpr int VEC = Vec16<T>::N;
  constexpr int LPK = D / VEC;   // lanes per key
  constexpr int KPW = 64 / LPK;  // keys per wave-instruction
  constexpr int HALF = D / 2;
  constexpr int STRIDE = 4 * KPW;  // keys per block iteration
  constexpr int PF = 2;            // key iterations whose K/V rows are fetched up front (3 and 4 measured: no difference)
  __shared__ float qs[G][D];
  __shared__ float knew[D], vnew[D];
  __shared__ float sc[G][DEC_CHUNK_MAX];
  __shared__ float red[4][G][D];
  __shared__ float stat_m[G], stat_l[G];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if ((int)blockIdx.x >= n_attn) {  // ---- prefetch block (common.h) ----
    srgpt_prefetch_block(pf, (int)blockIdx.x - n_attn, wave, lane);
    return;
  }
  const int hk = (int)blockIdx.x % Hkv, split = ((int)blockIdx.x / Hkv) % nsplit, b = (int)blockIdx.x / (Hkv * nsplit);
  const int P = pos[b];
  const int total = P + 1;
  // the key ranges depend on the sequence length only (NOT on the cache capacity: fixed capacity-based ranges were measured --
  // no faster -- and make the summation order, hence the bits, depend on how large a cache the caller happened to allocate)
  const int chunk = (total + nsplit - 1) / nsplit;
  const int kbeg = split * chunk, kend = min(kbeg + chunk, total);
  const T* row = qkv + (size_t)b * (Hq + 2 * Hkv) * D;
  T* kc = kcache + ((size_t)b * Hkv + hk) * (size_t)max_pos * D;
  T* vc = vcache + ((size_t)b * Hkv + hk) * (size_t)max_pos * D;
  const int sub = lane / LPK, dl = (lane % LPK) * VEC;
  const int key0 = kbeg + wave * KPW + sub;

  // ---- all cache rows of the first PF iterations go out before anything depends on q: one memory latency ----
  Vec16<T> kreg[PF], vreg[PF];
#pragma unroll
  for (int j = 0; j < PF; ++j) {
    const int key = key0 + j * STRIDE;
    if (key < kend && key != P) {
      kreg[j] = *reinterpret_cast<const Vec16<T>*>(kc + (size_t)key * D + dl);
      vreg[j] = *reinterpret_cast<const Vec16<T>*>(vc + (size_t)key * D + dl);
    }
  }

  // ---- rotate q (G heads) and the new k; stage v.  Every global load of this stage is issued before any of
  //      them is consumed (unrolled, index wrapped instead of branched): one L2 latency instead of three. ----
  {
    constexpr int NITEM = (G + 1) * HALF;
    constexpr int ITEMS = (NITEM + 255) / 256;
    float x1v[ITEMS], x2v[ITEMS], cv[ITEMS], sv[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const int w = (tid + 256 * it) % NITEM;
      const int hh = w / HALF, i = w - hh * HALF;
      const T* p = (hh < G) ? row + (size_t)(hk * G + hh) * D : row + (size_t)(Hq + hk) * D;
      x1v[it] = to_f(p[i]);
      x2v[it] = to_f(p[i + HALF]);
      cv[it] = to_f(cos_tab[(size_t)P * HALF + i]);
      sv[it] = to_f(sin_tab[(size_t)P * HALF + i]);
    }
    const float vraw = to_f(row[(size_t)(Hq + Hkv + hk) * D + (tid % D)]);
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const int w0 = tid + 256 * it;
      if (w0 < NITEM) {
        const int hh = w0 / HALF, i = w0 - hh * HALF;
        const float o1 = rnd<T>(rnd<T>(x1v[it] * cv[it]) + rnd<T>(-x2v[it] * sv[it]));
        const float o2 = rnd<T>(rnd<T>(x2v[it] * cv[it]) + rnd<T>(x1v[it] * sv[it]));
        if (hh < G) {
          qs[hh][i] = o1;
          qs[hh][i + HALF] = o2;
        } else {
          knew[i] = o1;
          knew[i + HALF] = o2;
        }
      }
    }
    if (tid < D) vnew[tid] = vraw;
  }
  __syncthreads();
  if (split == 0) {  // exactly one block per (b, hk) appends; nobody reads position P from the cache
    for (int d = tid; d < D; d += 256) {
      kc[(size_t)P * D + d] = from_f<T>(knew[d]);
      vc[(size_t)P * D + d] = from_f<T>(vnew[d]);
    }
  }

  float* wbase = ws + attn_ws_group(b, hk, Hkv, G, D);
  const PublishPartial publish;
  const bool empty = kbeg >= kend;
  if (empty) {  // empty split: neutral partial (zeros, m = -inf, l = 0)
    for (int w = tid; w < G * (D + 2); w += 256) {
      const int gq = w / (D + 2), d = w - gq * (D + 2);
      publish(wbase + attn_ws_row(gq, split, D) + d, (d == D) ? -INFINITY : 0.f);
    }
  }
  if (!empty) {

  // ---- pass 1: scores ----
  auto score = [&](int key, const float* kv) {
#pragma unroll
    for (int gq = 0; gq < G; ++gq) {
      float part = 0.f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) part = fmaf(kv[i], qs[gq][dl + i], part);
      part = lanes_sum<LPK>(part);  // DPP / permlane: a ds_bpermute chain here cost ~2k cycles per key batch
      if ((lane % LPK) == 0) sc[gq][key - kbeg] = part * scale;
    }
  };
#pragma unroll
  for (int j = 0; j < PF; ++j) {
    const int key = key0 + j * STRIDE;
    if (key < kend) {
      float kv[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) kv[i] = (key == P) ? knew[dl + i] : kreg[j].get(i);
      score(key, kv);
    }
  }
  for (int key = key0 + PF * STRIDE; key < kend; key += STRIDE) {
    float kv[VEC];
    if (key == P) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) kv[i] = knew[dl + i];
    } else {
      const Vec16<T> t = *reinterpret_cast<const Vec16<T>*>(kc + (size_t)key * D + dl);
#pragma unroll
      for (int i = 0; i < VEC; ++i) kv[i] = t.get(i);
    }
    score(key, kv);
  }
  __syncthreads();
  // ---- softmax statistics of the chunk, one wave per q head ----
  const int n = kend - kbeg;
  for (int gq = wave; gq < G; gq += 4) {
    float mx = -INFINITY;
    for (int i = lane; i < n; i += 64) mx = fmaxf(mx, sc[gq][i]);
    mx = lanes_max<64>(mx);
    float sum = 0.f;
    for (int i = lane; i < n; i += 64) {
      const float pv = __expf(sc[gq][i] - mx);
      sc[gq][i] = pv;
      sum += pv;
    }
    sum = lanes_sum<64>(sum);
    if (lane == 0) {
      stat_m[gq] = mx;
      stat_l[gq] = sum;
    }
  }
  __syncthreads();
  // ---- pass 2: O = P V ----
  float acc[G][VEC];
#pragma unroll
  for (int gq = 0; gq < G; ++gq)
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[gq][i] = 0.f;
  auto accum = [&](int key, const float* vv) {
#pragma unroll
    for (int gq = 0; gq < G; ++gq) {
      const float pg = sc[gq][key - kbeg];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[gq][i] = fmaf(pg, vv[i], acc[gq][i]);
    }
  };
#pragma unroll
  for (int j = 0; j < PF; ++j) {
    const int key = key0 + j * STRIDE;
    if (key < kend) {
      float vv[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) vv[i] = (key == P) ? vnew[dl + i] : vreg[j].get(i);
      accum(key, vv);
    }
  }
  for (int key = key0 + PF * STRIDE; key < kend; key += STRIDE) {
    float vv[VEC];
    if (key == P) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) vv[i] = vnew[dl + i];
    } else {
      const Vec16<T> t = *reinterpret_cast<const Vec16<T>*>(vc + (size_t)key * D + dl);
#pragma unroll
      for (int i = 0; i < VEC; ++i) vv[i] = t.get(i);
    }
    accum(key, vv);
  }
#pragma unroll
  for (int gq = 0; gq < G; ++gq)
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const float x = strided_sum<LPK>(acc[gq][i]);  // over the wave's KPW key sub-groups
      if (sub == 0) red[wave][gq][dl + i] = x;
    }
  __syncthreads();
  // 8-byte write-through stores (pairs of floats; rows of D + 2 floats are 8-byte aligned because D is even)
  for (int w = tid; w < G * (D / 2); w += 256) {
    const int gq = w / (D / 2), d = 2 * (w - gq * (D / 2));
    float* wp = wbase + attn_ws_row(gq, split, D);
    publish(wp + d, red[0][gq][d] + red[1][gq][d] + red[2][gq][d] + red[3][gq][d],
             red[0][gq][d + 1] + red[1][gq][d + 1] + red[2][gq][d + 1] + red[3][gq][d + 1]);
    if (d == 0) publish(wp + D, stat_m[gq], stat_l[gq]);
  }
  }  // !empty

  decode_ticket_merge<T, D, G, DEC_CHUNK_MAX>(wbase, attn_ws_ticket(tickets, b, hk, Hkv), nsplit,
                                              out + ((size_t)b * Hq + (size_t)hk * G) * D, &sc[0][0], stat_m, stat_l, tid, lane, wave);
}

// ------------------------------------------------------------------------------------------------
// decode attention, bf16 / head_dim 128 (every LLM geometry of the reference's recipes): round 3.
// The VALU kernel above spends ~10k of its ~23k cycles in three dependent-chain phases (scores with a cross-lane reduction per key
// and head, block-wide statistics, P.V with 32 cross-lane reductions per thread: profiles/r02_decode_attention_stamps.txt).  Here
//   * scores are ONE chain of four v_mfma_f32_16x16x32_bf16 per wave and 16 keys: A = K rows exactly as they lie in the cache
//     (lane = key, 16-byte d slices -- loaded straight from global in fragment shape), B = the G roped query heads (columns >= G
//     zero); the result leaves lane (head, key quad) with its 4 scores -- softmax statistics are two row swaps, no LDS, no barrier;
//   * P.V runs with lane = a pair of output dims over the wave's 16 keys (V rows as 256-byte wave loads, probabilities broadcast
//     from LDS): no cross-lane reduction at all;
//   * the four waves of a block (64 keys) meet once, through LDS, with per-wave (m, l) statistics -- one barrier;
// a block covers 64 keys (8 splits at <= 512 cached positions instead of 16): half as many partials for the merging block.
// All K / V row loads of a wave's first key group go out before anything depends on q.  Same partial format, ticket and merge.
// ------------------------------------------------------------------------------------------------
constexpr int DM_QLD = 136;  // bf16 row stride of the staged query heads (272 bytes: rows land on different bank groups)

template <int G>
__global__ __launch_bounds__(256) void decode_mfma_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kcache,
                                                          bf16_t* __restrict__ vcache, const int* __restrict__ pos,
                                                          const bf16_t* __restrict__ cos_tab, const bf16_t* __restrict__ sin_tab,
                                                          float* __restrict__ ws, int* __restrict__ tickets,
                                                          bf16_t* __restrict__ out, int Hq, int Hkv, int max_pos, int nsplit,
                                                          int kpb, float scale, int n_attn, DecodePrefetch pf) {
  typedef bf16_t T;
  constexpr int D = 128, HALF = 64;
  __shared__ __attribute__((aligned(16))) bf16_t qs[16 * DM_QLD];  // B operand source: rows = query heads (>= G: zero)
  __shared__ __attribute__((aligned(16))) bf16_t knew[D], vnew[D];
  __shared__ __attribute__((aligned(16))) float pw[4][16][G];      // a wave's probabilities [key][head]
  __shared__ __attribute__((aligned(16))) float accs[4][G][D];     // per-wave P.V
  __shared__ float wm[4][G], wl[4][G];
  __shared__ float sc[G][64];                                      // merge weights (decode_ticket_merge)
  __shared__ float stat_m[G], stat_l[G];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if ((int)blockIdx.x >= n_attn) {  // ---- prefetch block (common.h) ----
    srgpt_prefetch_block(pf, (int)blockIdx.x - n_attn, wave, lane);
    return;
  }
  const int hk = (int)blockIdx.x % Hkv, split = ((int)blockIdx.x / Hkv) % nsplit, b = (int)blockIdx.x / (Hkv * nsplit);
  const int P = pos[b];
  const int total = P + 1;
  // FIXED key ranges: block `split` owns keys [split * kpb, (split + 1) * kpb), kpb = 64 for caches up to 4096 positions -- the
  // partition, hence the summation order and the bits, depend on the sequence length only, never on how large a cache the caller
  // happened to allocate (a pooled state serves requests of different sizes: scripts/soak.py caught exactly that); splits past the
  // sequence publish the neutral partial, which the merge adds as exact zeros
  const int kbeg = split * kpb, kend = min(kbeg + kpb, total);
  // Only the first ceil(total / kpb) splits own keys.  The blocks behind them leave at once -- no fetch, no RoPE, no partial, no
  // ticket: a state pooled for a long request (or max_length = 4096 out of a generation_config.json) costs a short request nothing
  // (ADVICE r3).  The merge covers the `nlive` partials only; the neutral partials the dead splits used to publish entered it as
  // exact zeros (weight exp(-inf) = 0), so the bits are the ones of the all-splits merge and stay independent of the capacity.
  const int nlive = min(nsplit, (total + kpb - 1) / kpb);
  if (split >= nlive) return;  // uniform per block
  const T* row = qkv + (size_t)b * (Hq + 2 * Hkv) * D;
  T* kc = kcache + ((size_t)b * Hkv + hk) * (size_t)max_pos * D;
  T* vc = vcache + ((size_t)b * Hkv + hk) * (size_t)max_pos * D;
  const int lq = lane & 15, g4 = lane >> 4;
  const int lastrow = max(P - 1, 0);  // rows >= P are not in the cache yet (row P is written by the split-0 block of THIS launch)

  // ---- K rows (fragment shape) and V rows (256-byte wave loads) of the wave's first 16-key group: one memory latency ----
  u32x4 kreg[4];
  unsigned int vreg[16];
  auto fetch = [&](int kb) {
    const T* kr = kc + (size_t)min(kb + lq, lastrow) * D + g4 * 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) kreg[j] = *reinterpret_cast<const u32x4*>(kr + 32 * j);
#pragma unroll
    for (int i = 0; i < 16; ++i)
      vreg[i] = *reinterpret_cast<const unsigned int*>(vc + (size_t)min(kb + i, lastrow) * D + 2 * lane);
  };
  int kb = kbeg + 16 * wave;
  fetch(kb);

  // ---- rotate q (G heads) and the new k; stage v.  Every global load of this stage is issued before any is consumed ----
  {
    constexpr int NITEM = (G + 1) * HALF;
    constexpr int ITEMS = (NITEM + 255) / 256;
    float x1v[ITEMS], x2v[ITEMS], cv[ITEMS], sv[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const int w = (tid + 256 * it) % NITEM;
      const int hh = w / HALF, i = w - hh * HALF;
      const T* p = (hh < G) ? row + (size_t)(hk * G + hh) * D : row + (size_t)(Hq + hk) * D;
      x1v[it] = to_f(p[i]);
      x2v[it] = to_f(p[i + HALF]);
      cv[it] = to_f(cos_tab[(size_t)P * HALF + i]);
      sv[it] = to_f(sin_tab[(size_t)P * HALF + i]);
    }
    const T vraw = row[(size_t)(Hq + Hkv + hk) * D + (tid % D)];
    // query rows G .. 15 of the B operand are zero
    for (int i = tid; i < (16 - G) * (D / 2); i += 256) {
      const int r = G + i / (D / 2), c = 2 * (i % (D / 2));
      *reinterpret_cast<unsigned int*>(qs + r * DM_QLD + c) = 0u;
    }
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const int w0 = tid + 256 * it;
      if (w0 < NITEM) {
        const int hh = w0 / HALF, i = w0 - hh * HALF;
        const T o1 = from_f<T>(rnd<T>(x1v[it] * cv[it]) + rnd<T>(-x2v[it] * sv[it]));
        const T o2 = from_f<T>(rnd<T>(x2v[it] * cv[it]) + rnd<T>(x1v[it] * sv[it]));
        if (hh < G) {
          qs[hh * DM_QLD + i] = o1;
          qs[hh * DM_QLD + i + HALF] = o2;
        } else {
          knew[i] = o1;
          knew[i + HALF] = o2;
        }
      }
    }
    if (tid < D) vnew[tid] = vraw;
  }
  __syncthreads();
  if (split == 0) {  // exactly one block per (b, hk) appends; nobody reads position P from the cache
    if (tid < D / 2) {
      *reinterpret_cast<unsigned int*>(kc + (size_t)P * D + 2 * tid) = *reinterpret_cast<const unsigned int*>(knew + 2 * tid);
      *reinterpret_cast<unsigned int*>(vc + (size_t)P * D + 2 * tid) = *reinterpret_cast<const unsigned int*>(vnew + 2 * tid);
    }
  }
  // B operand: lane (head lq, d slice g4) -- the same four fragments for every key group
  bf16x8 qf[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) qf[j] = *reinterpret_cast<const bf16x8*>(qs + lq * DM_QLD + 32 * j + g4 * 8);
  u32x4 knf[4];  // the new key in fragment shape (for the lane whose key is P)
#pragma unroll
  for (int j = 0; j < 4; ++j) knf[j] = *reinterpret_cast<const u32x4*>(knew + 32 * j + g4 * 8);
  const unsigned int vnw = *reinterpret_cast<const unsigned int*>(vnew + 2 * lane);

  float m_run = -INFINITY, l_run = 0.f;  // per column (head lq): identical in the four lanes of a column
  float acc[G][2];
#pragma unroll
  for (int h = 0; h < G; ++h) acc[h][0] = acc[h][1] = 0.f;

  for (; kb < kend; kb += 64) {
    // ---- S^T = K Q^T: lane (head lq, quad g4) ends with the scores of keys kb + 4 g4 + r ----
    f32x4 sacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      u32x4 kv = kreg[j];
      if (kb + lq == P) kv = knf[j];
      sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kv), qf[j], sacc, 0, 0, 0);
    }
    float sv4[4], mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = kb + 4 * g4 + r;
      sv4[r] = key < kend ? sacc[r] * scale : -INFINITY;
      mx = fmaxf(mx, sv4[r]);
    }
    mx = rows_pair(mx, [](float a, float b2) { return fmaxf(a, b2); });
    mx = halves_pair(mx, [](float a, float b2) { return fmaxf(a, b2); });
    const float m_new = fmaxf(m_run, mx);  // kb < kend: at least one valid key, m_new is finite
    const float alpha = __expf(m_run - m_new);  // first group: exp(-inf) = 0
    float rs = 0.f;
    f32x4 pv;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pv[r] = __expf(sv4[r] - m_new);
      rs += pv[r];
    }
    rs = rows_pair(rs, [](float a, float b2) { return a + b2; });
    rs = halves_pair(rs, [](float a, float b2) { return a + b2; });
    l_run = l_run * alpha + rs;
    m_run = m_new;
    // probabilities -> LDS [key][head] (a wave's own slab: in-order DS ops of ONE wave, no block barrier)
    if (lq < G) {
#pragma unroll
      for (int r = 0; r < 4; ++r) pw[wave][4 * g4 + r][lq] = pv[r];
    }
    // the rescale factor of the running P.V is per head: broadcast it the same way
    if (lq < G && g4 == 0) wm[wave][lq] = alpha;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int h = 0; h < G; ++h) {
      const float a_h = wm[wave][h];
      acc[h][0] *= a_h;
      acc[h][1] *= a_h;
    }
    // ---- P V: lane = output dims (2 lane, 2 lane + 1) ----
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int key = kb + i;
      unsigned int vv = vreg[i];
      if (key == P) vv = vnw;
      if (key >= kend) vv = 0u;  // clamped rows may hold anything (0 * NaN)
      const float v0 = bf16lo(vv), v1 = bf16hi(vv);
#pragma unroll
      for (int h = 0; h < G; ++h) {
        const float ph = pw[wave][i][h];
        acc[h][0] = fmaf(ph, v0, acc[h][0]);
        acc[h][1] = fmaf(ph, v1, acc[h][1]);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if (kb + 64 < kend) fetch(kb + 64);  // contexts beyond 64 keys per split (max_pos > 64 * ATTN_DEC_SPLIT_MAX never; > 512 here)
  }
  // ---- the four waves meet: per-wave (m, l) and P.V through LDS ----
  if (lq < G && g4 == 0) {
    wm[wave][lq] = m_run;
    wl[wave][lq] = l_run;
  }
#pragma unroll
  for (int h = 0; h < G; ++h) *reinterpret_cast<f32x2*>(&accs[wave][h][2 * lane]) = f32x2{acc[h][0], acc[h][1]};
  __syncthreads();
  float* wbase = ws + attn_ws_group(b, hk, Hkv, G, D);
  const PublishPartial publish;
  for (int w = tid; w < G * (D / 2); w += 256) {
    const int gq = w / (D / 2), d = 2 * (w - gq * (D / 2));
    const float M = fmaxf(fmaxf(wm[0][gq], wm[1][gq]), fmaxf(wm[2][gq], wm[3][gq]));
    float n0 = 0.f, n1 = 0.f, L = 0.f;
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) {  // fixed wave order
      const float e = (wm[wv][gq] > -INFINITY) ? __expf(wm[wv][gq] - M) : 0.f;
      n0 = fmaf(e, accs[wv][gq][d], n0);
      n1 = fmaf(e, accs[wv][gq][d + 1], n1);
      L = fmaf(e, wl[wv][gq], L);
    }
    float* wp = wbase + attn_ws_row(gq, split, D);
    publish(wp + d, n0, n1);
    if (d == 0) publish(wp + D, M, L);
  }
  decode_ticket_merge<T, D, G, 64>(wbase, attn_ws_ticket(tickets, b, hk, Hkv), nlive, out + ((size_t)b * Hq + (size_t)hk * G) * D,
                                   &sc[0][0], stat_m, stat_l, tid, lane, wave);
}

// ------------------------------------------------------------------------------------------------
// decode attention for T new tokens per sequence (srgpt_decode_attention_multi): the next token and T - 1 drafted ones ride through
// ONE pass over the cache.  decode_mfma_kernel multiplies against a 16-column B operand of which G columns are live; here column
// c = t * G + g holds query head g of token t (T * G <= 16), token t sits at position P + t and sees the keys s <= P + t.  The T new
// k / v rows are roped into LDS, appended by the split-0 block and read from LDS by every block -- never back from the cache.
// Every column runs decode_mfma_kernel's arithmetic for ITS position, operation for operation: the same fixed key ranges, the same
// per-wave online softmax, the same wave and split merges -- so row t equals what srgpt_decode_attention answers at position P + t
// over a cache that holds rows P .. P + t - 1 (tests/test_gpu_attention_multi.py, bit for bit).  What the single-token kernel never
// meets: a column that sees NO key of a 16-key group, of a wave or of a whole split (the keys behind its own position).  Such a group
// leaves the column's running (m, l, P.V) untouched -- rescale 1, probabilities 0, no exp(-inf - -inf) --, such a wave or split
// publishes the neutral partial (m = -inf, l = 0, zeros), which both merges add as exact zeros, as they do for a short sequence.
// Rows at or beyond max_pos are neither appended nor attended (their columns are dead); a sequence whose pos lies outside the cache
// leaves at once.
// ------------------------------------------------------------------------------------------------
constexpr int DMM_C = ATTN_DEC_MULTI_COLS;

// decode_ticket_merge for a runtime number of columns: column c of the group -> out row (token c / G, head hk * G + c % G).  The same
// weights, the same fma chain in split order, the same rounding.
__device__ __forceinline__ void decode_multi_ticket_merge(float* __restrict__ wbase, int* __restrict__ ticket, int nsplit, int ncol,
                                                          int G, bf16_t* __restrict__ outp, size_t tok_stride, float* __restrict__ sc,
                                                          float* __restrict__ stat_m, float* __restrict__ stat_l, int tid, int lane,
                                                          int wave) {
  constexpr int D = 128, PRE = 16;
  constexpr size_t HEAD = attn_ws_row(1, 0, D), ROW = attn_ws_row(0, 1, D);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    stat_l[0] = (t == nsplit - 1) ? 1.f : 0.f;
  }
  __syncthreads();
  if (stat_l[0] == 0.f) return;
  __syncthreads();
  for (int c = wave; c < ncol; c += 4) {  // per-column merge weights: one split per lane
    const float* wp = wbase + c * HEAD;
    const bool ok = lane < nsplit;
    const int sidx = ok ? lane : nsplit - 1;
    const unsigned long long ml = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(wp + sidx * ROW + D),
                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float ms_raw = __uint_as_float((unsigned)ml), ls_raw = __uint_as_float((unsigned)(ml >> 32));
    const float ms = ok ? ms_raw : -INFINITY;
    const float ls = ok ? ls_raw : 0.f;
    const float M = lanes_max<64>(ms);
    const float wv = (ms > -INFINITY) ? __expf(ms - M) : 0.f;
    const float den = lanes_sum<64>(wv * ls);
    sc[c * 64 + lane] = wv;
    if (lane == 0) stat_m[c] = den > 0.f ? 1.f / den : 0.f;
  }
  __syncthreads();
  for (int w = tid; w < ncol * (D / 2); w += 256) {
    const int c = w / (D / 2), d = 2 * (w - c * (D / 2));
    const float* wp = wbase + c * HEAD + d;
    float n0 = 0.f, n1 = 0.f;
    for (int s0 = 0; s0 < nsplit; s0 += PRE) {  // 16 loads in flight, consumed in split order
      unsigned long long u[PRE];
#pragma unroll
      for (int j = 0; j < PRE; ++j)
        u[j] = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(wp + min(s0 + j, nsplit - 1) * ROW), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int j = 0; j < PRE; ++j)
        if (s0 + j < nsplit) {
          n0 = fmaf(sc[c * 64 + s0 + j], __uint_as_float((unsigned)u[j]), n0);
          n1 = fmaf(sc[c * 64 + s0 + j], __uint_as_float((unsigned)(u[j] >> 32)), n1);
        }
    }
    bf16_t* op = outp + (size_t)(c / G) * tok_stride + (size_t)(c % G) * D + d;
    op[0] = from_f<bf16_t>(n0 * stat_m[c]);
    op[1] = from_f<bf16_t>(n1 * stat_m[c]);
  }
  if (tid == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// NC: the live columns rounded up to 2 / 4 / 8 / 16 -- what sizes the per-column registers and LDS.  The columns in [T * G, NC) are
// dead: zero queries, no visible key, nothing published.  (The column count as a RUNTIME bound inside the unrolled P.V loops made
// the compiler predicate 512 fma and spill 12 000 registers: 400 us per launch.  G only enters index arithmetic: a runtime value.)
template <int NC>
__global__ __launch_bounds__(256) void decode_mfma_multi_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kcache,
                                                                bf16_t* __restrict__ vcache, const int* __restrict__ pos,
                                                                const bf16_t* __restrict__ cos_tab, const bf16_t* __restrict__ sin_tab,
                                                                float* __restrict__ ws, int* __restrict__ tickets,
                                                                bf16_t* __restrict__ out, int T, int G, int Hq, int Hkv,
                                                                int max_pos, int nsplit, int kpb, float scale) {
  typedef bf16_t Tb;
  constexpr int D = 128, HALF = 64;
  __shared__ __attribute__((aligned(16))) bf16_t qs[DMM_C * DM_QLD];      // B operand source: rows = columns (dead ones zero)
  __shared__ __attribute__((aligned(16))) bf16_t knew[DMM_C][D], vnew[DMM_C][D];  // the new rows, by token
  __shared__ __attribute__((aligned(16))) float pw[4][16][NC];            // a wave's probabilities [key][column]
  __shared__ __attribute__((aligned(16))) float accs[4][NC][D];           // per-wave P.V
  __shared__ float wm[4][NC], wl[4][NC];
  __shared__ float sc[NC * 64];                                           // merge weights
  __shared__ float stat_m[NC < 4 ? 4 : NC], stat_l[NC < 4 ? 4 : NC];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hk = (int)blockIdx.x % Hkv, split = ((int)blockIdx.x / Hkv) % nsplit, b = (int)blockIdx.x / (Hkv * nsplit);
  const int P = pos[b];
  if (P < 0 || P >= max_pos) return;  // nothing of this sequence lies inside the cache (uniform over its blocks: no ticket is drawn)
  const int Tv = min(T, max_pos - P);  // tokens whose rows exist: the others are neither appended nor attended
  const int ncol = Tv * G, total = P + Tv;
  const int kbeg = split * kpb, kend = min(kbeg + kpb, total);  // the keys ANY column of this block sees
  const int nlive = min(nsplit, (total + kpb - 1) / kpb);
  if (split >= nlive) return;  // uniform per block
  const size_t QW = (size_t)(Hq + 2 * Hkv) * D;
  const Tb* rows = qkv + (size_t)b * T * QW;
  Tb* kc = kcache + ((size_t)b * Hkv + hk) * (size_t)max_pos * D;
  Tb* vc = vcache + ((size_t)b * Hkv + hk) * (size_t)max_pos * D;
  const int lq = lane & 15, g4 = lane >> 4;
  const int lastrow = max(P - 1, 0);  // rows >= P are not in the cache yet
  // this lane's column: token lq / G at position P + lq / G sees the keys below kend_c (0: a dead column)
  const int kend_c = lq < ncol ? min(kbeg + kpb, P + lq / G + 1) : 0;

  u32x4 kreg[4];
  unsigned int vreg[16];
  auto fetch = [&](int kb) {
    const Tb* kr = kc + (size_t)min(kb + lq, lastrow) * D + g4 * 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) kreg[j] = *reinterpret_cast<const u32x4*>(kr + 32 * j);
#pragma unroll
    for (int i = 0; i < 16; ++i)
      vreg[i] = *reinterpret_cast<const unsigned int*>(vc + (size_t)min(kb + i, lastrow) * D + 2 * lane);
  };
  int kb = kbeg + 16 * wave;
  fetch(kb);

  // ---- rotate the Tv * G query heads and the Tv new keys at their own positions; stage v ----
  for (int i = tid; i < (DMM_C - ncol) * (D / 2); i += 256) {  // dead columns of the B operand are zero
    const int r = ncol + i / (D / 2), c = 2 * (i % (D / 2));
    *reinterpret_cast<unsigned int*>(qs + r * DM_QLD + c) = 0u;
  }
  for (int w = tid; w < Tv * (G + 1) * HALF; w += 256) {
    const int t = w / ((G + 1) * HALF), r = w - t * (G + 1) * HALF;
    const int hh = r / HALF, i = r - hh * HALF;
    const Tb* row = rows + (size_t)t * QW;
    const Tb* p = (hh < G) ? row + (size_t)(hk * G + hh) * D : row + (size_t)(Hq + hk) * D;
    const float x1 = to_f(p[i]), x2 = to_f(p[i + HALF]);
    const float cv = to_f(cos_tab[(size_t)(P + t) * HALF + i]), sv = to_f(sin_tab[(size_t)(P + t) * HALF + i]);
    const Tb o1 = from_f<Tb>(rnd<Tb>(x1 * cv) + rnd<Tb>(-x2 * sv));
    const Tb o2 = from_f<Tb>(rnd<Tb>(x2 * cv) + rnd<Tb>(x1 * sv));
    if (hh < G) {
      qs[(t * G + hh) * DM_QLD + i] = o1;
      qs[(t * G + hh) * DM_QLD + i + HALF] = o2;
    } else {
      knew[t][i] = o1;
      knew[t][i + HALF] = o2;
    }
  }
  for (int w = tid; w < Tv * D; w += 256) {
    const int t = w / D, i = w - t * D;
    vnew[t][i] = rows[(size_t)t * QW + (size_t)(Hq + Hkv + hk) * D + i];
  }
  __syncthreads();
  if (split == 0) {  // exactly one block per (b, hk) appends rows P .. P + Tv - 1 (all below max_pos)
    for (int w = tid; w < Tv * (D / 2); w += 256) {
      const int t = w / (D / 2), i = w - t * (D / 2);
      *reinterpret_cast<unsigned int*>(kc + (size_t)(P + t) * D + 2 * i) = *reinterpret_cast<const unsigned int*>(&knew[t][2 * i]);
      *reinterpret_cast<unsigned int*>(vc + (size_t)(P + t) * D + 2 * i) = *reinterpret_cast<const unsigned int*>(&vnew[t][2 * i]);
    }
  }
  bf16x8 qf[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) qf[j] = *reinterpret_cast<const bf16x8*>(qs + lq * DM_QLD + 32 * j + g4 * 8);

  float m_run = -INFINITY, l_run = 0.f;  // per column: identical in the four lanes of a column
  float acc[NC][2];
#pragma unroll
  for (int h = 0; h < NC; ++h) acc[h][0] = acc[h][1] = 0.f;

  for (; kb < kend; kb += 64) {
    // ---- S^T = K Q^T: lane (column lq, quad g4) ends with the scores of keys kb + 4 g4 + r ----
    f32x4 sacc = {0.f, 0.f, 0.f, 0.f};
    const int nk = kb + lq - P;  // >= 0: this lane's key row is new row nk (it exists where nk < Tv)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      u32x4 kv = kreg[j];
      if (nk >= 0) kv = *reinterpret_cast<const u32x4*>(&knew[min(nk, Tv - 1)][32 * j + g4 * 8]);
      sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kv), qf[j], sacc, 0, 0, 0);
    }
    const bool live = kb < kend_c;  // this column sees at least the group's first key
    float sv4[4], mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = kb + 4 * g4 + r;
      sv4[r] = key < kend_c ? sacc[r] * scale : -INFINITY;
      mx = fmaxf(mx, sv4[r]);
    }
    mx = rows_pair(mx, [](float a, float b2) { return fmaxf(a, b2); });
    mx = halves_pair(mx, [](float a, float b2) { return fmaxf(a, b2); });
    const float m_new = fmaxf(m_run, mx);  // live: finite; else m_run, possibly still -inf
    const float alpha = live ? __expf(m_run - m_new) : 1.f;  // a group without a visible key rescales nothing
    float rs = 0.f;
    f32x4 pv;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pv[r] = live ? __expf(sv4[r] - m_new) : 0.f;
      rs += pv[r];
    }
    rs = rows_pair(rs, [](float a, float b2) { return a + b2; });
    rs = halves_pair(rs, [](float a, float b2) { return a + b2; });
    l_run = l_run * alpha + rs;
    m_run = m_new;
    if (lq < NC) {  // a dead column's probabilities are zeros, its rescale 1
#pragma unroll
      for (int r = 0; r < 4; ++r) pw[wave][4 * g4 + r][lq] = pv[r];
    }
    if (lq < NC && g4 == 0) wm[wave][lq] = alpha;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int h = 0; h < NC; ++h) {
      const float a_h = wm[wave][h];
      acc[h][0] *= a_h;
      acc[h][1] *= a_h;
    }
    // ---- P V: lane = output dims (2 lane, 2 lane + 1) ----
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int key = kb + i;
      unsigned int vv = vreg[i];
      if (key >= P) vv = *reinterpret_cast<const unsigned int*>(&vnew[min(key - P, Tv - 1)][2 * lane]);
      if (key >= kend) vv = 0u;  // clamped rows may hold anything (0 * NaN)
      const float v0 = bf16lo(vv), v1 = bf16hi(vv);
#pragma unroll
      for (int h = 0; h < NC; ++h) {
        const float ph = pw[wave][i][h];
        acc[h][0] = fmaf(ph, v0, acc[h][0]);
        acc[h][1] = fmaf(ph, v1, acc[h][1]);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if (kb + 64 < kend) fetch(kb + 64);
  }
  // ---- the four waves meet: per-wave (m, l) and P.V through LDS ----
  if (lq < NC && g4 == 0) {
    wm[wave][lq] = m_run;
    wl[wave][lq] = l_run;
  }
#pragma unroll
  for (int h = 0; h < NC; ++h) *reinterpret_cast<f32x2*>(&accs[wave][h][2 * lane]) = f32x2{acc[h][0], acc[h][1]};
  __syncthreads();
  float* wbase = ws + attn_ws_group(b, hk, Hkv, T * G, D);
  const PublishPartial publish;
  for (int w = tid; w < ncol * (D / 2); w += 256) {
    const int gq = w / (D / 2), d = 2 * (w - gq * (D / 2));
    const float M = fmaxf(fmaxf(wm[0][gq], wm[1][gq]), fmaxf(wm[2][gq], wm[3][gq]));
    float n0 = 0.f, n1 = 0.f, L = 0.f;
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) {  // fixed wave order
      const float e = (wm[wv][gq] > -INFINITY) ? __expf(wm[wv][gq] - M) : 0.f;
      n0 = fmaf(e, accs[wv][gq][d], n0);
      n1 = fmaf(e, accs[wv][gq][d + 1], n1);
      L = fmaf(e, wl[wv][gq], L);
    }
    float* wp = wbase + attn_ws_row(gq, split, D);
    publish(wp + d, n0, n1);
    if (d == 0) publish(wp + D, M, L);
  }
  decode_multi_ticket_merge(wbase, attn_ws_ticket(tickets, b, hk, Hkv), nlive, ncol, G, out + ((size_t)b * T * Hq + (size_t)hk * G) * D,
                               (size_t)Hq * D, sc, stat_m, stat_l, tid, lane, wave);
}

// the RoPE / append launch of the composed route: rope_kv_append_kernel's arithmetic (misc.hip) with the row guard of
// srgpt_decode_attention_multi -- a token whose position lies outside the cache is neither rotated nor appended
template <typename T>
__global__ void rope_kv_append_guarded_kernel(T* __restrict__ qkv, T* __restrict__ kcache, T* __restrict__ vcache,
                                              const int* __restrict__ pos0, const T* __restrict__ cos_tab,
                                              const T* __restrict__ sin_tab, int Tn, int Hq, int Hkv, int D, int max_pos) {
  const int t = blockIdx.x, b = blockIdx.y;
  const int half = D >> 1;
  const int p0 = pos0[b];
  if (p0 < 0 || p0 >= max_pos || p0 + t >= max_pos) return;
  const int pos = p0 + t;
  T* row = qkv + ((size_t)b * Tn + t) * (size_t)(Hq + 2 * Hkv) * D;
  const int nrot = (Hq + Hkv) * half;
  for (int w = threadIdx.x; w < nrot; w += blockDim.x) {
    const int h = w / half, i = w - h * half;
    const float c = to_f(cos_tab[(size_t)pos * half + i]), s = to_f(sin_tab[(size_t)pos * half + i]);
    T* p = row + (size_t)h * D;
    const float x1 = to_f(p[i]), x2 = to_f(p[i + half]);
    const float o1 = rnd<T>(rnd<T>(x1 * c) + rnd<T>(-x2 * s));
    const float o2 = rnd<T>(rnd<T>(x2 * c) + rnd<T>(x1 * s));
    if (h < Hq) {
      p[i] = from_f<T>(o1);
      p[i + half] = from_f<T>(o2);
    } else {
      T* kc = kcache + (((size_t)b * Hkv + (h - Hq)) * max_pos + pos) * D;
      kc[i] = from_f<T>(o1);
      kc[i + half] = from_f<T>(o2);
    }
  }
  const T* vsrc = row + (size_t)(Hq + Hkv) * D;
  for (int w = threadIdx.x; w < Hkv * D; w += blockDim.x) {
    const int h = w / D, i = w - h * D;
    vcache[(((size_t)b * Hkv + h) * max_pos + pos) * D + i] = vsrc[w];
  }
}

// validated arguments -> the route (attn_route.h) -> its refusal, or the one launch of its template instance
template <typename T>
int launch_decode(const void* qkv, void* kc, void* vc, const int* pos, const void* ct, const void* st, void* out,
                  float* ws, int B, int Hq, int Hkv, int D, int max_pos, const DecodePrefetch& pf, hipStream_t s) {
  const AttnDecodeRoute r = attn_decode_route(std::is_same<T, bf16_t>::value, B, Hq, Hkv, D, max_pos, srgpt_device_cus());
  SRGPT_CHECK(r.status != ATTN_MAX_POS_TOO_LONG, SRGPT_ERR_UNSUPPORTED, "srgpt_decode_attention: max_pos %d exceeds %d cached positions",
              max_pos, ATTN_DEC_SPLIT_MAX * ATTN_DEC_CHUNK_MAX);
  SRGPT_CHECK(r.status != ATTN_BAD_HEAD_DIM, SRGPT_ERR_UNSUPPORTED, "srgpt_decode_attention: head_dim %d not supported (16,32,64,128)", D);
  SRGPT_CHECK(r.status != ATTN_BAD_GROUP, SRGPT_ERR_UNSUPPORTED, "srgpt_decode_attention: heads/kv_heads = %d not supported (1,2,4,8)",
              r.G);
  const float scale = 1.0f / sqrtf((float)D);
  int* tickets = reinterpret_cast<int*>(ws + attn_ws_partial_floats(B, Hq, D));
  const dim3 grid(r.n_attn + (pf.base ? pf.nblocks : 0)), block(256);
  int rc = SRGPT_OK;
  if constexpr (std::is_same<T, bf16_t>::value) {
    if (r.family == ATTN_DECODE_MFMA)
      rc = srgpt_switch<1, 2, 4, 8>(r.G, "heads/kv_heads", [&](auto g_c) {
        hipLaunchKernelGGL((decode_mfma_kernel<decltype(g_c)::value>), grid, block, 0, s, (const T*)qkv, (T*)kc, (T*)vc, pos,
                           (const T*)ct, (const T*)st, ws, tickets, (T*)out, Hq, Hkv, max_pos, r.nsplit, r.kpb, scale, r.n_attn, pf);
        return (int)SRGPT_OK;
      });
  }
  if (r.family == ATTN_DECODE_VALU)
    rc = srgpt_switch<16, 32, 64, 128>(D, "head_dim", [&](auto d_c) {
      return srgpt_switch<1, 2, 4, 8>(r.G, "heads/kv_heads", [&](auto g_c) {
        hipLaunchKernelGGL((decode_split_kernel<T, decltype(d_c)::value, decltype(g_c)::value>), grid, block, 0, s, (const T*)qkv,
                           (T*)kc, (T*)vc, pos, (const T*)ct, (const T*)st, ws, tickets, (T*)out, Hq, Hkv, max_pos, r.nsplit, scale,
                           r.n_attn, pf);
        return (int)SRGPT_OK;
      });
    });
  SRGPT_TRY(rc);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

}  // namespace

extern "C" int64_t srgpt_decode_attn_ws_floats(int B, int Hq, int D) {
  return (int64_t)attn_ws_floats(B, Hq, D);  // partials + arrival tickets (attn_route.h)
}

// internal entry (model.hip): decode attention + L2 prefetch of the weight matrix the next GEMV streams.
// next_w = NULL -> no prefetch.  batch > 1 goes through the skinny kernel: no prefetch there (measured, common.h).
int srgpt_decode_attention_pf(const void* qkv, void* kcache, void* vcache, const int* pos, const void* cos_tab,
                              const void* sin_tab, void* out, float* ws, int B, int Hq, int Hkv, int D, int max_pos, int dtype,
                              const void* next_w, int next_n, int next_k, int next_fp8, srgpt_stream_t stream) {
  SRGPT_CHECK(qkv && kcache && vcache && pos && cos_tab && sin_tab && out && ws, SRGPT_ERR_ARG,
              "srgpt_decode_attention: null pointer");
  SRGPT_CHECK(B > 0 && Hq > 0 && Hkv > 0 && Hq % Hkv == 0, SRGPT_ERR_ARG, "srgpt_decode_attention: bad heads");
  // bf16 activations only.  B > 1 gets no prefetch blocks (common.h); o_proj's packed tiles pulled by this launch were measured without
  // gain (profiles/r06_decode_prefetch_tiles.txt)
  const DecodePrefetch pf = srgpt_prefetch_for_gemv(dtype == SRGPT_BF16 ? next_w : nullptr, next_n, next_k, next_fp8, B);
  if (dtype == SRGPT_BF16)
    return launch_decode<bf16_t>(qkv, kcache, vcache, pos, cos_tab, sin_tab, out, ws, B, Hq, Hkv, D, max_pos, pf,
                                 as_stream(stream));
  if (dtype == SRGPT_F32)
    return launch_decode<float>(qkv, kcache, vcache, pos, cos_tab, sin_tab, out, ws, B, Hq, Hkv, D, max_pos, pf,
                                as_stream(stream));
  srgpt_set_error("srgpt_decode_attention: bad dtype %d", dtype);
  return SRGPT_ERR_ARG;
}

// the arrival tickets behind the partials (internal; model.hip zeroes them in every prefill so that a state whose workspace was
// never zeroed, or whose last launch was aborted, heals -- ADVICE r2 -- and srgpt_llm_decode_sync_state reads them back)
void* srgpt_decode_attn_sync_words(float* ws, int B, int Hq, int D, size_t* bytes) {
  if (bytes) *bytes = attn_ws_tickets_reserved(B, Hq) * sizeof(int);
  return ws + attn_ws_partial_floats(B, Hq, D);
}

extern "C" int srgpt_decode_attention(const void* qkv, void* kcache, void* vcache, const int* pos, const void* cos_tab,
                                      const void* sin_tab, void* out, float* ws, int B, int Hq, int Hkv, int D,
                                      int max_pos, int dtype, srgpt_stream_t stream) {
  return srgpt_decode_attention_pf(qkv, kcache, vcache, pos, cos_tab, sin_tab, out, ws, B, Hq, Hkv, D, max_pos, dtype, nullptr, 0,
                                   0, 0, stream);
}

extern "C" int64_t srgpt_decode_attn_multi_ws_floats(int B, int T, int Hq, int D) {
  return (int64_t)attn_multi_ws_floats(B, T, Hq, D);  // T * Hq columns' partials + arrival tickets (attn_route.h)
}

// the tickets of srgpt_decode_attention_multi's workspace (internal: srgpt_llm_lookup_sync_state of model.hip reads them back)
void* srgpt_decode_attn_multi_sync_words(float* ws, int B, int T, int Hq, int D, size_t* bytes) {
  if (bytes) *bytes = attn_ws_tickets_reserved(B, Hq) * sizeof(int);
  return ws + attn_multi_ws_partial_floats(B, T, Hq, D);
}

extern "C" int srgpt_decode_attention_multi(void* qkv, void* kcache, void* vcache, const int* pos, const void* cos_tab,
                                            const void* sin_tab, void* out, float* ws, int B, int T, int Hq, int Hkv, int D, int max_pos,
                                            int dtype, srgpt_stream_t stream) {
  SRGPT_CHECK(qkv && kcache && vcache && pos && cos_tab && sin_tab && out && ws, SRGPT_ERR_ARG,
              "srgpt_decode_attention_multi: null pointer");
  SRGPT_CHECK(B > 0 && T > 0 && Hq > 0 && Hkv > 0 && Hq % Hkv == 0 && D > 0 && D <= 256 && D % 2 == 0 && max_pos > 0, SRGPT_ERR_ARG,
              "srgpt_decode_attention_multi: bad shape B=%d T=%d Hq=%d Hkv=%d D=%d max_pos=%d", B, T, Hq, Hkv, D, max_pos);
  SRGPT_CHECK(dtype == SRGPT_BF16 || dtype == SRGPT_F32, SRGPT_ERR_ARG, "srgpt_decode_attention_multi: bad dtype %d", dtype);
  const AttnDecodeMultiRoute r = attn_decode_multi_route(dtype == SRGPT_BF16, B, T, Hq, Hkv, D, max_pos);
  SRGPT_CHECK(r.status != ATTN_TOO_MANY_COLUMNS, SRGPT_ERR_UNSUPPORTED,
              "srgpt_decode_attention_multi: T=%d tokens x %d heads per kv head exceed the %d columns of the MFMA kernel (T <= %d)", T, r.G,
              ATTN_DEC_MULTI_COLS, attn_decode_multi_cap(r.G));
  hipStream_t s = as_stream(stream);
  const float scale = 1.0f / sqrtf((float)D);
  if (r.family == ATTN_DECODE_MULTI_MFMA) {
    typedef bf16_t Tb;
    int* tickets = reinterpret_cast<int*>(ws + attn_multi_ws_partial_floats(B, T, Hq, D));
    SRGPT_TRY((srgpt_switch<2, 4, 8, 16>(r.nc, "columns", [&](auto nc_c) {
      hipLaunchKernelGGL((decode_mfma_multi_kernel<decltype(nc_c)::value>), dim3(r.blocks), dim3(256), 0, s, (const Tb*)qkv, (Tb*)kcache,
                         (Tb*)vcache, pos, (const Tb*)cos_tab, (const Tb*)sin_tab, ws, tickets, (Tb*)out, T, r.G, Hq, Hkv, max_pos,
                         r.nsplit, r.kpb, scale);
      return (int)SRGPT_OK;
    })));
    SRGPT_LAUNCH_CHECK();
    return SRGPT_OK;
  }
  // the parity path: the guarded RoPE / append launch (q rotated in place), then causal attention over the cache with q_pos0 = pos and
  // the capacity as the bound on the keys
  if (dtype == SRGPT_BF16)
    hipLaunchKernelGGL(rope_kv_append_guarded_kernel<bf16_t>, dim3(T, B), dim3(256), 0, s, (bf16_t*)qkv, (bf16_t*)kcache, (bf16_t*)vcache,
                       pos, (const bf16_t*)cos_tab, (const bf16_t*)sin_tab, T, Hq, Hkv, D, max_pos);
  else
    hipLaunchKernelGGL(rope_kv_append_guarded_kernel<float>, dim3(T, B), dim3(256), 0, s, (float*)qkv, (float*)kcache, (float*)vcache, pos,
                       (const float*)cos_tab, (const float*)sin_tab, T, Hq, Hkv, D, max_pos);
  SRGPT_LAUNCH_CHECK();
  // srgpt_attention_append's one-wave kernel, on every dtype: it reads no key behind a row's own position, and the cache rows behind
  // the live length may hold anything (the flash kernel would multiply them by a zero probability)
  const int64_t QW = (int64_t)(Hq + 2 * Hkv) * D, hs = (int64_t)max_pos * D;
  const dim3 grid(T, Hq, B), block(64);
  if (dtype == SRGPT_BF16)
    hipLaunchKernelGGL(simple_attn_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)qkv, (const bf16_t*)kcache, (const bf16_t*)vcache,
                       (bf16_t*)out, T, max_pos, Hq, Hkv, D, (int64_t)T * QW, QW, (int64_t)D, (int64_t)Hkv * hs, (int64_t)D, hs,
                       (int64_t)Hkv * hs, (int64_t)D, hs, scale, 1, (const int*)nullptr, pos);
  else
    hipLaunchKernelGGL(simple_attn_kernel<float>, grid, block, 0, s, (const float*)qkv, (const float*)kcache, (const float*)vcache,
                       (float*)out, T, max_pos, Hq, Hkv, D, (int64_t)T * QW, QW, (int64_t)D, (int64_t)Hkv * hs, (int64_t)D, hs,
                       (int64_t)Hkv * hs, (int64_t)D, hs, scale, 1, (const int*)nullptr, pos);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

// srgpt_attention and srgpt_attention_append for validated arguments: the route (attn_route.h) and the one launch of its kernel.
// q_pos0 = NULL: the uniform causal offset Tk - Tq; else (causal) the per-row one
static int attention_launch(const void* q, const void* k, const void* v, void* o, int B, int Tq, int Tk, int Hq, int Hkv, int D,
                            int64_t q_bs, int64_t q_ts, int64_t q_hs, int64_t k_bs, int64_t k_ts, int64_t k_hs, int64_t v_bs,
                            int64_t v_ts, int64_t v_hs, float scale, int causal, const int* kv_len, const int* q_pos0, int dtype,
                            hipStream_t s) {
  const bool qkv16 = (uintptr_t)q % 16 == 0 && (uintptr_t)k % 16 == 0 && (uintptr_t)v % 16 == 0;
  const AttnPrefillRoute r = attn_prefill_route(dtype == SRGPT_BF16, D, Tq, Tk, Hq, B, q_bs, q_ts, q_hs, k_bs, k_ts, k_hs, v_bs, v_ts, v_hs,
                                                qkv16, (uintptr_t)o % 8 == 0, scale > 0.f);
  const dim3 grid(r.grid_x, r.grid_y, r.grid_z), block(r.block);
  if (r.family == ATTN_FLASH) {
    AttnArgs a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, Tq, Tk, Hq, Hkv, D,
               q_bs, q_ts, q_hs, k_bs, k_ts, k_hs, v_bs, v_ts, v_hs, scale, kv_len, q_pos0};
    SRGPT_TRY(srgpt_flash_bf16_launch(a, r, causal != 0, s));
  } else if (dtype == SRGPT_BF16) {
    hipLaunchKernelGGL(simple_attn_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o,
                       Tq, Tk, Hq, Hkv, D, q_bs, q_ts, q_hs, k_bs, k_ts, k_hs, v_bs, v_ts, v_hs, scale, causal, kv_len, q_pos0);
  } else {
    hipLaunchKernelGGL(simple_attn_kernel<float>, grid, block, 0, s, (const float*)q, (const float*)k, (const float*)v, (float*)o, Tq,
                       Tk, Hq, Hkv, D, q_bs, q_ts, q_hs, k_bs, k_ts, k_hs, v_bs, v_ts, v_hs, scale, causal, kv_len, q_pos0);
  }
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

extern "C" int srgpt_attention(const void* q, const void* k, const void* v, void* o, int B, int Tq, int Tk, int Hq,
                               int Hkv, int D, int64_t q_bs, int64_t q_ts, int64_t q_hs, int64_t k_bs, int64_t k_ts,
                               int64_t k_hs, int64_t v_bs, int64_t v_ts, int64_t v_hs, float scale, int causal,
                               const int* kv_len, int dtype, srgpt_stream_t stream) {
  SRGPT_CHECK(q && k && v && o, SRGPT_ERR_ARG, "srgpt_attention: null pointer");
  SRGPT_CHECK(B > 0 && Tq > 0 && Tk > 0 && Hq > 0 && Hkv > 0 && Hq % Hkv == 0 && D > 0 && D <= 256, SRGPT_ERR_ARG,
              "srgpt_attention: bad shape B=%d Tq=%d Tk=%d Hq=%d Hkv=%d D=%d", B, Tq, Tk, Hq, Hkv, D);
  SRGPT_CHECK(dtype == SRGPT_BF16 || dtype == SRGPT_F32, SRGPT_ERR_ARG, "srgpt_attention: bad dtype %d", dtype);
  return attention_launch(q, k, v, o, B, Tq, Tk, Hq, Hkv, D, q_bs, q_ts, q_hs, k_bs, k_ts, k_hs, v_bs, v_ts, v_hs, scale, causal, kv_len,
                          nullptr, dtype, as_stream(stream));
}

extern "C" int srgpt_attention_append(const void* q, const void* k, const void* v, void* o, int B, int Tq, int Tk, int Hq, int Hkv,
                                      int D, int64_t q_bs, int64_t q_ts, int64_t q_hs, int64_t k_bs, int64_t k_ts, int64_t k_hs,
                                      int64_t v_bs, int64_t v_ts, int64_t v_hs, float scale, const int* q_pos0, const int* kv_len,
                                      int dtype, srgpt_stream_t stream) {
  SRGPT_CHECK(q && k && v && o, SRGPT_ERR_ARG, "srgpt_attention_append: null pointer");
  SRGPT_CHECK(q_pos0, SRGPT_ERR_ARG, "srgpt_attention_append: q_pos0 is null (a uniform causal offset is srgpt_attention)");
  SRGPT_CHECK(B > 0 && Tq > 0 && Tk > 0 && Hq > 0 && Hkv > 0 && Hq % Hkv == 0 && D > 0 && D <= 256, SRGPT_ERR_ARG,
              "srgpt_attention_append: bad shape B=%d Tq=%d Tk=%d Hq=%d Hkv=%d D=%d", B, Tq, Tk, Hq, Hkv, D);
  SRGPT_CHECK(dtype == SRGPT_BF16 || dtype == SRGPT_F32, SRGPT_ERR_ARG, "srgpt_attention_append: bad dtype %d", dtype);
  return attention_launch(q, k, v, o, B, Tq, Tk, Hq, Hkv, D, q_bs, q_ts, q_hs, k_bs, k_ts, k_hs, v_bs, v_ts, v_hs, scale, 1, kv_len,
                          q_pos0, dtype, as_stream(stream));
}
