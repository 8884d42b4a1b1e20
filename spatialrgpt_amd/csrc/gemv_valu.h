// What the VALU decode products share (gemv.hip, gemv_w8.hip, gemv_w4.hip, gemv_p13.hip): the prologue that stages the activation
// rows into LDS, the lane-0 epilogue with the rounding points of include/srgpt.h, and the launch tail.  Every kernel is 256 threads,
// a wave per unit (COLS output columns of the plain product, or of the gate and the up half), units grid-strided; what differs
// between them -- the weight stream and its decoding -- stays in their own files.
#pragma once
#include "common.h"
#include "gemv_route.h"

// residual elements of a wave's first GEMV_RES_MAXU units are staged through LDS by the prologue: res_s[row][wave][unit * COLS + column]
constexpr int GEMV_RES_MAXU = 4;

// block_sum (common.h) for the four waves these kernels always have: the same additions in the same order, hence the same bits,
// without reading blockDim.  (Called from the prologue below in an instance that stages residual elements, block_sum fetched
// blockDim.x with a VECTOR load -- the compiler no longer folded the work-group size there -- and the s_waitcnt vmcnt(0) in front
// of its use drained the wave's first weight batch before the statistics: q/k/v 10.3 -> 11.5 us per launch at one bf16 row, measured.)
__device__ __forceinline__ float gemv_valu_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) t += red[i];
  return t;
}

// ---- prologue: stage x (and RMSNorm it, LlamaRMSNorm's two roundings) into LDS: xs[B][K] ----
// All global loads of the prologue (activation chunks AND norm gains) are issued up front, branch-free, so the block pays one L2
// latency.  NXMAX (2 or 8, picked by the host: gemv_route.h) = chunks per thread held in registers; unused slots WRAP around to valid
// chunks (a clamped address would hot-spot one cache line from every thread of the grid); chunks beyond NXMAX * 256 (B * K > 16384
// elements) take the generic loops marked "rare".
// first_batch(): issues the wave's first weight batch (and whatever else the kernel wants behind the prologue's loads, such as LDS
// stores the statistics do not wait for).  It goes out BEHIND the prologue's own loads -- in-order return: the statistics below wait
// for the activations only -- and its HBM latency overlaps the RMSNorm, the LDS staging and the barrier.  Inside it, as in every
// later batch, ISSUE order must equal CONSUMPTION order (a sched_barrier(0) after each load): left alone, the scheduler issued the
// first-consumed chunk last, which turns the consumers' counted waits into a full vmcnt(0) drain before the first FMA.
// red: 16 floats of LDS for the block sums.  Ends with the block barrier: xs and res_s are readable on return.
template <typename T, int B, int NXMAX, int COLS, bool SWIGLU, typename FirstBatch>
__device__ __forceinline__ void gemv_valu_prologue(const T* x, const T* norm_w, float norm_eps, const T* residual, int N, int K, T* xs,
                                                   float* red, float (&res_s)[B][4][COLS * GEMV_RES_MAXU], FirstBatch&& first_batch) {
  constexpr int VEC = Vec16<T>::N;
  constexpr unsigned RSLOT = COLS * GEMV_RES_MAXU;  // (unit, column of the unit) slots per wave and row
  static_assert(B * 4 * RSLOT <= 256, "one thread per staged residual element");
  const int tid = threadIdx.x;
  const int nchunks = K / VEC, total = B * nchunks;  // 16-byte activation chunks per row, of all rows
  const bool do_norm = norm_w != nullptr;
  Vec16<T> xr[NXMAX], gr[NXMAX];
  // Residual elements this block will need: fetched with the prologue's loads (a load placed next to its use at the end of a row gets
  // sunk behind the weight stream by the compiler and exposes a full memory latency per row).  The load is UNCONDITIONAL and its value
  // is not touched until the LDS store below.  Written as `if (residual) r = to_f(residual[i])` the compiler emitted branch -> load ->
  // s_waitcnt vmcnt(0) -> convert at the very top of the kernel: o_proj and down_proj spent a whole memory round trip (the row was
  // just written by the launch before: an L2 miss) before requesting their first activation or weight byte.
  // Thread t owns slot (row rb, wave rw, rk): shifts and masks, RSLOT and COLS are powers of two where they are not 1.
  const unsigned ut = threadIdx.x, rb = B == 1 ? 0u : ut / (4 * RSLOT), rw = (ut / RSLOT) & 3u, rk = ut % RSLOT;
  const unsigned rcol = (blockIdx.x * 4 + rw + (rk / COLS) * gridDim.x * 4) * COLS + rk % COLS;  // output column
  const bool rok = !SWIGLU && residual != nullptr && ut < B * 4 * RSLOT && rcol < (unsigned)N;
  const T res_raw = (residual != nullptr ? residual : x)[rok ? (size_t)rb * N + rcol : 0];
#pragma unroll
  for (int j = 0; j < NXMAX; ++j) {
    const int c = (tid + 256 * j) % total;
    xr[j] = *reinterpret_cast<const Vec16<T>*>(x + (size_t)c * VEC);
    gr[j] = *reinterpret_cast<const Vec16<T>*>((do_norm ? norm_w : x) + (size_t)(c % nchunks) * VEC);
  }
  __builtin_amdgcn_sched_barrier(0);
  first_batch();
  __builtin_amdgcn_sched_barrier(0);
  float ss[B];
#pragma unroll
  for (int b = 0; b < B; ++b) ss[b] = 0.f;
#pragma unroll
  for (int j = 0; j < NXMAX; ++j) {
    const int c = tid + 256 * j;
    const bool ok = c < total;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < VEC; ++i) sq += xr[j].get(i) * xr[j].get(i);
    const int b = (B == 1) ? 0 : (c % total) / nchunks;
#pragma unroll
    for (int bb = 0; bb < B; ++bb) ss[bb] += (ok && bb == b) ? sq : 0.f;
  }
  for (int c = tid + 256 * NXMAX; c < total; c += 256) {  // rare
    const Vec16<T> v = *reinterpret_cast<const Vec16<T>*>(x + (size_t)c * VEC);
    *reinterpret_cast<Vec16<T>*>(xs + (size_t)c * VEC) = v;
    const int b = (B == 1) ? 0 : c / nchunks;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < VEC; ++i) sq += v.get(i) * v.get(i);
#pragma unroll
    for (int bb = 0; bb < B; ++bb)
      if (bb == b) ss[bb] += sq;
  }
  if (rok) res_s[rb][rw][rk] = to_f(res_raw);
  float rs[B];
#pragma unroll
  for (int b = 0; b < B; ++b) rs[b] = 1.f;
  if (do_norm) {
    // (the SwiGLU instances keep common.h's block_sum: there blockDim.x still folds to a scalar load, and the unrolled sum cost
    //  them registers and occupancy -- gemv_w4_kernel<4, true, 2> 148 -> 237 VGPRs)
#pragma unroll
    for (int b = 0; b < B; ++b)
      rs[b] = rsqrtf((SWIGLU ? block_sum(ss[b], red) : gemv_valu_block_sum(ss[b], red)) / (float)K + norm_eps);
  }
#pragma unroll
  for (int j = 0; j < NXMAX; ++j) {
    const int c = tid + 256 * j;
    if (c < total) {
      Vec16<T> v = xr[j];
      if (do_norm) {
        const int b = (B == 1) ? 0 : c / nchunks;
        float r = rs[0];
#pragma unroll
        for (int bb = 1; bb < B; ++bb)
          if (bb == b) r = rs[bb];
#pragma unroll
        for (int i = 0; i < VEC; ++i) v.set(i, gr[j].get(i) * rnd<T>(xr[j].get(i) * r));  // weight * h.to(dtype)
      }
      *reinterpret_cast<Vec16<T>*>(xs + (size_t)c * VEC) = v;
    }
  }
  if (do_norm) {
    for (int c = tid + 256 * NXMAX; c < total; c += 256) {  // rare; each thread re-reads the chunks it wrote itself
      const int b = (B == 1) ? 0 : c / nchunks, kc = c - b * nchunks;
      Vec16<T> v = *reinterpret_cast<Vec16<T>*>(xs + (size_t)c * VEC);
      const Vec16<T> g = *reinterpret_cast<const Vec16<T>*>(norm_w + (size_t)kc * VEC);
      float r = rs[0];
#pragma unroll
      for (int bb = 1; bb < B; ++bb)
        if (bb == b) r = rs[bb];
#pragma unroll
      for (int i = 0; i < VEC; ++i) v.set(i, g.get(i) * rnd<T>(v.get(i) * r));
      *reinterpret_cast<Vec16<T>*>(xs + (size_t)c * VEC) = v;
    }
  }
  __syncthreads();
}

// ---- epilogue (one lane): the numeric contract of include/srgpt.h for one output element out[idx] ----
// a: the reduced (and scaled) dot product; SwiGLU: a = the gate row's, up = the up row's -> rnd(silu(rnd(a))) * rnd(up), one more
// rounding at the store.  Otherwise rnd(a), plus the residual element (residual != NULL) with a second rounding: *staged, the copy
// the prologue took, or (staged == NULL: a unit past the wave's first GEMV_RES_MAXU) residual[idx]; out_f32: fp32 logits instead of T.
// (Plain arguments on purpose: a callable that captured the unit loop's variables by reference cost gemv_w8_kernel two VGPRs and
// two more spilled ones.)
template <typename T, bool SWIGLU>
__device__ __forceinline__ void gemv_valu_epilogue(float a, float up, const T* residual, const float* staged, void* out, size_t idx,
                                                   int out_f32) {
  if (SWIGLU) {
    const float g = rnd<T>(a), u = rnd<T>(up);
    reinterpret_cast<T*>(out)[idx] = from_f<T>(rnd<T>(silu(g)) * u);
  } else {
    float v = rnd<T>(a);
    if (residual) v = rnd<T>((staged ? *staged : to_f(residual[idx])) + v);
    if (out_f32)
      reinterpret_cast<float*>(out)[idx] = v;
    else
      reinterpret_cast<T*>(out)[idx] = from_f<T>(v);
  }
}

// ---- launch tail of the kernels above: the LDS cap of gemv_route.h, the raised dynamic-LDS limit, 256 threads.  `what` heads the
//      refusal ("srgpt_gemv: batch*K") ----
template <auto kfn, typename... Args>
int gemv_valu_run(const GemvValuLaunch& l, const char* what, hipStream_t s, Args... args) {
  SRGPT_CHECK(l.lds <= GEMV_LDS_CAP, SRGPT_ERR_UNSUPPORTED, "%s too large for LDS (%zu bytes)", what, (size_t)l.lds);
  return srgpt_launch_dyn_lds<kfn>(l.raise_lds_limit ? GEMV_LDS_CAP : 0, dim3(l.grid), dim3(256), (size_t)l.lds, s, args...);
}
