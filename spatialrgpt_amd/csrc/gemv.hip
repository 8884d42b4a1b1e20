// Decode-path weight-streaming GEMV (bf16: one row, fp32: up to 4; more rows -> skinny.hip): out[b, n] = W[n, :] . x[b, :]   (HBM-bound)
//
// Roofline: every weight byte is read exactly once per token (non-temporal 16-byte loads, one 1 KiB
// wave-instruction per row chunk); x lives in LDS; fp32 accumulate on the VALU (24 lane-ops per 16 B --
// ~12 % of VALU issue at HBM rate, so no MFMA reshaping).
//
// Work decomposition: a unit = one output row (plain) or one (gate row, up row) pair (SwiGLU); each wave owns
// units grid-strided; per unit the K range is walked in batches of 8 row chunks: 8 independent 1-KiB loads are
// issued back to back, then consumed in order with counted waits.  No cross-batch software pipeline: measured
// (scripts/experiments/ubench_stream.hip and per-wave timestamps, round 2) a 3-deep register pipeline with 16+ loads in flight per wave
// was 2-3 us SLOWER per launch -- 8 waves/CU x 8 KiB already saturate HBM, and the independent waves of a CU
// drift apart so that some stream while others multiply.  Grid = 2 blocks per CU.
//
// Fusions (include/srgpt.h): RMSNorm prologue (LlamaRMSNorm), SwiGLU epilogue, residual add, fp32 logits.
// Rounding points mirror PyTorch's bf16 materialisation of each intermediate.  The prologue and the epilogue are the ones of
// gemv_valu.h, shared with the other VALU products (gemv_w8.hip, gemv_w4.hip, gemv_p13.hip); this file also holds the one pass loop
// of every decode product (srgpt_decode_product).
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "gemv_route.h"
#include "gemv_valu.h"
#include "internal.h"

namespace {

template <typename T>
struct WChunk;  // 16 bytes of weights -> VEC floats
template <>
struct WChunk<bf16_t> {
  static constexpr int VEC = 8;
  static __device__ __forceinline__ void cvt(const u32x4& r, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = bf16lo(r[i]);
      f[2 * i + 1] = bf16hi(r[i]);
    }
  }
};
template <>
struct WChunk<float> {
  static constexpr int VEC = 4;
  static __device__ __forceinline__ void cvt(const u32x4& r, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = __uint_as_float(r[i]);
  }
};

// UB = loads per batch (8; 7 for rows whose chunk iterations are a multiple of 7 and not of 8 -- K = 14336, down_proj: 28 iterations are
// 4 batches of 7, where batches of 8 spent every row's fourth batch half on clamped re-reads of the row's last chunk)
template <typename T, int B, bool SWIGLU, int NXMAX, int UB = 8>
__global__ __launch_bounds__(256, 2) void gemv_kernel(const T* __restrict__ x, const T* __restrict__ W,
                                                      const T* __restrict__ norm_w, float norm_eps,
                                                      const T* __restrict__ residual, void* __restrict__ out, int N,
                                                      int K, int out_f32) {
  constexpr int VEC = WChunk<T>::VEC;
  constexpr int R = SWIGLU ? 2 : 1;  // weight rows per unit
  constexpr int U = UB / R;          // K-chunks per row per batch: 8 loads (8 KiB per wave) in flight, then consumed
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* xs = reinterpret_cast<T*>(smem);  // [B][K]
  __shared__ float red[16];
  __shared__ float res_s[B][4][GEMV_RES_MAXU];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunks = K / VEC;          // 16-byte chunks per row
  const int nit = (nchunks + 63) >> 6;  // chunk iterations per row (64 lanes each)

  // one batch = 8 independent 1-KiB wave loads (R rows x U chunks), issued back to back in consumption order, indices clamped,
  // never branched, so the compiler can place counted s_waitcnt vmcnt(N) in front of each consumer
  u32x4 w[R][U];
  auto issue = [&](int unit, int it0) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const u32x4* p = reinterpret_cast<const u32x4*>(W + (size_t)(unit + r * N) * K);
#pragma unroll
      for (int j = 0; j < U; ++j) {
        w[r][j] = __builtin_nontemporal_load(p + min((it0 + j) * 64 + lane, nchunks - 1));
        __builtin_amdgcn_sched_barrier(0);  // issue order == consumption order (see gemv_valu.h)
      }
    }
  };

  // x (RMSNormed) into LDS, the residual elements of the wave's first units, the first weight batch behind the prologue's loads
  gemv_valu_prologue<T, B, NXMAX, 1, SWIGLU>(x, norm_w, norm_eps, residual, N, K, xs, red, res_s,
                                             [&] { issue(min((int)blockIdx.x * 4 + wave, N - 1), 0); });

  int uk = 0;
  for (int unit = blockIdx.x * 4 + wave; unit < N; unit += gridDim.x * 4, ++uk) {
    float acc[R][B];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int b = 0; b < B; ++b) acc[r][b] = 0.f;

    for (int it0 = 0; it0 < nit; it0 += U) {
      // Waves drift apart naturally, so some stream while others multiply; 8 waves/CU keep 64 KiB in flight.
#pragma unroll
      for (int j = 0; j < U; ++j) {
        // branch-free: a chunk index past the row end is clamped for the loads and its weights are zeroed here.
        // (A per-chunk `if` made the compiler sink the chunk's global load INTO the branch, behind all the others,
        //  followed by s_waitcnt vmcnt(0): every batch was fully drained before its first FMA.)
        const int ch = (it0 + j) * 64 + lane;
        const bool valid = ch < nchunks;
        const int chc = valid ? ch : nchunks - 1;
        float wf[R][VEC];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          u32x4 wv = w[r][j];
#pragma unroll
          for (int q = 0; q < 4; ++q) wv[q] = valid ? wv[q] : 0u;
          WChunk<T>::cvt(wv, wf[r]);
        }
#pragma unroll
        for (int b = 0; b < B; ++b) {
          const Vec16<T> xv = *reinterpret_cast<const Vec16<T>*>(xs + (size_t)b * K + (size_t)chc * VEC);
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float xf = xv.get(i);
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r][b] = fmaf(wf[r][i], xf, acc[r][b]);
          }
        }
      }
      // the registers are free again: the next batch of this wave's stream (the row's next chunks, or the first chunks of its
      // next unit; past the last unit a valid row is re-read and dropped) goes out before the reduction and the store
      {
        const bool more = it0 + U < nit;
        issue(more ? unit : min(unit + (int)gridDim.x * 4, N - 1), more ? it0 + U : 0);
      }
    }

#pragma unroll
    for (int b = 0; b < B; ++b) {
      float a[R];
#pragma unroll
      for (int r = 0; r < R; ++r) a[r] = wave_sum(acc[r][b]);
      if (lane == 0)
        gemv_valu_epilogue<T, SWIGLU>(a[0], a[R - 1], residual, uk < GEMV_RES_MAXU ? &res_s[b][wave][uk] : nullptr, out, (size_t)b * N + unit,
                                      out_f32);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Batch-1 bf16 variant with the activation row held in REGISTERS (no LDS, no block barrier).  Lane l only ever multiplies
// chunks l, l + 64, ... of the row, so a wave keeps NIT = ceil(K / 512) packed 16-byte chunks per lane (32 VGPRs at
// K = 4096, 112 at 14336) for all its rows; every wave holds the whole row across its lanes, so the RMSNorm sum of squares
// is one wave_sum -- no cross-wave reduction, no __syncthreads.  The prologue shrinks to NIT (+NIT gain) loads and a
// shuffle reduction, the inner loop loses its ds_read per chunk, and a K that is not a multiple of 4096 wastes no load
// slots (NIT is a template parameter: static register indexing, exact batch sizes).  Residual elements of the wave's first
// units are fetched up front by lanes 0..3 and broadcast with a shuffle.
// ------------------------------------------------------------------------------------------------
template <bool SWIGLU, bool NORM, int NIT, int UB = 8>
__global__ __launch_bounds__(256, 2) void gemv_reg_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ W,
                                                          const bf16_t* __restrict__ norm_w, float norm_eps,
                                                          const bf16_t* __restrict__ residual, void* __restrict__ out, int N,
                                                          int K, int out_f32) {
  typedef bf16_t T;
  constexpr int VEC = 8;
  constexpr int R = SWIGLU ? 2 : 1;
  constexpr int U = UB / R;
  constexpr int RES_MAXU = GEMV_RES_MAXU;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunks = K / VEC;

  // one batch of the weight stream: the static chunks IT0 .. IT0 + U - 1 of the unit's R rows (issue order == consumption order)
  u32x4 w[R][U];
  auto issue = [&](int unit, auto it0_c) {
    constexpr int IT0 = decltype(it0_c)::value;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const u32x4* p = reinterpret_cast<const u32x4*>(W + (size_t)(unit + r * N) * K);
#pragma unroll
      for (int j = 0; j < U; ++j) {
        if (IT0 + j < NIT) {  // static
          w[r][j] = __builtin_nontemporal_load(p + min((IT0 + j) * 64 + lane, nchunks - 1));
          __builtin_amdgcn_sched_barrier(0);  // issue order == consumption order (see gemv_kernel)
        }
      }
    }
  };

  // ---- prologue: the lane's chunks of x (and gains), straight to registers; nothing here is shared between waves ----
  u32x4 xp[NIT];
  unsigned int res_raw;  // bf16 bits of the residual element of unit `lane` (lanes 0..3); unconditional load, converted at its use
  {
    {
      const int ru = (int)blockIdx.x * 4 + wave + min(lane, RES_MAXU - 1) * (int)gridDim.x * 4;
      const bool has = !SWIGLU && residual != nullptr;  // (see gemv_kernel: a branch here cost a memory round trip per launch)
      res_raw = *reinterpret_cast<const unsigned short*>((has ? residual : x) + (has ? min(ru, N - 1) : 0));
    }
    u32x4 gr[NORM ? NIT : 1];
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      const int c = min(j * 64 + lane, nchunks - 1);
      xp[j] = *reinterpret_cast<const u32x4*>(x + (size_t)c * VEC);
      if (NORM) gr[j] = *reinterpret_cast<const u32x4*>(norm_w + (size_t)c * VEC);
    }
    if (NORM) {
      float ss = 0.f;
#pragma unroll
      for (int j = 0; j < NIT; ++j) {
        const bool ok = j * 64 + lane < nchunks;
        float sq = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float lo = bf16lo(xp[j][q]), hi = bf16hi(xp[j][q]);
          sq += lo * lo + hi * hi;
        }
        ss += ok ? sq : 0.f;
      }
      const float r = rsqrtf(wave_sum(ss) / (float)K + norm_eps);
#pragma unroll
      for (int j = 0; j < NIT; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          // weight * hidden.to(dtype): two roundings, as LlamaRMSNorm materialises them
          bf16x2 p;
          p[0] = (bf16_t)(bf16lo(gr[j][q]) * rnd<T>(bf16lo(xp[j][q]) * r));
          p[1] = (bf16_t)(bf16hi(gr[j][q]) * rnd<T>(bf16hi(xp[j][q]) * r));
          xp[j][q] = __builtin_bit_cast(unsigned int, p);
        }
    }
  }

  int uk = 0;
  for (int unit = blockIdx.x * 4 + wave; unit < N; unit += gridDim.x * 4, ++uk) {
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    if constexpr (NIT > 16) {
      // long rows: the activations are loop-invariant, and left alone the compiler hoists their bf16 -> fp32 unpacking out of the
      // unit loop -- twice the registers for x (224 at K = 14336) and the kernel spills; opaque per unit, the packed form stays
#pragma unroll
      for (int j = 0; j < NIT; ++j) asm volatile("" : "+v"(xp[j]));
    }
    auto batch = [&](auto it0_c) {
      constexpr int it0 = decltype(it0_c)::value;
      // issue -> consume per batch: the pipelined form of gemv_kernel was measured slower here (o_proj, whose weights are
      // L2-prefetched: 3.036 vs 3.042 ms per token, o_proj 5.0 vs 5.45 us)
      issue(unit, it0_c);
#pragma unroll
      for (int j = 0; j < U; ++j) {
        if (it0 + j < NIT) {  // static
          const bool valid = (it0 + j) * 64 + lane < nchunks;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float x0 = bf16lo(xp[it0 + j][q]), x1 = bf16hi(xp[it0 + j][q]);
#pragma unroll
            for (int r = 0; r < R; ++r) {
              const unsigned int wq = valid ? w[r][j][q] : 0u;
              acc[r] = fmaf(bf16lo(wq), x0, acc[r]);
              acc[r] = fmaf(bf16hi(wq), x1, acc[r]);
            }
          }
        }
      }
    };
    batch(std::integral_constant<int, 0>{});
    if constexpr (U < NIT) batch(std::integral_constant<int, U>{});
    if constexpr (2 * U < NIT) batch(std::integral_constant<int, 2 * U>{});
    if constexpr (3 * U < NIT) batch(std::integral_constant<int, 3 * U>{});
    static_assert(4 * U >= NIT, "gemv_reg_kernel: at most 4 batches per row");
    float a[R];
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = wave_sum(acc[r]);
    // lane uk of res_pre holds the residual element of this unit (uniform index: v_readlane, not a ds_bpermute)
    const float res_b = __uint_as_float((unsigned int)__builtin_amdgcn_readlane((int)res_raw, uk < RES_MAXU ? uk : 0) << 16);
    if (lane == 0)
      gemv_valu_epilogue<T, SWIGLU>(a[0], a[R - 1], residual, uk < RES_MAXU ? &res_b : nullptr, out, (size_t)unit, out_f32);
  }
}

// one launch of up to 4 rows on the route's VALU kernel (GEMV_LDS or GEMV_REG)
template <typename T>
int launch_gemv(GemvFamily family, const DecodeProduct& p, hipStream_t s) {
  const GemvValuLaunch l = gemv_valu_launch(family, p.batch, p.N, p.K, sizeof(T) == 2, p.swiglu != 0, srgpt_device_cus());
  const T *x = (const T*)p.x, *W = (const T*)p.W, *norm_w = (const T*)p.norm_w, *residual = (const T*)p.residual;
  SRGPT_TRY((srgpt_switch<false, true>(p.swiglu != 0, "SWIGLU", [&](auto sw_c) {
    constexpr bool SW = decltype(sw_c)::value;
    if constexpr (sizeof(T) == 2) {
      if (family == GEMV_REG)
        return srgpt_switch<5, 8, 14>(l.NIT, "NIT", [&](auto nit_c) {  // K = 2560, 4096, 6912
          hipLaunchKernelGGL((gemv_reg_kernel<SW, false, decltype(nit_c)::value>), dim3(l.grid), dim3(256), 0, s, x, W, norm_w, p.eps,
                             residual, p.out, p.N, p.K, p.out_f32);
          return (int)SRGPT_OK;
        });
    }
    return srgpt_switch<1, 2, 3, 4>(l.B, "B", [&](auto b_c) {
      return srgpt_switch<2, 8>(l.NX, "NX", [&](auto nx_c) {
        constexpr int B = decltype(b_c)::value, NX = decltype(nx_c)::value;
        const auto go = [&](auto ub_c) {
          constexpr auto kfn = &gemv_kernel<T, B, SW, NX, decltype(ub_c)::value>;
          return gemv_valu_run<kfn>(l, "srgpt_gemv: batch*K", s, x, W, norm_w, p.eps, residual, p.out, p.N, p.K, p.out_f32);
        };
        if constexpr (!SW && NX == 8) {  // the only instances with batches of 7 loads (scripts/compare_isa.py guards the instance set)
          if (l.UB == 7) return go(std::integral_constant<int, 7>{});
        }
        return go(std::integral_constant<int, 8>{});
      });
    });
  })));
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

}  // namespace

// The decode products' one way in: every entry point validates its arguments, asks gemv_route.h for its route and comes here.  The
// route names the kernel family and the rows per weight pass; every pass takes its rows of x, residual, out and both statistics
// tables.  A wide route (chunk 32, gemv_wide_route): a chunk of 17 - 32 rows is one wide launch, a tail of 16 rows or fewer the
// 16-row launch of its row count (srgpt_skinny_launch picks by the chunk's rows).
int srgpt_decode_product(const DecodeProduct& p, const GemvRoute& r, hipStream_t s) {
  const bool bf16 = p.dtype == SRGPT_BF16;
  const size_t es = dtype_size(p.dtype), on = p.out_f32 ? sizeof(float) : es;
  for (int b0 = 0; b0 < p.batch; b0 += r.chunk) {
    DecodeProduct c = p;
    c.batch = p.batch - b0 < r.chunk ? p.batch - b0 : r.chunk;
    c.x = (const char*)p.x + (size_t)b0 * p.K * es;
    if (p.residual) c.residual = (const char*)p.residual + (size_t)b0 * p.N * es;
    c.out = (char*)p.out + (size_t)b0 * p.N * on;
    if (p.ss_in) c.ss_in = p.ss_in + (size_t)b0 * SRGPT_ROWSS_STRIDE;
    if (p.ss_out) c.ss_out = p.ss_out + (size_t)b0 * SRGPT_ROWSS_STRIDE;
    switch (r.family) {
      case GEMV_SKINNY:
      case GEMV_W4_MFMA: SRGPT_TRY(srgpt_skinny_launch(c, s)); break;
      case GEMV_W8: SRGPT_TRY(srgpt_gemv_w8_valu(c, s)); break;
      case GEMV_W4: SRGPT_TRY(srgpt_gemv_w4_valu(c, s)); break;
      default: SRGPT_TRY(bf16 ? launch_gemv<bf16_t>(r.family, c, s) : launch_gemv<float>(r.family, c, s));
    }
  }
  return SRGPT_OK;
}

// srgpt_gemv, srgpt_gemv_w8 (skinny.hip) and srgpt_gemv_rowss: the route of gemv_route
int srgpt_decode_product(const DecodeProduct& p, hipStream_t s) {
  return srgpt_decode_product(p, gemv_route(p.batch, p.K, p.dtype == SRGPT_BF16, p.fp8 != 0, p.norm_w != nullptr), s);
}

extern "C" int srgpt_gemv(const void* x, const void* W, const void* norm_w, float norm_eps, const void* residual,
                          void* out, int batch, int N, int K, int swiglu, int out_f32, int dtype,
                          srgpt_stream_t stream) {
  SRGPT_CHECK(x && W && out, SRGPT_ERR_ARG, "srgpt_gemv: null pointer");
  SRGPT_CHECK(N > 0 && K > 0 && batch > 0, SRGPT_ERR_ARG, "srgpt_gemv: bad shape");
  SRGPT_CHECK(dtype == SRGPT_F32 || dtype == SRGPT_BF16, SRGPT_ERR_ARG, "srgpt_gemv: bad dtype %d", dtype);
  const int vec = dtype == SRGPT_BF16 ? 8 : 4;
  SRGPT_CHECK(K % vec == 0, SRGPT_ERR_ARG, "srgpt_gemv: K=%d must be a multiple of %d", K, vec);
  SRGPT_CHECK(!(swiglu && (residual || out_f32)), SRGPT_ERR_ARG, "srgpt_gemv: swiglu excludes residual/out_f32");
  return srgpt_decode_product(DecodeProduct{x, W, nullptr, norm_w, norm_eps, residual, out, batch, N, K, swiglu, out_f32, dtype, 0,
                                            nullptr, nullptr, 0},
                              as_stream(stream));
}

// ------------------------------------------------------------------------------------------------
// The same products with the row-statistics hand-off of skinny.hip (ABI 8): bf16 activations, 2+ rows (the MFMA kernel).
// ------------------------------------------------------------------------------------------------
static_assert(GEMV_ROWSS_SLOTS == SRGPT_ROWSS_STRIDE, "gemv_route.h counts the slots of include/srgpt.h's tables");
extern "C" int srgpt_gemv_rowss_supported(int batch, int dtype, int fp8) {
  return gemv_rowss_supported(batch, dtype == SRGPT_BF16, fp8 != 0, srgpt_device_cus()) ? 1 : 0;
}

// srgpt_gemv_rowss (pass_rows = 16: gemv_route's own route) and srgpt_gemv_rowss_wide (32: gemv_wide_route's)
static int gemv_rowss_impl(const void* x, const void* W, const void* W8, const float* wscale, const void* norm_w, float norm_eps,
                           const void* residual, void* out, int batch, int N, int K, int swiglu, int out_f32, const float* rowss_in,
                           float* rowss_out, int packed_rows, int pass_rows, srgpt_stream_t stream) {
  SRGPT_CHECK(x && (W || W8) && out, SRGPT_ERR_ARG, "srgpt_gemv_rowss: null pointer");
  SRGPT_CHECK(packed_rows == 0 || packed_rows == 4 || packed_rows == 8 || packed_rows == 16, SRGPT_ERR_ARG,
              "srgpt_gemv_rowss: packed_rows = %d (0: row-major; 4, 8 or 16 rows per granule)", packed_rows);
  SRGPT_CHECK(packed_rows == 0 || (N % packed_rows == 0 && K % (W8 ? 64 : 32) == 0), SRGPT_ERR_ARG,
              "srgpt_gemv_rowss: the packed layout needs N %% %d == 0 and K %% %d == 0 (N = %d, K = %d)", packed_rows, W8 ? 64 : 32, N, K);
  SRGPT_CHECK(!W8 || wscale, SRGPT_ERR_ARG, "srgpt_gemv_rowss: fp8 weights without row scales");
  SRGPT_CHECK(N > 0 && K > 0 && batch > 0 && K % 8 == 0, SRGPT_ERR_ARG, "srgpt_gemv_rowss: bad shape");
  SRGPT_CHECK(!(swiglu && (residual || out_f32)), SRGPT_ERR_ARG, "srgpt_gemv_rowss: swiglu excludes residual/out_f32");
  SRGPT_CHECK(srgpt_gemv_rowss_supported(batch, SRGPT_BF16, W8 != nullptr), SRGPT_ERR_UNSUPPORTED,
              "srgpt_gemv_rowss: %d row(s) of %s weights take a kernel without the statistics hand-off", batch, W8 ? "fp8" : "bf16");
  return srgpt_decode_product(DecodeProduct{x, W8 ? W8 : W, W8 ? wscale : nullptr, norm_w, norm_eps, residual, out, batch, N, K, swiglu,
                                            out_f32, SRGPT_BF16, W8 != nullptr, rowss_in, rowss_out, packed_rows},
                              gemv_wide_route(batch, K, W8 != nullptr, packed_rows, false, norm_w != nullptr, swiglu != 0, pass_rows),
                              as_stream(stream));
}

extern "C" int srgpt_gemv_rowss(const void* x, const void* W, const void* W8, const float* wscale, const void* norm_w,
                                float norm_eps, const void* residual, void* out, int batch, int N, int K, int swiglu, int out_f32,
                                const float* rowss_in, float* rowss_out, int packed_rows, srgpt_stream_t stream) {
  return gemv_rowss_impl(x, W, W8, wscale, norm_w, norm_eps, residual, out, batch, N, K, swiglu, out_f32, rowss_in, rowss_out, packed_rows,
                         16, stream);
}

// The same product with chunks of 17 - 32 rows in ONE weight pass (gemv_wide_route); 16 rows or fewer: srgpt_gemv_rowss itself
extern "C" int srgpt_gemv_rowss_wide(const void* x, const void* W, const void* W8, const float* wscale, const void* norm_w,
                                     float norm_eps, const void* residual, void* out, int batch, int N, int K, int swiglu, int out_f32,
                                     const float* rowss_in, float* rowss_out, int packed_rows, srgpt_stream_t stream) {
  return gemv_rowss_impl(x, W, W8, wscale, norm_w, norm_eps, residual, out, batch, N, K, swiglu, out_f32, rowss_in, rowss_out, packed_rows,
                         GEMV_WIDE_ROWS, stream);
}

// rows per weight pass gemv_wide_route picks for a call of `batch` rows (16 or 32; a VALU route: its chunk), for tests and callers
extern "C" int srgpt_gemv_wide_pass_rows(int batch, int fp8, int packed, int w4, int N, int K, int norm, int swiglu) {
  (void)N;
  return gemv_wide_route(batch, K, fp8 != 0, packed, w4 != 0, norm != 0, swiglu != 0, GEMV_WIDE_ROWS).chunk;
}
