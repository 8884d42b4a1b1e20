// Decode-path weight-streaming product with MXFP4 weights (W4A16): OCP e2m1 codes, one E8M0 scale byte per 32 values of a row
//   out[b, n] = round_bf16( sum_k x[b, k] * e2m1(W4[n, k]) * 2^(wscale8[n, k / 32] - 127) )       (HBM-bound, a quarter of the bf16 bytes)
// and the exact bf16 expansion of such a matrix (srgpt_dequant_mxfp4, what the prefill multiplies).
//
// Same structure as gemv_w8.hip (wave per unit, 1-KiB non-temporal wave loads issued in consumption order, branch-free consumption
// with clamped indices, scales requested ahead of the weight stream; the prologue -- x in LDS behind the fused RMSNorm, the residual
// elements -- and the SwiGLU / residual / fp32-logit epilogue with the header's rounding points are gemv_valu.h's) with these differences:
//   * a 16-byte chunk holds 32 weights = exactly ONE MX block: a lane needs one scale byte per chunk, fetched (a byte load per
//     chunk) in front of the batch's weight loads;
//   * a K = 4096 row is only 2 wave loads; a unit is W4_UNIT_COLS = 2 output columns like gemv_w8.hip's (plain: 2 rows x 2 chunks =
//     4 loads per batch; SwiGLU: 2 gate + 2 up rows = 8 loads = 8 KiB per wave in flight) -- 4 and 8 columns, which would match
//     gemv_w8.hip's bytes in flight, measured slower (gemv_route.h);
//   * codes are widened with v_cvt_scalef32_pk_f32_fp4, two values per instruction with the block scale applied on the way (the
//     scale operand is the fp32 number 2^(byte - 127) = byte << 23: bytes 1 .. 254, the quantiser never emits 0 or 255); products
//     accumulate as fp32 pairs (even k, odd k), added once per row before the wave reduction;
//   * 1 .. 4 rows of x per launch (template argument), a longer call is cut into launches of 4 (gemv_w4_route): there is no MFMA
//     kernel for this format yet, and no per-row fp32 scale.
#include <stdlib.h>

#include "common.h"
#include "gemv_route.h"
#include "gemv_valu.h"
#include "internal.h"

namespace {

typedef bf16_t T;

// 2^(byte - 127) as the fp32 the conversion instructions take their block scale from (bytes 1 .. 254: a normal number)
__device__ __forceinline__ float e8m0_scale(unsigned int byte) { return __uint_as_float(byte << 23); }

// the two values of byte `SEL` of `word`: [0] = low nibble (even k), [1] = high nibble (odd k), times `scale`
template <int SEL>
__device__ __forceinline__ f32x2 fp4x2(unsigned int word, float scale) {
  return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, scale, SEL);
}

template <int B, bool SWIGLU, int NXMAX>
__global__ __launch_bounds__(256, 2) void gemv_w4_kernel(const T* __restrict__ x, const unsigned char* __restrict__ W,
                                                         const unsigned char* __restrict__ wscale, const T* __restrict__ norm_w,
                                                         float norm_eps, const T* __restrict__ residual,
                                                         void* __restrict__ out, int N, int K, int out_f32) {
  constexpr int WVEC = 32;  // weight elements per 16-byte chunk = one MX block
  constexpr int C = W4_UNIT_COLS;    // output columns per unit
  constexpr int R = SWIGLU ? 2 * C : C;  // weight rows per unit (SwiGLU: C gate + C up rows -> C outputs)
  constexpr int U = 2;               // K-chunks per row per batch
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* xs = reinterpret_cast<T*>(smem);  // [B][K]
  __shared__ float red[16];
  __shared__ float res_s[B][4][C * GEMV_RES_MAXU];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wchunks = K / WVEC;          // 16-byte weight chunks (= scale bytes) per row
  const int nit = (wchunks + 63) >> 6;   // weight-chunk iterations per row (64 lanes each)
  const int NUNIT = (N + C - 1) / C;

  // rows of a unit (wave-uniform: scalar addressing).  plain: rows C u .. C u + C - 1; SwiGLU: those gate rows and the up rows N + ...
  // Rows of a tail unit beyond N are clamped and never stored.
  auto unit_rows = [&](int unit, int* rows) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      rows[c] = __builtin_amdgcn_readfirstlane(min(C * unit + c, N - 1));
      if (SWIGLU) rows[C + c] = __builtin_amdgcn_readfirstlane(N + min(C * unit + c, N - 1));
    }
  };
  // one batch of the weight stream: R rows x U chunks.  The scale bytes go out first (they come back first), then the weight
  // chunks in consumption order; indices clamped, never branched
  u32x4 w[R][U];
  unsigned int sb[R][U];
  auto issue = [&](int unit, int it0) {
    int rows[R];
    unit_rows(unit, rows);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const unsigned char* p = wscale + (size_t)rows[r] * wchunks;
#pragma unroll
      for (int j = 0; j < U; ++j) sb[r][j] = p[min((it0 + j) * 64 + lane, wchunks - 1)];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const u32x4* p = reinterpret_cast<const u32x4*>(W + (size_t)rows[r] * (K / 2));
#pragma unroll
      for (int j = 0; j < U; ++j) {
        w[r][j] = __builtin_nontemporal_load(p + min((it0 + j) * 64 + lane, wchunks - 1));
        __builtin_amdgcn_sched_barrier(0);  // issue order == consumption order (see gemv_valu.h)
      }
    }
  };

  // x (RMSNormed) into LDS, the residual elements of the wave's first units (C columns each), the first weight batch
  gemv_valu_prologue<T, B, NXMAX, C, SWIGLU>(x, norm_w, norm_eps, residual, N, K, xs, red, res_s,
                                             [&] { issue(min((int)blockIdx.x * 4 + wave, NUNIT - 1), 0); });

  int uk = 0;
  for (int unit = blockIdx.x * 4 + wave; unit < NUNIT; unit += gridDim.x * 4, ++uk) {
    f32x2 acc[R][B];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int b = 0; b < B; ++b) acc[r][b] = f32x2{0.f, 0.f};

    for (int it0 = 0; it0 < nit; it0 += U) {
      // A step is word q of chunk j (8 codes of each of the unit's R rows) against activations 8 q .. 8 q + 7 of the chunk as fp32
      // pairs (even k, odd k): one 16-byte LDS read per row of x, shared by the R weight rows.  The reads of step t + 1 are issued
      // ahead of step t's arithmetic, and nothing else moves between steps: left alone, the scheduler hoists every conversion of
      // the batch (256 VGPRs of widened weights) and spills the accumulators.
      auto xread = [&](int t, u32x4* xv) {
        const int ch = min((it0 + (t >> 2)) * 64 + lane, wchunks - 1);
#pragma unroll
        for (int b = 0; b < B; ++b) xv[b] = *reinterpret_cast<const u32x4*>(xs + (size_t)b * K + (size_t)ch * WVEC + 8 * (t & 3));
      };
      u32x4 xv[2][B];
      xread(0, xv[0]);
#pragma unroll
      for (int t = 0; t < 4 * U; ++t) {
        const int j = t >> 2, q = t & 3;
        const bool valid = (it0 + j) * 64 + lane < wchunks;
        if (t + 1 < 4 * U) xread(t + 1, xv[(t + 1) & 1]);
#pragma unroll
        for (int b = 0; b < B; ++b) {
          f32x2 xp[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) xp[i] = f32x2{bf16lo(xv[t & 1][b][i]), bf16hi(xv[t & 1][b][i])};
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const float sc = e8m0_scale(sb[r][j]);
            const unsigned int wq = valid ? w[r][j][q] : 0u;  // code 0 = +0.0
            acc[r][b] = __builtin_elementwise_fma(fp4x2<0>(wq, sc), xp[0], acc[r][b]);
            acc[r][b] = __builtin_elementwise_fma(fp4x2<1>(wq, sc), xp[1], acc[r][b]);
            acc[r][b] = __builtin_elementwise_fma(fp4x2<2>(wq, sc), xp[2], acc[r][b]);
            acc[r][b] = __builtin_elementwise_fma(fp4x2<3>(wq, sc), xp[3], acc[r][b]);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // the next batch of the wave's stream goes out before the reduction and the store (past the last unit: a valid unit, dropped)
      {
        const bool more = it0 + U < nit;
        issue(more ? unit : min(unit + (int)gridDim.x * 4, NUNIT - 1), more ? it0 + U : 0);
      }
    }

#pragma unroll
    for (int b = 0; b < B; ++b) {
      float a[R];
#pragma unroll
      for (int r = 0; r < R; ++r) a[r] = wave_sum(acc[r][b][0] + acc[r][b][1]);
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int n = C * unit + c;
          if (n < N)
            gemv_valu_epilogue<T, SWIGLU>(a[c], a[R - C + c], residual, uk < GEMV_RES_MAXU ? &res_s[b][wave][C * uk + c] : nullptr, out,
                                          (size_t)b * N + n, out_f32);
        }
      }
    }
  }
}

// the bf16 expansion: one thread per 16-byte chunk of codes (one MX block) -> 32 bf16 = four 16-byte stores.  code * 2^e is exact
// in bf16 (one mantissa bit), so the fp32 -> bf16 conversion rounds nothing
__global__ __launch_bounds__(256) void dequant_mxfp4_kernel(const unsigned char* __restrict__ W, const unsigned char* __restrict__ wscale,
                                                            T* __restrict__ out, long long nblocks) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nblocks; i += (long long)gridDim.x * 256) {
    const float sc = e8m0_scale(wscale[i]);
    const u32x4 wv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(W) + i);
    u32x4* dst = reinterpret_cast<u32x4*>(out + i * 32);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x2 v0 = fp4x2<0>(wv[q], sc), v1 = fp4x2<1>(wv[q], sc), v2 = fp4x2<2>(wv[q], sc), v3 = fp4x2<3>(wv[q], sc);
      u32x4 o;
      o[0] = (__float_as_uint(v0[0]) >> 16) | (__float_as_uint(v0[1]) & 0xffff0000u);  // exact values: truncation == rounding
      o[1] = (__float_as_uint(v1[0]) >> 16) | (__float_as_uint(v1[1]) & 0xffff0000u);
      o[2] = (__float_as_uint(v2[0]) >> 16) | (__float_as_uint(v2[1]) & 0xffff0000u);
      o[3] = (__float_as_uint(v3[0]) >> 16) | (__float_as_uint(v3[1]) & 0xffff0000u);
      dst[q] = o;
    }
  }
}

}  // namespace

// one launch of up to W4_MAX_ROWS rows (GEMV_W4 of gemv_route.h), entered from srgpt_decode_product (gemv.hip)
int srgpt_gemv_w4_valu(const DecodeProduct& p, hipStream_t s) {
  const GemvValuLaunch l = gemv_w4_launch(p.batch, p.N, p.K, p.swiglu != 0, srgpt_device_cus());
  SRGPT_TRY((srgpt_switch<false, true>(p.swiglu != 0, "SWIGLU", [&](auto sw_c) {
    return srgpt_switch<1, 2, 3, 4>(l.B, "B", [&](auto b_c) {
      return srgpt_switch<2, 8>(l.NX, "NX", [&](auto nx_c) {
        constexpr auto kfn = &gemv_w4_kernel<decltype(b_c)::value, decltype(sw_c)::value, decltype(nx_c)::value>;
        return gemv_valu_run<kfn>(l, "srgpt_gemv_w4: batch*K", s, (const T*)p.x, (const unsigned char*)p.W, p.wscale8, (const T*)p.norm_w,
                                  p.eps, (const T*)p.residual, p.out, p.N, p.K, p.out_f32);
      });
    });
  })));
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

extern "C" int srgpt_gemv_w4(const void* x, const void* W4, const void* wscale8, const void* norm_w, float norm_eps,
                             const void* residual, void* out, int batch, int N, int K, int swiglu, int out_f32,
                             srgpt_stream_t stream) {
  SRGPT_CHECK(x && W4 && wscale8 && out, SRGPT_ERR_ARG, "srgpt_gemv_w4: null pointer");
  SRGPT_CHECK(N > 0 && K > 0 && batch > 0, SRGPT_ERR_ARG, "srgpt_gemv_w4: bad shape");
  SRGPT_CHECK(K % 32 == 0, SRGPT_ERR_ARG, "srgpt_gemv_w4: K=%d must be a multiple of 32 (one scale per 32 values)", K);
  SRGPT_CHECK(!(swiglu && (residual || out_f32)), SRGPT_ERR_ARG, "srgpt_gemv_w4: swiglu excludes residual/out_f32");
  SRGPT_CHECK((long long)N * (swiglu ? 2 : 1) <= 0x7fffffffLL / 2, SRGPT_ERR_ARG, "srgpt_gemv_w4: N=%d too large", N);
  return srgpt_decode_product(DecodeProduct{x, W4, nullptr, norm_w, norm_eps, residual, out, batch, N, K, swiglu, out_f32, SRGPT_BF16, 0,
                                            nullptr, nullptr, 0, 0, (const unsigned char*)wscale8},
                              gemv_w4_route(batch), as_stream(stream));
}

extern "C" int srgpt_dequant_mxfp4(const void* W4, const void* wscale8, void* out_bf16, int N, int K, srgpt_stream_t stream) {
  SRGPT_CHECK(W4 && wscale8 && out_bf16, SRGPT_ERR_ARG, "srgpt_dequant_mxfp4: null pointer");
  SRGPT_CHECK(N > 0 && K > 0, SRGPT_ERR_ARG, "srgpt_dequant_mxfp4: bad shape");
  SRGPT_CHECK(K % 32 == 0, SRGPT_ERR_ARG, "srgpt_dequant_mxfp4: K=%d must be a multiple of 32 (one scale per 32 values)", K);
  const long long nblocks = (long long)N * (K / 32);
  const long long want = (nblocks + 255) / 256, cap = (long long)srgpt_device_cus() * 16;
  hipLaunchKernelGGL(dequant_mxfp4_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, as_stream(stream),
                     (const unsigned char*)W4, (const unsigned char*)wscale8, (T*)out_bf16, nblocks);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}
