// Decode-path weight-streaming GEMV with fp8 weights for one batch row (W8A16, BASELINE config 5):
//   out[b, n] = round_bf16( (sum_k x[b, k] * fp8(W8[n, k])) * wscale[n] )            (HBM-bound, half the bytes of bf16)
//
// Same structure as gemv.hip (wave per unit, 8 independent 1-KiB non-temporal wave loads per batch issued in consumption
// order, branch-free consumption with counted vmcnt; the prologue -- x in LDS behind the fused RMSNorm -- and the SwiGLU /
// residual / fp32-logit epilogue are gemv_valu.h's, with two output columns per unit) with these differences:
//   * a 16-byte chunk holds 16 weights, so a K = 4096 row is 4 wave loads: a unit is TWO output columns (plain: rows 2u,
//     2u+1 -> 8 loads per batch; SwiGLU: gate rows 2u, 2u+1 and up rows N+2u, N+2u+1 -> 16 loads = 16 KiB per batch:
//     at half the bytes per row the per-row latency dominates, fewer and larger rounds win here);
//   * weights are widened with v_cvt_pk_f32_fp8 (OCP e4m3fn on gfx950), 2 values per instruction; the two rows of a unit
//     share the fp32 copies of x;
//   * the per-row scale multiplies the reduced dot product.
// 2+ rows go through the MFMA skinny kernel (skinny.hip, W8 variant: W8_VALU_MAX_BATCH in gemv_route.h).
#include <stdlib.h>

#include "common.h"
#include "gemv_route.h"
#include "gemv_valu.h"
#include "internal.h"

namespace {

typedef bf16_t T;

template <int B, bool SWIGLU, int NXMAX>
__global__ __launch_bounds__(256, 2) void gemv_w8_kernel(const T* __restrict__ x, const unsigned char* __restrict__ W,
                                                         const float* __restrict__ wscale, const T* __restrict__ norm_w,
                                                         float norm_eps, const T* __restrict__ residual,
                                                         void* __restrict__ out, int N, int K, int out_f32) {
  constexpr int WVEC = 16;  // weight elements per 16-byte chunk
  constexpr int R = SWIGLU ? 4 : 2;  // weight rows per unit (SwiGLU: 2 gate + 2 up rows -> 2 outputs; 16 KiB per wave in flight)
  constexpr int U = 4;               // K-chunks per row per batch
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* xs = reinterpret_cast<T*>(smem);  // [B][K]
  __shared__ float red[16];
  __shared__ float res_s[B][4][2 * GEMV_RES_MAXU];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wchunks = K / WVEC;          // 16-byte weight chunks per row
  const int nit = (wchunks + 63) >> 6;   // weight-chunk iterations per row (64 lanes each)
  const int NUNIT = (N + 1) >> 1;

  // rows of a unit (wave-uniform: scalar addressing).  plain: rows 2u, 2u+1; SwiGLU: gate rows 2u, 2u+1 and up rows N+2u, N+2u+1.
  // The second row of an odd-N tail unit is clamped and never stored.
  auto unit_rows = [&](int unit, int* rows) {
    rows[0] = __builtin_amdgcn_readfirstlane(2 * unit);
    rows[1] = __builtin_amdgcn_readfirstlane(min(2 * unit + 1, N - 1));
    if (SWIGLU) {
      rows[R - 2] = __builtin_amdgcn_readfirstlane(N + 2 * unit);
      rows[R - 1] = __builtin_amdgcn_readfirstlane(N + min(2 * unit + 1, N - 1));
    }
  };
  // one batch of the weight stream: R rows x U chunks, issued in consumption order, indices clamped, never branched
  u32x4 w[R][U];
  auto issue = [&](int unit, int it0) {
    int rows[R];
    unit_rows(unit, rows);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const u32x4* p = reinterpret_cast<const u32x4*>(W + (size_t)rows[r] * K);
#pragma unroll
      for (int j = 0; j < U; ++j) {
        w[r][j] = __builtin_nontemporal_load(p + min((it0 + j) * 64 + lane, wchunks - 1));
        __builtin_amdgcn_sched_barrier(0);  // issue order == consumption order (see gemv_valu.h)
      }
    }
  };

  // x (RMSNormed) into LDS, the residual elements of the wave's first units (two columns each), the first weight batch
  gemv_valu_prologue<T, B, NXMAX, 2, SWIGLU>(x, norm_w, norm_eps, residual, N, K, xs, red, res_s,
                                             [&] { issue(min((int)blockIdx.x * 4 + wave, NUNIT - 1), 0); });

  int uk = 0;
  for (int unit = blockIdx.x * 4 + wave; unit < NUNIT; unit += gridDim.x * 4, ++uk) {
    int rows[R];
    unit_rows(unit, rows);
    // the row scales are requested BEFORE the weight stream (scalar loads): placed at their use they would queue behind
    // the weight loads and expose a memory latency per unit (same trap as the residual element, see gemv_valu.h)
    float sc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) sc[r] = wscale[rows[r]];
    float acc[R][B];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int b = 0; b < B; ++b) acc[r][b] = 0.f;

    for (int it0 = 0; it0 < nit; it0 += U) {
#pragma unroll
      for (int j = 0; j < U; ++j) {
        const int ch = (it0 + j) * 64 + lane;
        const bool valid = ch < wchunks;
        const int chc = valid ? ch : wchunks - 1;
        float xf[B][WVEC];
#pragma unroll
        for (int b = 0; b < B; ++b) {
          const u32x4 x0 = *reinterpret_cast<const u32x4*>(xs + (size_t)b * K + (size_t)chc * WVEC);
          const u32x4 x1 = *reinterpret_cast<const u32x4*>(xs + (size_t)b * K + (size_t)chc * WVEC + 8);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            xf[b][2 * q] = bf16lo(x0[q]);
            xf[b][2 * q + 1] = bf16hi(x0[q]);
            xf[b][8 + 2 * q] = bf16lo(x1[q]);
            xf[b][8 + 2 * q + 1] = bf16hi(x1[q]);
          }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int wq = valid ? (int)w[r][j][q] : 0;  // fp8 code 0 = +0.0
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(wq, false);
            const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(wq, true);
#pragma unroll
            for (int b = 0; b < B; ++b) {
              acc[r][b] = fmaf(lo[0], xf[b][4 * q], acc[r][b]);
              acc[r][b] = fmaf(lo[1], xf[b][4 * q + 1], acc[r][b]);
              acc[r][b] = fmaf(hi[0], xf[b][4 * q + 2], acc[r][b]);
              acc[r][b] = fmaf(hi[1], xf[b][4 * q + 3], acc[r][b]);
            }
          }
        }
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
      for (int r = 0; r < R; ++r) a[r] = wave_sum(acc[r][b]) * sc[r];
      if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int n = 2 * unit + r;
          if (n < N)
            gemv_valu_epilogue<T, SWIGLU>(a[r], a[R - 2 + r], residual, uk < GEMV_RES_MAXU ? &res_s[b][wave][2 * uk + r] : nullptr, out,
                                          (size_t)b * N + n, out_f32);
        }
      }
    }
  }
}

}  // namespace

// one row on the VALU kernel (GEMV_W8 of gemv_route.h), entered from srgpt_decode_product (gemv.hip)
int srgpt_gemv_w8_valu(const DecodeProduct& p, hipStream_t s) {
  const GemvValuLaunch l = gemv_valu_launch(GEMV_W8, p.batch, p.N, p.K, true, p.swiglu != 0, srgpt_device_cus());
  SRGPT_TRY((srgpt_switch<false, true>(p.swiglu != 0, "SWIGLU", [&](auto sw_c) {
    return srgpt_switch<1>(l.B, "B", [&](auto b_c) {
      return srgpt_switch<2, 8>(l.NX, "NX", [&](auto nx_c) {
        constexpr auto kfn = &gemv_w8_kernel<decltype(b_c)::value, decltype(sw_c)::value, decltype(nx_c)::value>;
        return gemv_valu_run<kfn>(l, "srgpt_gemv_w8: batch*K", s, (const T*)p.x, (const unsigned char*)p.W, p.wscale, (const T*)p.norm_w,
                                  p.eps, (const T*)p.residual, p.out, p.N, p.K, p.out_f32);
      });
    });
  })));
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}
