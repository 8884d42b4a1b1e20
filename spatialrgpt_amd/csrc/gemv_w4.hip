// Decode-path weight-streaming product with MXFP4 weights (W4A16): OCP e2m1 codes, one E8M0 scale byte per 32 values of a row
//   out[b, n] = round_bf16( sum_k x[b, k] * e2m1(W4[n, k]) * 2^(wscale8[n, k / 32] - 127) )       (HBM-bound, a quarter of the bf16 bytes)
// and the exact bf16 expansion of such a matrix (srgpt_dequant_mxfp4, what the prefill multiplies).
//
// Same structure as gemv_w8.hip (wave per unit, 1-KiB non-temporal wave loads issued in consumption order, branch-free consumption
// with clamped indices, x in LDS behind the fused RMSNorm prologue, residual elements and scales requested ahead of the weight
// stream, SwiGLU / residual / fp32-logit epilogues with the header's rounding points) with these differences:
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
  constexpr int VEC = 8;    // activation elements per 16-byte chunk
  constexpr int WVEC = 32;  // weight elements per 16-byte chunk = one MX block
  constexpr int C = W4_UNIT_COLS;    // output columns per unit
  constexpr int R = SWIGLU ? 2 * C : C;  // weight rows per unit (SwiGLU: C gate + C up rows -> C outputs)
  constexpr int U = 2;               // K-chunks per row per batch
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* xs = reinterpret_cast<T*>(smem);  // [B][K]
  __shared__ float red[16];
  constexpr int RES_MAXU = 4;  // residual elements of a wave's first 4 units are staged through LDS by the prologue
  constexpr int RSLOT = C * RES_MAXU;  // (unit, column-of-unit) slots per wave
  static_assert(B * 4 * RSLOT <= 256, "one thread per staged residual element");
  __shared__ float res_s[B][4][RSLOT];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunks = K / VEC;           // 16-byte activation chunks per row
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
        __builtin_amdgcn_sched_barrier(0);  // issue order == consumption order (see gemv.hip)
      }
    }
  };

  // ---- prologue: stage x (and RMSNorm it) into LDS: gemv_w8.hip's, with the residual slots of C-column units ----
  {
    const int total = B * nchunks;
    const bool do_norm = norm_w != nullptr;
    Vec16<T> xr[NXMAX], gr[NXMAX];
    // residual elements this block will need: fetched with the prologue's loads (see gemv_w8.hip)
    const int rb = tid / (4 * RSLOT), rw = (tid / RSLOT) & 3, rk = tid % RSLOT;
    const long long rcol = ((long long)blockIdx.x * 4 + rw + (long long)(rk / C) * gridDim.x * 4) * C + (rk % C);  // output column
    const bool rok = !SWIGLU && residual != nullptr && tid < B * 4 * RSLOT && rcol < N;
    const T res_raw = (residual != nullptr ? residual : x)[rok ? (size_t)rb * N + (size_t)rcol : 0];
#pragma unroll
    for (int j = 0; j < NXMAX; ++j) {
      const int c = (tid + 256 * j) % total;
      xr[j] = *reinterpret_cast<const Vec16<T>*>(x + (size_t)c * VEC);
      gr[j] = *reinterpret_cast<const Vec16<T>*>((do_norm ? norm_w : x) + (size_t)(c % nchunks) * VEC);
    }
    // first weight batch behind the prologue's own loads: its HBM latency overlaps the RMSNorm, the LDS staging and the barrier
    __builtin_amdgcn_sched_barrier(0);
    issue(min((int)blockIdx.x * 4 + wave, NUNIT - 1), 0);
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
      const int b = c / nchunks;
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
#pragma unroll
      for (int b = 0; b < B; ++b) rs[b] = rsqrtf(block_sum(ss[b], red) / (float)K + norm_eps);
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
        const int b = c / nchunks, kc = c - b * nchunks;
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
          if (n < N) {
            if (SWIGLU) {
              const float g = rnd<T>(a[c]), u = rnd<T>(a[C + c]);
              reinterpret_cast<T*>(out)[(size_t)b * N + n] = from_f<T>(rnd<T>(silu(g)) * u);
            } else {
              float v = rnd<T>(a[c]);
              if (residual)
                v = rnd<T>((uk < RES_MAXU ? res_s[b][wave][C * uk + c] : to_f(residual[(size_t)b * N + n])) + v);
              if (out_f32)
                reinterpret_cast<float*>(out)[(size_t)b * N + n] = v;
              else
                reinterpret_cast<T*>(out)[(size_t)b * N + n] = from_f<T>(v);
            }
          }
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

// one launch of up to W4_MAX_ROWS rows
int launch_gemv_w4(const void* x, const void* W4, const void* wscale8, const void* norm_w, float eps, const void* residual, void* out,
                   int B, int N, int K, int swiglu, int out_f32, hipStream_t s) {
  const GemvValuLaunch l = gemv_w4_launch(B, N, K, swiglu != 0, srgpt_device_cus());
  SRGPT_CHECK(l.lds <= GEMV_LDS_CAP, SRGPT_ERR_UNSUPPORTED, "srgpt_gemv_w4: batch*K too large for LDS (%zu bytes)", (size_t)l.lds);
  SRGPT_TRY((srgpt_switch<false, true>(swiglu != 0, "SWIGLU", [&](auto sw_c) {
    return srgpt_switch<1, 2, 3, 4>(l.B, "B", [&](auto b_c) {
      return srgpt_switch<2, 8>(l.NX, "NX", [&](auto nx_c) {
        constexpr auto kfn = &gemv_w4_kernel<decltype(b_c)::value, decltype(sw_c)::value, decltype(nx_c)::value>;
        return srgpt_launch_dyn_lds<kfn>(l.raise_lds_limit ? GEMV_LDS_CAP : 0, dim3(l.grid), dim3(256), (size_t)l.lds, s, (const T*)x,
                                         (const unsigned char*)W4, (const unsigned char*)wscale8, (const T*)norm_w, eps,
                                         (const T*)residual, out, N, K, out_f32);
      });
    });
  })));
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

}  // namespace

extern "C" int srgpt_gemv_w4(const void* x, const void* W4, const void* wscale8, const void* norm_w, float norm_eps,
                             const void* residual, void* out, int batch, int N, int K, int swiglu, int out_f32,
                             srgpt_stream_t stream) {
  SRGPT_CHECK(x && W4 && wscale8 && out, SRGPT_ERR_ARG, "srgpt_gemv_w4: null pointer");
  SRGPT_CHECK(N > 0 && K > 0 && batch > 0, SRGPT_ERR_ARG, "srgpt_gemv_w4: bad shape");
  SRGPT_CHECK(K % 32 == 0, SRGPT_ERR_ARG, "srgpt_gemv_w4: K=%d must be a multiple of 32 (one scale per 32 values)", K);
  SRGPT_CHECK(!(swiglu && (residual || out_f32)), SRGPT_ERR_ARG, "srgpt_gemv_w4: swiglu excludes residual/out_f32");
  SRGPT_CHECK((long long)N * (swiglu ? 2 : 1) <= 0x7fffffffLL / 2, SRGPT_ERR_ARG, "srgpt_gemv_w4: N=%d too large", N);
  const GemvRoute r = gemv_w4_route(batch);
  const size_t on = out_f32 ? sizeof(float) : sizeof(T);
  for (int b0 = 0; b0 < batch; b0 += r.chunk) {
    const int nb = batch - b0 < r.chunk ? batch - b0 : r.chunk;
    SRGPT_TRY(launch_gemv_w4((const char*)x + (size_t)b0 * K * sizeof(T), W4, wscale8, norm_w, norm_eps,
                             residual ? (const char*)residual + (size_t)b0 * N * sizeof(T) : nullptr, (char*)out + (size_t)b0 * N * on, nb,
                             N, K, swiglu, out_f32, as_stream(stream)));
  }
  return SRGPT_OK;
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
