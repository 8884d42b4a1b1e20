// Batch-1 decode product over bf16 weights stored in the lossless 13-bit code of pack13.h: 0.8125 of the bytes of gemv.hip's stream,
// and bit for bit its results.
//   out[n] = W[n, :] . x      with W[n, k] decoded from (sign, exponent-code, low byte) planes to exactly the bf16 the raw matrix holds
//
// gemv_kernel<bf16, 1, ...> of gemv.hip with another weight stream: the same unit / wave / grid decomposition (a unit = one output
// row, or a gate and an up row; a wave owns units grid-strided; 2 blocks per CU), the same prologue (gemv_valu.h: x staged -- and RMSNormed -- into
// LDS, the wave's first weight batch issued behind the prologue's own loads), the next batch issued before the reduction, and for
// every row the same fp32 accumulation: lane l adds the weights k = (it * 64 + l) * 8 + i, it ascending, i = 0 .. 7, then the same
// wave_sum and epilogue roundings.  Only how a lane comes by its 8 weights of iteration `it` differs:
//   * a batch is one group (4 iterations = 4 wave loads: 256 B of signs, 1 KiB of exponent nibbles, 2 x 1 KiB of low bytes,
//     non-temporal, issued in consumption order) of each of the unit's rows;
//   * per iteration two and-or-add sequences rebuild the eight high bytes, one v_perm_b32 per weight places high and low byte as the
//     fp32 the FMA takes (pack13.h) -- about 33 lane operations per 8 weights against the raw kernel's 24, well inside the VALU
//     time the HBM stream leaves;
//   * the activation row in LDS is zero-filled up to whole groups: the padding of a row whose K is not a multiple of 2048 decodes
//     to finite weights and adds +0.
// Exception rows (pack13.h: a row with a zero, a denormal, an Inf, a NaN, or a value below its window) are streamed from the raw
// matrix by the raw kernel's loop; a SwiGLU unit takes it if either of its rows is one.  The meta words of a wave's first 64 units
// are fetched with the prologue's loads, one per lane, and read back with a v_readlane per unit.
#include <stdlib.h>

#include "common.h"
#include "gemv_route.h"
#include "gemv_valu.h"
#include "internal.h"
#include "pack13.h"

namespace {

typedef bf16_t T;

template <bool SWIGLU, int NXMAX>
__global__ __launch_bounds__(256, 2) void gemv_p13_kernel(const T* __restrict__ x, const unsigned char* __restrict__ P,
                                                          const uint32_t* __restrict__ meta, const T* __restrict__ W,
                                                          const T* __restrict__ norm_w, float norm_eps, const T* __restrict__ residual,
                                                          void* __restrict__ out, int N, int K, int out_f32) {
  constexpr int VEC = 8;
  constexpr int R = SWIGLU ? 2 : 1;  // weight rows per unit
  constexpr int GI = P13_GROUP_ITS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* xs = reinterpret_cast<T*>(smem);  // [groups * 2048]: x, then zeros
  __shared__ float red[16];
  __shared__ float res_s[1][4][GEMV_RES_MAXU];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nchunks = K / VEC;         // 16-byte chunks of activations per row
  const int nit = nchunks >> 6;        // chunk iterations per row (K % 512 == 0)
  const int groups = (nit + GI - 1) / GI;
  const size_t row_bytes = (size_t)groups * P13_GROUP_BYTES;
  const int stride = (int)gridDim.x * 4;

  // one batch of the packed stream: one group of each of the unit's R rows, planes in consumption order (see gemv_valu.h: the
  // scheduling barriers pin issue order == consumption order, so the consumers get counted waits)
  uint32_t sg[R];
  u32x4 nb[R], lo[R][2];
  auto issue = [&](int unit, int g) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const unsigned char* prow = P + (size_t)(unit + r * N) * row_bytes;
      const unsigned char* pg = prow + (size_t)g * P13_GROUP_BYTES;
      sg[r] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(pg + P13_SIGN_OFF) + lane);
      __builtin_amdgcn_sched_barrier(0);
      nb[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(pg + P13_NIB_OFF) + lane);
      __builtin_amdgcn_sched_barrier(0);
      lo[r][0] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(pg + P13_LOW_OFF) + lane);
      __builtin_amdgcn_sched_barrier(0);
      lo[r][1] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(pg + P13_LOW_OFF + 1024) + lane);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // the meta words of the wave's units go out with the prologue's loads: lane l holds the word(s) of the wave's l-th unit
  uint32_t mw[R];
  {
    const long long mu = (long long)blockIdx.x * 4 + wave + (long long)lane * stride;
    const int mi = (int)(mu < N ? mu : N - 1);
#pragma unroll
    for (int r = 0; r < R; ++r) mw[r] = meta[mi + r * N];
  }
  // x (RMSNormed) into LDS and the residual elements of the wave's first units; behind the prologue's loads the first packed batch,
  // then the zero tail of the LDS row (no iteration when K % 2048 == 0; nothing the statistics wait for)
  gemv_valu_prologue<T, 1, NXMAX, 1, SWIGLU>(x, norm_w, norm_eps, residual, N, K, xs, red, res_s, [&] {
    issue(min((int)blockIdx.x * 4 + wave, N - 1), 0);
    for (int c = nchunks + tid; c < groups * (P13_GROUP_WEIGHTS / VEC); c += 256)
      *reinterpret_cast<u32x4*>(xs + (size_t)c * VEC) = u32x4{0u, 0u, 0u, 0u};
  });

  int uk = 0;
  for (int unit = blockIdx.x * 4 + wave; unit < N; unit += stride, ++uk) {
    float acc[R];
    uint32_t bb[R];  // the rows' base bytes (wave-uniform)
    bool exception = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      acc[r] = 0.f;
      bb[r] = uk < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)mw[r], uk) : meta[unit + r * N];
      exception = exception || bb[r] == P13_EXCEPTION;
    }

    if (!exception) {
      for (int g = 0; g < groups; ++g) {
#pragma unroll
        for (int t = 0; t < GI; ++t) {
          const int ch = (g * GI + t) * 64 + lane;
          const Vec16<T> xv = *reinterpret_cast<const Vec16<T>*>(xs + (size_t)ch * VEC);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            uint32_t high[R], low[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
              high[r] = p13_high4(sg[r], nb[r][t], bb[r], t, h);
              low[r] = lo[r][t >> 1][2 * (t & 1) + h];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float xf = xv.get(4 * h + j);
#pragma unroll
              for (int r = 0; r < R; ++r) acc[r] = fmaf(__uint_as_float(p13_f32_bits(high[r], low[r], j)), xf, acc[r]);
            }
          }
        }
        // the registers are free again: the next batch of this wave's stream (the row's next group, or the first group of its
        // next unit; past the last unit a valid row is re-read and dropped) goes out before the reduction and the store
        {
          const bool more = g + 1 < groups;
          issue(more ? unit : min(unit + stride, N - 1), more ? g + 1 : 0);
        }
      }
    } else {
      // the raw kernel's loop over the rows of the raw matrix; the packed batch issued for this unit is dropped
      // (batches of 8 loads like the raw kernel's, indices clamped: a synthetic gaussian matrix
      // has an exact zero in one row of a thousand, and a one-load-at-a-time loop made each of them the launch's tail)
      constexpr int RU = 8 / R;
      for (int it0 = 0; it0 < nit; it0 += RU) {
        u32x4 wv[R][RU];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < RU; ++j)
            wv[r][j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(W + (size_t)(unit + r * N) * K) +
                                                  min(it0 + j, nit - 1) * 64 + lane);
#pragma unroll
        for (int j = 0; j < RU; ++j) {
          if (it0 + j >= nit) break;  // wave-uniform: the clamped re-reads past the row are dropped, not added as zeros
          const Vec16<T> xv = *reinterpret_cast<const Vec16<T>*>(xs + (size_t)(min(it0 + j, nit - 1) * 64 + lane) * VEC);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float x0 = xv.get(2 * q), x1 = xv.get(2 * q + 1);
#pragma unroll
            for (int r = 0; r < R; ++r) {
              const unsigned int wq = wv[r][j][q];
              acc[r] = fmaf(bf16lo(wq), x0, acc[r]);
              acc[r] = fmaf(bf16hi(wq), x1, acc[r]);
            }
          }
        }
      }
      issue(min(unit + stride, N - 1), 0);
    }

    float a[R];
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = wave_sum(acc[r]);
    if (lane == 0)
      gemv_valu_epilogue<T, SWIGLU>(a[0], a[R - 1], residual, uk < GEMV_RES_MAXU ? &res_s[0][wave][uk] : nullptr, out, (size_t)unit, out_f32);
  }
}

}  // namespace

extern "C" int srgpt_gemv_p13(const void* x, const void* packed, const void* flags, const void* W_raw, const void* norm_w, float norm_eps,
                              const void* residual, void* out, int N, int K, int swiglu, int out_f32, srgpt_stream_t stream) {
  SRGPT_CHECK(x && packed && flags && W_raw && out, SRGPT_ERR_ARG, "srgpt_gemv_p13: null pointer");
  SRGPT_CHECK(N > 0 && K > 0, SRGPT_ERR_ARG, "srgpt_gemv_p13: bad shape");
  SRGPT_CHECK(gemv_p13_eligible(1, K), SRGPT_ERR_ARG, "srgpt_gemv_p13: K=%d must be a multiple of 512 (whole 64-lane chunk iterations)", K);
  SRGPT_CHECK(!(swiglu && (residual || out_f32)), SRGPT_ERR_ARG, "srgpt_gemv_p13: swiglu excludes residual/out_f32");
  SRGPT_CHECK((long long)N * (swiglu ? 2 : 1) <= 0x7fffffffLL / 2, SRGPT_ERR_ARG, "srgpt_gemv_p13: N=%d too large", N);
  const GemvValuLaunch l = gemv_p13_launch(N, K, srgpt_device_cus());
  hipStream_t s = as_stream(stream);
  const auto go = [&](auto sw_c, auto nx_c) {
    constexpr auto kfn = &gemv_p13_kernel<decltype(sw_c)::value, decltype(nx_c)::value>;
    return gemv_valu_run<kfn>(l, "srgpt_gemv_p13: K", s, (const T*)x, (const unsigned char*)packed, (const uint32_t*)flags, (const T*)W_raw,
                              (const T*)norm_w, norm_eps, (const T*)residual, out, N, K, out_f32);
  };
  SRGPT_TRY((srgpt_switch<2, 8>(l.NX, "NX", [&](auto nx_c) {
    return swiglu ? go(std::true_type{}, nx_c) : go(std::false_type{}, nx_c);
  })));
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}
