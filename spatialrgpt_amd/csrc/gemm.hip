// GEMM family: C[M,N] = act(A[M,K] @ W[N,K]^T + bias) + residual      (see include/srgpt.h)
//
// bf16: LDS-tiled MFMA kernel (v_mfma_f32_32x32x16_bf16), 256 threads = 4 waves, BK = 64,
//       direct-to-LDS staging, XOR-swizzled 16-byte LDS slots: slot ^ ((row >> 1) & 7) -- with 128-byte rows the
//       16 lanes of a ds_read_b128 pass (16 consecutive rows, one slot) then cover all 64 banks exactly once (the row's
//       parity picks the 128-byte half, the swizzled slot the 16 bytes within it); slot ^ (row & 7) left rows r and r + 8
//       on the same banks: SQ_LDS_BANK_CONFLICT was 50 % of SQ_LDS_IDX_ACTIVE, fused epilogue (bias / activation / residual / deconv pixel-shuffle / fp32 out).
//       Both operands are K-contiguous (nn.Linear weight layout), so A and W tiles stage identically.
// fp32: plain LDS-tiled FMA kernel; exists for tight-tolerance parity runs of the same host path.
#include <stdlib.h>

#include "common.h"
#include "gemm_epilogue.h"
#include "gemm_route.h"
#include "internal.h"

namespace {

constexpr int BK = 64;  // bf16 elements per K tile = 8 slots of 16 B

// ------------------------------------------------------------------------------------------------
// bf16 MFMA kernel, direct-to-LDS staging (global_load_lds_dwordx4): no staging VGPRs, no ds_write pass, single LDS
// buffer (BM+BN) x 128 B -> 3 blocks per CU at 128x128, whose independent K loops overlap each other's barriers.
// A wave-instruction moves 8 rows x 128 B into 1 KiB of LDS at (wave-uniform base + lane * 16); the XOR slot swizzle
// (see the top of the file) is kept by permuting WHICH 16-byte chunk of its row a lane fetches (chunk = slot ^ ((row >> 1) & 7)),
// so the fragment reads below are the same conflict-free ds_read_b128.  Rows past M / N re-read the last valid row
// (their outputs are never stored); a ragged last K tile (K % 64 != 0) is staged through registers with zero fill.
// ------------------------------------------------------------------------------------------------
// NBUF = 1: single buffer, two barriers per K tile, overlap comes from the other blocks of the CU (large grids).
// NBUF = 2: the next tile's LDS-DMA is issued before the current tile is multiplied, one barrier per K tile -- for grids that
//           leave a CU with only 1-2 blocks (the M = 259 prefill and ViT shapes), where each K step would otherwise pay a
//           full memory latency.
//
// W4: the weight operand is row-major MXFP4 codes [N, K / 2] + E8M0 bytes [N, K / 32] (include/srgpt.h), K % 64 == 0.  The code tile
// of a K tile is BN rows x 32 B = 8 dwords per row, a dword = the 8 codes of one MFMA fragment (k = 16 ks + 8 (lane >> 5) .. + 8):
// LDS-DMA with 4 bytes per lane moves 8 rows x 32 B per wave-instruction (the same GW requests per wave, the same lane >> 3 /
// lane & 7 mapping), a fragment is one ds_read_b32 + four v_cvt_scalef32_pk_bf16_fp4 with the block scale `byte << 23` (exact), and
// the two scale bytes a row needs per K tile are loaded from global memory by the lanes that multiply the row, one tile ahead
// when double-buffered.  Dword swizzle: slot ^ ((row >> 2) & 7) -- a ds_read_b32 resolves banks (dword address mod 32) per 32-lane
// half, a half reads 32 consecutive rows at one slot = dword 8 row + slot', and for a fixed row & 3 the eight row >> 2 give eight
// different slot' (SQ_LDS_BANK_CONFLICT 0; slot ^ (((row >> 3) & 3) << 1), derived for 64 banks, measured half of the W reads'
// cycles as conflicts); the source side permutes which dword a lane fetches ((row >> 2) & 7 = ((wave & 3) << 1) | (lane >> 5) for
// every group of a wave).  The k of every step, the MFMA, the accumulators, the split ranges and the epilogue are the bf16
// instance's, so the product equals it on srgpt_dequant_mxfp4 of the codes bit for bit.  The mode is the presence of the trailing scale-pointer argument (a parameter pack of
// zero or one `const unsigned char*`; W then points at the codes): the bf16 instantiation keeps its parameter list and compiles to the
// instructions it had without this mode (a body shared through a __device__ function did not: checked on the disassembly).
template <int BM, int BN, int NBUF, typename... Scale8>
__global__ __launch_bounds__(256, NBUF == 1 ? 3 : 2) void gemm_bf16_glds(const bf16_t* __restrict__ A, const bf16_t* __restrict__ W,
                                                                         int K, int lda, Epilogue e, Scale8... scale8) {
  constexpr bool W4 = sizeof...(Scale8) == 1;
  static_assert(sizeof...(Scale8) <= 1, "at most one scale pointer");
  // wave layout: 2 x 2 waves of (BM/2) x (BN/2) when BM is a multiple of 64; BM = 96 (three 32-row MFMA tiles -- 259 rows pad to
  // 288 instead of 320 and a tile step moves 17.8 instead of 23.4 bytes per kFLOP through the fill path that bounds this kernel):
  // 1 x 4 waves of 96 x (BN/4)
  constexpr int WAVES_M = BM % 64 == 0 ? 2 : 1, WAVES_N = 4 / WAVES_M;
  constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;  // rows / columns of a wave's sub-tile
  constexpr int TM = WTM / 32, TN = WTN / 32;
  static_assert(TM * 32 * WAVES_M == BM && TN * 32 * WAVES_N == BN && BM % 32 == 0 && BN % 32 == 0, "tile / wave layout");
  constexpr int WROW = W4 ? BK / 4 : BK;    // bf16-sized elements a W row takes in LDS (W4: 32 bytes of codes)
  constexpr int TILE = BM * BK + BN * WROW;  // elements per stage buffer
  __shared__ __attribute__((aligned(1024))) bf16_t lds[NBUF * TILE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = WAVES_M == 2 ? wave >> 1 : 0, wn = WAVES_M == 2 ? wave & 1 : wave;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  // row within the 8-row group; logical chunk this lane fetches = physical slot ^ swz(row), swz(row) = (row >> 1) & 7
  // (group base rows are multiples of 8: (row >> 1) & 7 = ((wave & 1) << 2) | (lr >> 1) for every group of this wave)
  const int lr = lane >> 3, lc = (lane & 7) ^ (((wave & 1) << 2) | (lr >> 1));

  const int nk_all = (K + BK - 1) / BK;
  const int kt0 = e.splits > 1 ? (int)blockIdx.z * e.tiles_per_split : 0;
  const int nk = e.splits > 1 ? min(nk_all, kt0 + e.tiles_per_split) : nk_all;

  // per-lane row base pointers (clamped rows), one per 8-row group this wave stages
  constexpr int GA = BM / 32, GW = BN / 32;  // groups per wave (4 waves x 8 rows)
  const bf16_t* pa[GA];
  const bf16_t* pw[GW];
#pragma unroll
  for (int i = 0; i < GA; ++i) pa[i] = A + (size_t)min(m0 + (wave + 4 * i) * 8 + lr, e.M - 1) * lda + lc * 8;
#pragma unroll
  for (int i = 0; i < GW; ++i) {
    const size_t row = (size_t)min(n0 + (wave + 4 * i) * 8 + lr, e.N - 1);
    // W4: byte offsets in bf16_t units -- a row is K / 2 bytes = K / 4 elements, the lane's dword is slot ^ ((row >> 2) & 7)
    pw[i] = W4 ? W + row * (K / 4) + ((lane & 7) ^ (((wave & 3) << 1) | (lr >> 2))) * 2 : W + row * K + lc * 8;
  }
  // W4: the E8M0 bytes of the rows this lane multiplies (clamped like the rows themselves); sc[j] = bytes 2 kt, 2 kt + 1 of row j
  const unsigned char* ps[TN];
  unsigned int sc_cur[TN] = {}, sc_nxt[TN] = {};
  if constexpr (W4) {
    const unsigned char* wscale8 = (scale8, ...);
#pragma unroll
    for (int j = 0; j < TN; ++j) ps[j] = wscale8 + (size_t)min(n0 + wn * WTN + j * 32 + (lane & 31), e.N - 1) * (K / 32);
  }
  auto load_scales = [&](int kt, unsigned int* sc) {
#pragma unroll
    for (int j = 0; j < TN; ++j) sc[j] = (unsigned int)ps[j][2 * kt] | ((unsigned int)ps[j][2 * kt + 1] << 8);
  };

  auto stage = [&](int kt, int buf) {
    bf16_t* As = lds + buf * TILE;
    bf16_t* Ws = As + BM * BK;
    const int k0 = kt * BK;
    if (W4 || k0 + BK <= K) {  // (W4: K % 64 == 0, no ragged tile)
#pragma unroll
      for (int i = 0; i < GA; ++i)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pa[i] + k0),
                                         (__attribute__((address_space(3))) void*)(As + (wave + 4 * i) * 8 * BK), 16, 0, 0);
#pragma unroll
      for (int i = 0; i < GW; ++i) {
        if constexpr (W4)
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pw[i] + k0 / 4),
                                           (__attribute__((address_space(3))) void*)(Ws + (wave + 4 * i) * 8 * WROW), 4, 0, 0);
        else
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pw[i] + k0),
                                           (__attribute__((address_space(3))) void*)(Ws + (wave + 4 * i) * 8 * BK), 16, 0, 0);
      }
    } else {  // ragged last tile: zero-filled through registers, same swizzled slots
      const bool ok = k0 + lc * 8 < K;
#pragma unroll
      for (int i = 0; i < GA; ++i) {
        const u32x4 v = ok ? *reinterpret_cast<const u32x4*>(pa[i] + k0) : u32x4{0, 0, 0, 0};
        *reinterpret_cast<u32x4*>(As + ((wave + 4 * i) * 8 + lr) * BK + ((lane & 7) << 3)) = v;
      }
#pragma unroll
      for (int i = 0; i < GW; ++i) {
        const u32x4 v = ok ? *reinterpret_cast<const u32x4*>(pw[i] + k0) : u32x4{0, 0, 0, 0};
        *reinterpret_cast<u32x4*>(Ws + ((wave + 4 * i) * 8 + lr) * BK + ((lane & 7) << 3)) = v;
      }
    }
  };

  f32x16 acc[TM][TN];
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = zero16;

  auto compute = [&](int buf, const unsigned int* sc) {
    const bf16_t* As = lds + buf * TILE;
    const bf16_t* Ws = As + BM * BK;
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      bf16x8 fa[TM], fw[TN];
      const int slot = ks * 2 + (lane >> 5);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int r = wm * WTM + i * 32 + (lane & 31);
        fa[i] = *reinterpret_cast<const bf16x8*>(As + r * BK + ((slot ^ ((r >> 1) & 7)) << 3));
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int r = wn * WTN + j * 32 + (lane & 31);
        if constexpr (W4) {
          const unsigned int word = *reinterpret_cast<const unsigned int*>(Ws + r * WROW + ((slot ^ ((r >> 2) & 7)) << 1));
          const float s = __uint_as_float(((sc[j] >> (8 * (ks >> 1))) & 0xffu) << 23);  // k steps 0, 1: block 2 kt; 2, 3: 2 kt + 1
          u32x4 o;
          o[0] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, s, 0));
          o[1] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, s, 1));
          o[2] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, s, 2));
          o[3] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, s, 3));
          fw[j] = __builtin_bit_cast(bf16x8, o);
        } else {
          fw[j] = *reinterpret_cast<const bf16x8*>(Ws + r * BK + ((slot ^ ((r >> 1) & 7)) << 3));
        }
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fw[j], acc[i][j], 0, 0, 0);
    }
  };
  if (NBUF == 1) {
    for (int kt = kt0; kt < nk; ++kt) {
      stage(kt, 0);
      if constexpr (W4) load_scales(kt, sc_cur);
      __syncthreads();  // carries the vmcnt(0) that lands the LDS-DMA
      compute(0, sc_cur);
      __syncthreads();  // every wave is done reading before the next tile overwrites the buffer
    }
  } else {
    stage(kt0, 0);
    if constexpr (W4) load_scales(kt0, sc_cur);
    for (int kt = kt0; kt < nk; ++kt) {
      const int cur = (kt - kt0) & 1;
      __syncthreads();  // tile kt has landed (vmcnt(0)); every wave has finished tile kt-1, so the other buffer is free
      if (kt + 1 < nk) {
        stage(kt + 1, cur ^ 1);
        if constexpr (W4) load_scales(kt + 1, sc_nxt);
      }
      compute(cur, sc_cur);
      if constexpr (W4) {
#pragma unroll
        for (int j = 0; j < TN; ++j) sc_cur[j] = sc_nxt[j];
      }
    }
  }

  // D layout: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma clang loop unroll(full)
  for (int i = 0; i < TM; ++i)
#pragma clang loop unroll(full)
    for (int j = 0; j < TN; ++j) {
      const f32x16 a = acc[i][j];
      const int n = n0 + wn * WTN + j * 32 + (lane & 31);
      const int mb = m0 + wm * WTM + i * 32 + 4 * (lane >> 5);
      if (e.splits > 1) {
        float* slab = e.partial + (size_t)blockIdx.z * e.M * e.N;
#pragma clang loop unroll(full)
        for (int r = 0; r < 16; ++r) {
          const int m = mb + (r & 3) + 8 * (r >> 2);
          if (m < e.M && n < e.N) slab[(size_t)m * e.N + n] = a[r];
        }
      } else {
        epilogue_tile32<bf16_t>(e, mb, n, a);
      }
    }
}

// split-K second pass: fixed-order sum of the fp32 slabs, then the fused epilogue
template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(Epilogue e) {
  const size_t total = (size_t)e.M * e.N;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    float acc = 0.f;
    for (int z = 0; z < e.splits; ++z) acc += e.partial[(size_t)z * total + i];
    const int m = (int)(i / e.N), n = (int)(i - (size_t)m * e.N);
    epilogue_store<T>(e, m, n, acc);
  }
}

// The same pass, four columns per thread (N % 4 == 0, plain row-major output, bias / residual not periodic): the slabs are read
// with 16-byte loads, all splits of a thread in flight together (the scalar form above paid a 4-byte load and a 2-byte store per
// element: 11 us per reduction at M = 259, N = 4096), bias and residual as 8-byte loads, one 8-byte (bf16) / 16-byte (fp32) store.
// Same summation order, same rounding points.
template <typename T, int MAXS>
__global__ __launch_bounds__(256) void splitk_reduce4_kernel(Epilogue e) {
  const size_t total4 = (size_t)e.M * e.N / 4;
  const int n4 = e.N / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
    f32x4 p[MAXS];
#pragma unroll
    for (int z = 0; z < MAXS; ++z)
      p[z] = *reinterpret_cast<const f32x4*>(e.partial + (size_t)min(z, e.splits - 1) * (total4 * 4) + i * 4);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int z = 0; z < MAXS; ++z)
      if (z < e.splits) acc += p[z];
    const int m = (int)(i / n4), n = (int)(i - (size_t)m * n4) * 4;
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = e.wscale ? acc[q] * e.wscale[n + q] : acc[q];
    if (e.bias) {
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] += to_f(reinterpret_cast<const T*>(e.bias)[n + q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = rnd<T>(v[q]);  // nn.Linear / conv output is materialised in T
    if (e.act != SRGPT_ACT_NONE) {
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = rnd<T>(apply_act<T>(v[q], e.act));
    }
    if (e.residual) {
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = rnd<T>(v[q] + to_f(reinterpret_cast<const T*>(e.residual)[(size_t)m * e.N + n + q]));
    }
    const size_t off = (size_t)m * e.ldc + n;
    if (e.out_f32) {
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(e.C) + off) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
      bf16x4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = (bf16_t)v[q];
      static_assert(sizeof(T) == 2, "splitk_reduce4_kernel stores bf16 or fp32");
      *reinterpret_cast<bf16x4*>(reinterpret_cast<T*>(e.C) + off) = o;
    }
  }
}

// The same pass with the norm of the finished rows behind it (LlamaDecoderLayer: o_proj / down_proj + residual, then the next
// RMSNorm -- modeling_llama.py:611-684; the ViT encoder layer: out_proj / fc2 + residual, then the next LayerNorm): one block per
// row, thread t owns the 8-element chunks t, t + 256, ... exactly as rmsnorm_kernel / layernorm_kernel (norm.hip) do, sums the slabs
// in slab order, applies the epilogue with reduce4's roundings, stores the row of C, and runs the norm's statistics over the
// ROUNDED values in the norm kernels' element order through the same block_sum -- so C and the normalised row are bit-identical to
// [splitk_reduce4_kernel -> rmsnorm_kernel / layernorm_kernel], one launch and one read of the row less.
template <int MAXS, int CH>  // CH chunks of 8 per thread: N <= 2048 * CH
__global__ __launch_bounds__(256) void splitk_reduce_norm_kernel(Epilogue e) {
  __shared__ float red[16];
  const int m = blockIdx.x, nch = e.N / 8;
  const size_t total = (size_t)e.M * e.N;
  float x[CH][8];
  float ssq = 0.f, sum = 0.f;  // rmsnorm_kernel's / layernorm_kernel's first accumulation, in their element order
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int c = threadIdx.x + 256 * k;
    if (c < nch) {
      const int n = c * 8;
      f32x4 p[MAXS][2];
#pragma unroll
      for (int z = 0; z < MAXS; ++z) {
        const float* src = e.partial + (size_t)min(z, e.splits - 1) * total + (size_t)m * e.N + n;
        p[z][0] = *reinterpret_cast<const f32x4*>(src);
        p[z][1] = *reinterpret_cast<const f32x4*>(src + 4);
      }
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int z = 0; z < MAXS; ++z)
        if (z < e.splits) {
          a0 += p[z][0];
          a1 += p[z][1];
        }
      float v[8];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[q] = a0[q];
        v[4 + q] = a1[q];
      }
      if (e.wscale) {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] *= e.wscale[n + q];
      }
      if (e.bias) {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] += to_f(reinterpret_cast<const bf16_t*>(e.bias)[n + q]);
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = rnd<bf16_t>(v[q]);
      if (e.act != SRGPT_ACT_NONE) {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = rnd<bf16_t>(apply_act<bf16_t>(v[q], e.act));
      }
      if (e.residual) {
        const Vec16<bf16_t> r = *reinterpret_cast<const Vec16<bf16_t>*>(reinterpret_cast<const bf16_t*>(e.residual) + (size_t)m * e.N + n);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = rnd<bf16_t>(v[q] + r.get(q));
      }
      Vec16<bf16_t> o;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        o.set(q, v[q]);
        x[k][q] = v[q];
        ssq += v[q] * v[q];
        sum += v[q];
      }
      *reinterpret_cast<Vec16<bf16_t>*>(reinterpret_cast<bf16_t*>(e.C) + (size_t)m * e.ldc + n) = o;
    }
  }
  if (e.norm_kind == SRGPT_NORM_RMS) {
    const float r = rsqrtf(block_sum(ssq, red) / (float)e.N + e.norm_eps);
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int c = threadIdx.x + 256 * k;
      if (c < nch) {
        const Vec16<bf16_t> g = *reinterpret_cast<const Vec16<bf16_t>*>(reinterpret_cast<const bf16_t*>(e.norm_w) + c * 8);
        Vec16<bf16_t> o;
#pragma unroll
        for (int q = 0; q < 8; ++q) o.set(q, g.get(q) * rnd<bf16_t>(x[k][q] * r));  // weight * h.to(input_dtype)
        *reinterpret_cast<Vec16<bf16_t>*>(reinterpret_cast<bf16_t*>(e.norm_y) + (size_t)m * e.N + c * 8) = o;
      }
    }
  } else {  // LayerNorm: layernorm_kernel's three passes over the row, from registers
    const float mean = block_sum(sum, red) / (float)e.N;
    float qv = 0.f;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int c = threadIdx.x + 256 * k;
      if (c < nch) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float d = x[k][q] - mean;
          qv += d * d;
        }
      }
    }
    const float rstd = rsqrtf(block_sum(qv, red) / (float)e.N + e.norm_eps);
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int c = threadIdx.x + 256 * k;
      if (c < nch) {
        const Vec16<bf16_t> g = *reinterpret_cast<const Vec16<bf16_t>*>(reinterpret_cast<const bf16_t*>(e.norm_w) + c * 8);
        const Vec16<bf16_t> be = *reinterpret_cast<const Vec16<bf16_t>*>(reinterpret_cast<const bf16_t*>(e.norm_b) + c * 8);
        Vec16<bf16_t> o;
#pragma unroll
        for (int q = 0; q < 8; ++q) o.set(q, (x[k][q] - mean) * rstd * g.get(q) + be.get(q));
        *reinterpret_cast<Vec16<bf16_t>*>(reinterpret_cast<bf16_t*>(e.norm_y) + (size_t)m * e.N + c * 8) = o;
      }
    }
  }
}

// The slab reduction of the prefill's q/k/v projection with rope_kv_append_kernel (misc.hip) behind it: one block per token row, the
// reduced row (rounded to bf16 as the plain reduction stores it) goes to LDS, then every (head, pair) is rotated with
// rope_kv_append_kernel's arithmetic -- q back into the q/k/v buffer, k into the cache at the token's position -- and v is copied
// into the cache.  The un-rotated k and the v columns are stored to the q/k/v buffer as well, so every byte the two launches write
// is the same (tests compare all three buffers).
template <int MAXS>
__global__ __launch_bounds__(256) void splitk_reduce_rope_kernel(Epilogue e) {
  extern __shared__ __attribute__((aligned(16))) bf16_t rrow[];
  const int m = blockIdx.x, nch = e.N / 8;
  const size_t total = (size_t)e.M * e.N;
  const int D = e.rope_D, half = D >> 1, Hq = e.rope_Hq, Hkv = e.rope_Hkv;
  for (int c = threadIdx.x; c < nch; c += 256) {
    const int n = c * 8;
    f32x4 p[MAXS][2];
#pragma unroll
    for (int z = 0; z < MAXS; ++z) {
      const float* src = e.partial + (size_t)min(z, e.splits - 1) * total + (size_t)m * e.N + n;
      p[z][0] = *reinterpret_cast<const f32x4*>(src);
      p[z][1] = *reinterpret_cast<const f32x4*>(src + 4);
    }
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int z = 0; z < MAXS; ++z)
      if (z < e.splits) {
        a0 += p[z][0];
        a1 += p[z][1];
      }
    Vec16<bf16_t> o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      o.set(q, a0[q]);
      o.set(4 + q, a1[q]);
    }
    *reinterpret_cast<Vec16<bf16_t>*>(rrow + n) = o;
    if (n >= Hq * D) *reinterpret_cast<Vec16<bf16_t>*>(reinterpret_cast<bf16_t*>(e.C) + (size_t)m * e.ldc + n) = o;  // k (un-rotated), v
  }
  __syncthreads();
  const int b = m / e.rope_T, t = m - b * e.rope_T;
  const int pos = (e.rope_pos0 ? e.rope_pos0[b] : 0) + t;
  const bf16_t* cos_tab = reinterpret_cast<const bf16_t*>(e.rope_cos);
  const bf16_t* sin_tab = reinterpret_cast<const bf16_t*>(e.rope_sin);
  bf16_t* qrow = reinterpret_cast<bf16_t*>(e.C) + (size_t)m * e.ldc;
  const int nrot = (Hq + Hkv) * half;
  for (int w = threadIdx.x; w < nrot; w += 256) {
    const int h = w / half, i = w - h * half;
    const float c = to_f(cos_tab[(size_t)pos * half + i]), s = to_f(sin_tab[(size_t)pos * half + i]);
    const float x1 = to_f(rrow[h * D + i]), x2 = to_f(rrow[h * D + i + half]);
    // q*cos + rotate_half(q)*sin with every intermediate materialised in bf16
    const float o1 = rnd<bf16_t>(rnd<bf16_t>(x1 * c) + rnd<bf16_t>(-x2 * s));
    const float o2 = rnd<bf16_t>(rnd<bf16_t>(x2 * c) + rnd<bf16_t>(x1 * s));
    bf16_t* dst = h < Hq ? qrow + (size_t)h * D
                         : reinterpret_cast<bf16_t*>(e.rope_k) + (((size_t)b * Hkv + (h - Hq)) * e.rope_max_pos + pos) * D;
    dst[i] = from_f<bf16_t>(o1);
    dst[i + half] = from_f<bf16_t>(o2);
  }
  const bf16_t* vsrc = rrow + (size_t)(Hq + Hkv) * D;
  bf16_t* vc = reinterpret_cast<bf16_t*>(e.rope_v);
  for (int w = threadIdx.x; w < Hkv * D; w += 256) {
    const int h = w / D, i = w - h * D;
    vc[(((size_t)b * Hkv + h) * e.rope_max_pos + pos) * D + i] = vsrc[w];
  }
}

// launches the reduction that fits the epilogue (returns through SRGPT_LAUNCH_CHECK at the call site); true when the norm / RoPE
// the epilogue asks for went into it
template <typename T>
static inline bool launch_splitk_reduce(const Epilogue& e, hipStream_t s) {
  const size_t total = (size_t)e.M * e.N;
  const bool vec4 = e.N % 4 == 0 && e.ldc % 4 == 0 && e.out_mode != SRGPT_OUT_DECONV2X && e.bias_mod <= 0 && e.res_mod <= 0 &&
                    e.splits <= 8 && ((uintptr_t)e.C % 16 == 0);
// MAXS = the 4 or 8 slabs a thread of the vectorised kernels keeps in flight
#define SRGPT_FOR_MAXS(LAUNCH)  \
  do {                          \
    if (e.splits <= 4) {        \
      constexpr int MAXS = 4;   \
      LAUNCH;                   \
    } else {                    \
      constexpr int MAXS = 8;   \
      LAUNCH;                   \
    }                           \
  } while (0)
  if (e.rope_k && std::is_same<T, bf16_t>::value && vec4 && !e.out_f32 && !e.bias && !e.residual && !e.wscale &&
      e.act == SRGPT_ACT_NONE && e.N % 8 == 0 && e.ldc % 8 == 0 && e.N <= 24576) {
    const size_t lds = (size_t)e.N * sizeof(bf16_t);  // <= 48 KB
    SRGPT_FOR_MAXS(hipLaunchKernelGGL((splitk_reduce_rope_kernel<MAXS>), dim3(e.M), dim3(256), lds, s, e));
    return true;
  }
  if (e.norm_y && std::is_same<T, bf16_t>::value && vec4 && !e.out_f32 && e.N % 8 == 0 && e.ldc % 8 == 0 && e.N <= 8192 &&
      ((uintptr_t)e.norm_y % 16 == 0) && ((uintptr_t)e.norm_w % 16 == 0) && (!e.norm_b || (uintptr_t)e.norm_b % 16 == 0) &&
      (!e.residual || (uintptr_t)e.residual % 16 == 0)) {
    if (e.N > 4096) SRGPT_FOR_MAXS(hipLaunchKernelGGL((splitk_reduce_norm_kernel<MAXS, 4>), dim3(e.M), dim3(256), 0, s, e));
    else SRGPT_FOR_MAXS(hipLaunchKernelGGL((splitk_reduce_norm_kernel<MAXS, 2>), dim3(e.M), dim3(256), 0, s, e));
    return true;
  }
  if (vec4) {
    int rgrid = (int)((total / 4 + 255) / 256);
    if (rgrid > 2048) rgrid = 2048;
    SRGPT_FOR_MAXS(hipLaunchKernelGGL((splitk_reduce4_kernel<T, MAXS>), dim3(rgrid), dim3(256), 0, s, e));
    return false;
  }
#undef SRGPT_FOR_MAXS
  int rgrid = (int)((total + 255) / 256);
  if (rgrid > 2048) rgrid = 2048;
  hipLaunchKernelGGL(splitk_reduce_kernel<T>, dim3(rgrid), dim3(256), 0, s, e);
  return false;
}

// ------------------------------------------------------------------------------------------------
// fp32 FMA kernel (parity path): 64x64 tile, BK 16, each thread 4x4 outputs
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gemm_f32_simple(const float* __restrict__ A, const float* __restrict__ W,
                                                       int K, int lda, Epilogue e) {
  constexpr int BM = 64, BN = 64, BKF = 16;
  __shared__ float As[BKF][BM + 4];
  __shared__ float Ws[BKF][BN + 4];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  float acc[4][4] = {};
  const int lr = tid >> 2, lc = (tid & 3) * 4;  // 64 rows x 4 float4 per tile
  for (int k0 = 0; k0 < K; k0 += BKF) {
    {
      const int m = m0 + lr, k = k0 + lc;
      f32x4 v = {0, 0, 0, 0};
      if (m < e.M && k < K) v = *reinterpret_cast<const f32x4*>(A + (size_t)m * lda + k);
#pragma unroll
      for (int i = 0; i < 4; ++i) As[lc + i][lr] = v[i];
      const int n = n0 + lr;
      f32x4 u = {0, 0, 0, 0};
      if (n < e.N && k < K) u = *reinterpret_cast<const f32x4*>(W + (size_t)n * K + k);
#pragma unroll
      for (int i = 0; i < 4; ++i) Ws[lc + i][lr] = u[i];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < BKF; ++kk) {
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[kk][ty * 4 + i];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = Ws[kk][tx * 4 + j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) epilogue_store<float>(e, m0 + ty * 4 + i, n0 + tx * 4 + j, acc[i][j]);
}

// ------------------------------------------------------------------------------------------------
// fp8-weight fallback for K that is not a multiple of 64 (tiny test geometries): 64x64 tile, BK 16, scalar loads, fp32 FMA
// on the exactly widened operands -- correctness first, any K
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gemm_w8_simple(const bf16_t* __restrict__ A, const unsigned char* __restrict__ W8,
                                                      int K, int lda, Epilogue e) {
  constexpr int BM = 64, BN = 64, BKF = 16;
  __shared__ float As[BKF][BM + 4];
  __shared__ float Ws[BKF][BN + 4];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  float acc[4][4] = {};
  const int lr = tid >> 2, lc = (tid & 3) * 4;  // 64 rows x 4 groups of 4 k per tile
  for (int k0 = 0; k0 < K; k0 += BKF) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = k0 + lc + i;
      const int m = m0 + lr, n = n0 + lr;
      As[lc + i][lr] = (m < e.M && k < K) ? to_f(A[(size_t)m * lda + k]) : 0.f;
      float wv = 0.f;
      if (n < e.N && k < K) {
        const int code = W8[(size_t)n * K + k];
        wv = __builtin_amdgcn_cvt_pk_f32_fp8(code, false)[0];
      }
      Ws[lc + i][lr] = wv;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < BKF; ++kk) {
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[kk][ty * 4 + i];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = Ws[kk][tx * 4 + j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) epilogue_store<bf16_t>(e, m0 + ty * 4 + i, n0 + tx * 4 + j, acc[i][j]);
}

}  // namespace

// ---- split-K on the host, for every product of this file and of gemm_f8.hip (internal.h): the route's split goes into the
//      epilogue in front of the launch ...
void srgpt_splitk_apply(Epilogue& e, const GemmRoute& r, void* ws) {
  if (r.splits <= 1) return;
  e.partial = reinterpret_cast<float*>(ws);
  e.tiles_per_split = r.tiles_per_split;
  e.splits = r.splits;
}

// ... and the slab reduction + epilogue follows it.  *fused (may be NULL): the norm / RoPE the epilogue asks for went into the
// reduction; left alone when K was not split.
int srgpt_splitk_finish(const Epilogue& e, hipStream_t s, bool* fused) {
  if (e.splits <= 1) return SRGPT_OK;
  const bool f = launch_splitk_reduce<bf16_t>(e, s);
  if (fused) *fused = f;
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

extern "C" int64_t srgpt_gemm_ws_bytes(int M, int N) { return (int64_t)8 * M * N * 4; }

// a dense row-major product without bias, activation or residual; the entry points below assign what they add
static Epilogue plain_epilogue(void* C, int M, int N, int ldc) {
  Epilogue e{};
  e.C = C, e.M = M, e.N = N, e.ldc = ldc, e.act = SRGPT_ACT_NONE, e.out_mode = SRGPT_OUT_PLAIN, e.splits = 1;
  return e;
}

// The weight operand of a product: a row-major matrix of the activation dtype, or (ABI 9) row-major MXFP4 codes with their E8M0
// bytes (include/srgpt.h) and the bf16 scratch [N, K] they are expanded into where no kernel multiplies codes (gemm_w4_in_kernel).
struct WOperand {
  const void* w;       // the matrix, or the codes [N, K / 2]
  const void* scale8;  // NULL: `w` is a matrix of the dtype; else the block scales [N, K / 32]
  void* expand;        // codes only: written and read on the expansion path alone, may be NULL otherwise
  bool direct;         // codes only: the `_direct` entry points -- the whole-M kernel multiplies the codes too (gemm_w4_direct_in_kernel)
};

// the codes' checks, and their expansion where `in_kernel` is false: afterwards *W is what the bf16 launch reads
static int w4_resolve(const char* fn, const WOperand& w, int N, int K, int dtype, bool in_kernel, srgpt_stream_t stream, const void** W) {
  SRGPT_CHECK(dtype == SRGPT_BF16, SRGPT_ERR_ARG, "%s: MXFP4 weights need bf16 activations", fn);
  SRGPT_CHECK(K % 32 == 0, SRGPT_ERR_ARG, "%s: K=%d must be a multiple of 32 (one scale per 32 values)", fn, K);
  SRGPT_CHECK((uintptr_t)w.w % 4 == 0, SRGPT_ERR_ARG, "%s: the codes must be 4-byte aligned", fn);
  *W = w.w;
  if (in_kernel) return SRGPT_OK;
  SRGPT_CHECK(w.expand, SRGPT_ERR_ARG, "%s: this shape expands the codes first and needs the bf16 [N, K] scratch", fn);
  SRGPT_CHECK((uintptr_t)w.expand % 16 == 0, SRGPT_ERR_ARG, "%s: the scratch must be 16-byte aligned", fn);
  *W = w.expand;
  return srgpt_dequant_mxfp4(w.w, w.scale8, w.expand, N, K, stream);
}

// C = epilogue(A W^T) for the entry points below: validate, pick the route (gemm_route.h), launch its kernel, reduce the slabs.
// Codes take the route of the bf16 product and are multiplied in its kernel where gemm_w4_in_kernel (a `direct` operand:
// gemm_w4_direct_in_kernel) says so; everywhere else they are expanded and the launches are the bf16 ones.  *fused: see srgpt_splitk_finish.
static int gemm_run(const void* A, const WOperand& w, int K, int lda, int dtype, void* ws, int64_t ws_bytes, Epilogue e,
                    srgpt_stream_t stream, bool* fused) {
  const int M = e.M, N = e.N;
  const bool w4 = w.scale8 != nullptr;
  SRGPT_CHECK(A && w.w && e.C, SRGPT_ERR_ARG, "srgpt_gemm: null pointer");
  SRGPT_CHECK(M > 0 && N > 0 && K > 0, SRGPT_ERR_ARG, "srgpt_gemm: bad shape M=%d N=%d K=%d", M, N, K);
  SRGPT_CHECK(dtype == SRGPT_F32 || dtype == SRGPT_BF16, SRGPT_ERR_ARG, "srgpt_gemm: bad dtype %d", dtype);
  const int vec = dtype == SRGPT_BF16 ? 8 : 4;
  SRGPT_CHECK(K % vec == 0 && lda % vec == 0, SRGPT_ERR_ARG,
              "srgpt_gemm: K=%d and lda=%d must be multiples of %d (16-byte rows)", K, lda, vec);
  SRGPT_CHECK(((uintptr_t)A % 16 == 0) && (w4 || (uintptr_t)w.w % 16 == 0), SRGPT_ERR_ARG, "srgpt_gemm: A/W must be 16-byte aligned");
  if (e.out_mode == SRGPT_OUT_DECONV2X) {
    SRGPT_CHECK(N % 4 == 0 && e.gw > 0 && M % (e.gw * e.gw) == 0, SRGPT_ERR_ARG, "srgpt_gemm: bad deconv geometry");
  } else {
    SRGPT_CHECK(e.out_mode == SRGPT_OUT_PLAIN, SRGPT_ERR_ARG, "srgpt_gemm: unknown out_mode %d", e.out_mode);
    SRGPT_CHECK(e.ldc >= N, SRGPT_ERR_ARG, "srgpt_gemm: ldc < N");
  }
  hipStream_t s = as_stream(stream);
  const GemmRoute r = dtype == SRGPT_F32 ? gemm_route_f32() : gemm_route(M, N, K, srgpt_device_cus(), ws != nullptr, ws_bytes);
  const bool codes = w4 && (w.direct ? gemm_w4_direct_in_kernel(r, K) : gemm_w4_in_kernel(r, K));  // the kernel reads the codes
  const void* W = w.w;
  if (w4) SRGPT_TRY(w4_resolve("srgpt_gemm_w4", w, N, K, dtype, codes, stream, &W));
  srgpt_splitk_apply(e, r, ws);
  switch (r.family) {
    case GEMM_F32_SIMPLE:
      hipLaunchKernelGGL(gemm_f32_simple, dim3(cdiv(N, 64), cdiv(M, 64)), dim3(256), 0, s, (const float*)A, (const float*)W, K, lda, e);
      SRGPT_LAUNCH_CHECK();
      break;
    case GEMM_WHOLE_M_288:
      if (codes) SRGPT_TRY(srgpt_gemm288_w4_launch(A, W, w.scale8, K, lda, e, s));
      else SRGPT_TRY(srgpt_gemm288_launch(A, W, K, lda, e, s));
      break;
    case GEMM_TILE_256: SRGPT_TRY(srgpt_gemm256_launch(A, W, K, lda, e, s)); break;
    case GEMM_GLDS: {
      const dim3 grid(cdiv(N, 128), cdiv(M, r.bm), e.splits);
#define SRGPT_GLDS(BM, NBUF)                                                                                                        \
  do {                                                                                                                              \
    if (codes)                                                                                                                      \
      hipLaunchKernelGGL((gemm_bf16_glds<BM, 128, NBUF, const unsigned char*>), grid, dim3(256), 0, s, (const bf16_t*)A,            \
                         (const bf16_t*)W, K, lda, e, (const unsigned char*)w.scale8);                                              \
    else hipLaunchKernelGGL((gemm_bf16_glds<BM, 128, NBUF>), grid, dim3(256), 0, s, (const bf16_t*)A, (const bf16_t*)W, K, lda, e); \
  } while (0)
      if (r.bm == 128) SRGPT_GLDS(128, 1);
      else if (r.bm == 96 && r.nbuf == 2) SRGPT_GLDS(96, 2);
      else if (r.bm == 96) SRGPT_GLDS(96, 1);
      else if (r.nbuf == 2) SRGPT_GLDS(64, 2);
      else SRGPT_GLDS(64, 1);
#undef SRGPT_GLDS
      SRGPT_LAUNCH_CHECK();
      break;
    }
  }
  return srgpt_splitk_finish(e, s, fused);
}

extern "C" int srgpt_gemm(const void* A, const void* W, const void* bias, const void* residual, void* C, int M,
                          int N, int K, int lda, int ldc, int act, int bias_mod, int res_mod, int out_f32,
                          int out_mode, int gw, void* ws, int64_t ws_bytes, int dtype, srgpt_stream_t stream) {
  Epilogue e = plain_epilogue(C, M, N, ldc);
  e.bias = bias, e.residual = residual, e.act = act, e.bias_mod = bias_mod, e.res_mod = res_mod;
  e.out_f32 = out_f32, e.out_mode = out_mode, e.gw = gw;
  return gemm_run(A, WOperand{W, nullptr, nullptr}, K, lda, dtype, ws, ws_bytes, e, stream, nullptr);
}

// the W4 entry points' own pointer check (the scales make an operand a code operand, so a NULL one must not pass as a bf16 matrix)
static int w4_args(const char* fn, const void* W4, const void* wscale8) {
  SRGPT_CHECK(W4 && wscale8, SRGPT_ERR_ARG, "%s: null pointer", fn);
  return SRGPT_OK;
}

// Each W4 entry point and its `_direct` form (include/srgpt.h) are one call with WOperand::direct off / on.
extern "C" int srgpt_gemm_w4(const void* A, const void* W4, const void* wscale8, const void* residual, void* C, int M, int N, int K,
                             int lda, int ldc, int out_f32, void* expand, void* ws, int64_t ws_bytes, srgpt_stream_t stream) {
  SRGPT_TRY(w4_args("srgpt_gemm_w4", W4, wscale8));
  Epilogue e = plain_epilogue(C, M, N, ldc);
  e.residual = residual, e.out_f32 = out_f32;
  return gemm_run(A, WOperand{W4, wscale8, expand, false}, K, lda, SRGPT_BF16, ws, ws_bytes, e, stream, nullptr);
}

extern "C" int srgpt_gemm_w4_direct(const void* A, const void* W4, const void* wscale8, const void* residual, void* C, int M, int N,
                                    int K, int lda, int ldc, int out_f32, void* expand, void* ws, int64_t ws_bytes,
                                    srgpt_stream_t stream) {
  SRGPT_TRY(w4_args("srgpt_gemm_w4_direct", W4, wscale8));
  Epilogue e = plain_epilogue(C, M, N, ldc);
  e.residual = residual, e.out_f32 = out_f32;
  return gemm_run(A, WOperand{W4, wscale8, expand, true}, K, lda, SRGPT_BF16, ws, ws_bytes, e, stream, nullptr);
}

// C = A W^T + bias + residual (dense rows) and Y = norm(C) in one call (include/srgpt.h; the layer loops of model.hip).  The norm
// rides in the split-K reduction when the product is split; otherwise it is the ordinary srgpt_rmsnorm / srgpt_layernorm launch --
// either way the two outputs are bit-identical to srgpt_gemm followed by the norm.
static int gemm_norm_run(const void* A, const WOperand& w, const void* bias, const void* residual, void* C, int M, int N, int K, void* ws,
                         int64_t ws_bytes, int norm_kind, const void* norm_w, const void* norm_b, void* Y, float norm_eps, int dtype,
                         srgpt_stream_t stream) {
  SRGPT_CHECK(norm_kind == SRGPT_NORM_RMS || norm_kind == SRGPT_NORM_LAYER, SRGPT_ERR_ARG, "srgpt_gemm_norm: unknown norm kind %d",
              norm_kind);
  SRGPT_CHECK(norm_w && Y && (norm_kind == SRGPT_NORM_RMS || norm_b), SRGPT_ERR_ARG, "srgpt_gemm_norm: null pointer");
  SRGPT_CHECK(Y != C, SRGPT_ERR_ARG, "srgpt_gemm_norm: Y must not alias C");  // Y may be A: the norm runs after the product
  Epilogue e = plain_epilogue(C, M, N, N);
  e.bias = bias, e.residual = residual;
  e.norm_w = norm_w, e.norm_b = norm_b, e.norm_y = Y, e.norm_eps = norm_eps, e.norm_kind = norm_kind;
  bool fused = false;
  SRGPT_TRY(gemm_run(A, w, K, K, dtype, ws, ws_bytes, e, stream, &fused));
  if (!fused) {
    if (norm_kind == SRGPT_NORM_RMS) SRGPT_TRY(srgpt_rmsnorm(C, norm_w, Y, M, N, norm_eps, dtype, stream));
    else SRGPT_TRY(srgpt_layernorm(C, norm_w, norm_b, Y, M, N, norm_eps, SRGPT_ACT_NONE, dtype, stream));
  }
  return SRGPT_OK;
}

extern "C" int srgpt_gemm_norm(const void* A, const void* W, const void* bias, const void* residual, void* C, int M, int N, int K,
                               void* ws, int64_t ws_bytes, int norm_kind, const void* norm_w, const void* norm_b, void* Y,
                               float norm_eps, int dtype, srgpt_stream_t stream) {
  return gemm_norm_run(A, WOperand{W, nullptr, nullptr}, bias, residual, C, M, N, K, ws, ws_bytes, norm_kind, norm_w, norm_b, Y, norm_eps,
                       dtype, stream);
}

extern "C" int srgpt_gemm_w4_norm(const void* A, const void* W4, const void* wscale8, const void* residual, void* C, int M, int N, int K,
                                  void* expand, void* ws, int64_t ws_bytes, const void* norm_w, void* Y, float norm_eps,
                                  srgpt_stream_t stream) {
  SRGPT_TRY(w4_args("srgpt_gemm_w4_norm", W4, wscale8));
  return gemm_norm_run(A, WOperand{W4, wscale8, expand, false}, nullptr, residual, C, M, N, K, ws, ws_bytes, SRGPT_NORM_RMS, norm_w,
                       nullptr, Y, norm_eps, SRGPT_BF16, stream);
}

extern "C" int srgpt_gemm_w4_norm_direct(const void* A, const void* W4, const void* wscale8, const void* residual, void* C, int M, int N,
                                         int K, void* expand, void* ws, int64_t ws_bytes, const void* norm_w, void* Y, float norm_eps,
                                         srgpt_stream_t stream) {
  SRGPT_TRY(w4_args("srgpt_gemm_w4_norm_direct", W4, wscale8));
  return gemm_norm_run(A, WOperand{W4, wscale8, expand, true}, nullptr, residual, C, M, N, K, ws, ws_bytes, SRGPT_NORM_RMS, norm_w,
                       nullptr, Y, norm_eps, SRGPT_BF16, stream);
}

// qkv = A W^T for the B * T token rows of a prefill, then RoPE on q (in place) and k, k and v appended to the caches -- the
// projection and srgpt_rope_kv_append in one call (include/srgpt.h).  The rotation rides in the split-K reduction when the product is
// split; otherwise it is the ordinary srgpt_rope_kv_append launch.  Every byte written is the same either way.
static int gemm_rope_run(const void* A, const WOperand& w, void* qkv, int K, void* ws, int64_t ws_bytes, void* kcache, void* vcache,
                         const int* pos0, const void* cos_tab, const void* sin_tab, int B, int T_, int Hq, int Hkv, int D, int max_pos,
                         int dtype, srgpt_stream_t stream) {
  SRGPT_CHECK(qkv && kcache && vcache && cos_tab && sin_tab, SRGPT_ERR_ARG, "srgpt_gemm_rope_kv_append: null pointer");
  SRGPT_CHECK(B > 0 && T_ > 0 && Hq > 0 && Hkv > 0 && D > 0 && (D & 1) == 0 && T_ <= max_pos, SRGPT_ERR_ARG,
              "srgpt_gemm_rope_kv_append: bad shape");
  const int M = B * T_, N = (Hq + 2 * Hkv) * D;
  Epilogue e = plain_epilogue(qkv, M, N, N);
  e.rope_k = kcache, e.rope_v = vcache, e.rope_pos0 = pos0, e.rope_cos = cos_tab, e.rope_sin = sin_tab;
  e.rope_T = T_, e.rope_Hq = Hq, e.rope_Hkv = Hkv, e.rope_D = D, e.rope_max_pos = max_pos;
  bool fused = false;
  SRGPT_TRY(gemm_run(A, w, K, K, dtype, ws, ws_bytes, e, stream, &fused));
  if (!fused) SRGPT_TRY(srgpt_rope_kv_append(qkv, kcache, vcache, pos0, cos_tab, sin_tab, B, T_, Hq, Hkv, D, max_pos, dtype, stream));
  return SRGPT_OK;
}

extern "C" int srgpt_gemm_rope_kv_append(const void* A, const void* W, void* qkv, int K, void* ws, int64_t ws_bytes, void* kcache,
                                         void* vcache, const int* pos0, const void* cos_tab, const void* sin_tab, int B, int T_,
                                         int Hq, int Hkv, int D, int max_pos, int dtype, srgpt_stream_t stream) {
  return gemm_rope_run(A, WOperand{W, nullptr, nullptr}, qkv, K, ws, ws_bytes, kcache, vcache, pos0, cos_tab, sin_tab, B, T_, Hq, Hkv, D,
                       max_pos, dtype, stream);
}

extern "C" int srgpt_gemm_w4_rope_kv_append(const void* A, const void* W4, const void* wscale8, void* qkv, int K, void* expand, void* ws,
                                            int64_t ws_bytes, void* kcache, void* vcache, const int* pos0, const void* cos_tab,
                                            const void* sin_tab, int B, int T_, int Hq, int Hkv, int D, int max_pos,
                                            srgpt_stream_t stream) {
  SRGPT_TRY(w4_args("srgpt_gemm_w4_rope_kv_append", W4, wscale8));
  return gemm_rope_run(A, WOperand{W4, wscale8, expand, false}, qkv, K, ws, ws_bytes, kcache, vcache, pos0, cos_tab, sin_tab, B, T_, Hq,
                       Hkv, D, max_pos, SRGPT_BF16, stream);
}

extern "C" int srgpt_gemm_w4_rope_kv_append_direct(const void* A, const void* W4, const void* wscale8, void* qkv, int K, void* expand,
                                                   void* ws, int64_t ws_bytes, void* kcache, void* vcache, const int* pos0,
                                                   const void* cos_tab, const void* sin_tab, int B, int T_, int Hq, int Hkv, int D,
                                                   int max_pos, srgpt_stream_t stream) {
  SRGPT_TRY(w4_args("srgpt_gemm_w4_rope_kv_append_direct", W4, wscale8));
  return gemm_rope_run(A, WOperand{W4, wscale8, expand, true}, qkv, K, ws, ws_bytes, kcache, vcache, pos0, cos_tab, sin_tab, B, T_, Hq,
                       Hkv, D, max_pos, SRGPT_BF16, stream);
}

// out[M, I] = rnd(rnd(silu(A Wg^T)) * (A Wu^T)) for the stacked weight Wgu = [Wg; Wu] ([2 I, K]) -- LlamaMLP's gate / up products and
// srgpt_silu_mul in one call (include/srgpt.h).  On the whole-M kernel (225 .. 272 rows: the bs = 1 prefill) a block multiplies 64
// gate columns and the 64 matching up columns and the activation is its epilogue: the [M, 2 I] intermediate is neither written nor
// read.  Every other shape runs the plain product into `gu_scratch` and srgpt_silu_mul -- the result is the same to the last bit.
// Codes: the fused form expands them first, unless the operand is `direct` and the scale table fits (the whole-M kernel's W4
// instance, gemm288.hip); the plain product follows gemm_run's rule.
static int gemm_swiglu_run(const void* A, const WOperand& w, void* out, int M, int I, int K, void* gu_scratch, void* ws, int64_t ws_bytes,
                           int dtype, srgpt_stream_t stream) {
  const bool w4 = w.scale8 != nullptr;
  SRGPT_CHECK(A && w.w && out, SRGPT_ERR_ARG, "srgpt_gemm_swiglu: null pointer");
  SRGPT_CHECK(M > 0 && I > 0 && K > 0, SRGPT_ERR_ARG, "srgpt_gemm_swiglu: bad shape M=%d I=%d K=%d", M, I, K);
  if (dtype == SRGPT_BF16 && gemm_swiglu_fused_shape(M, I, K, srgpt_device_cus()) && ((uintptr_t)A % 16 == 0) &&
      (w4 || (uintptr_t)w.w % 16 == 0)) {
    const void* W = w.w;
    const bool codes = w4 && w.direct && gemm288_w4_scales_fit(K / 64);  // gemm_swiglu_w4_direct_in_kernel on the fused shape
    if (w4) SRGPT_TRY(w4_resolve("srgpt_gemm_w4_swiglu", w, 2 * I, K, dtype, codes, stream, &W));
    Epilogue e = plain_epilogue(out, M, I, I);
    e.swiglu_inter = I;
    if (codes) SRGPT_TRY(srgpt_gemm288_w4_launch(A, W, w.scale8, K, K, e, as_stream(stream)));
    else SRGPT_TRY(srgpt_gemm288_launch(A, W, K, K, e, as_stream(stream)));
    return SRGPT_OK;
  }
  SRGPT_CHECK(gu_scratch, SRGPT_ERR_ARG, "srgpt_gemm_swiglu: this shape needs the [M, 2 I] scratch buffer");
  SRGPT_TRY(gemm_run(A, w, K, K, dtype, ws, ws_bytes, plain_epilogue(gu_scratch, M, 2 * I, 2 * I), stream, nullptr));
  return srgpt_silu_mul(gu_scratch, out, M, I, dtype, stream);
}

extern "C" int srgpt_gemm_swiglu(const void* A, const void* Wgu, void* out, int M, int I, int K, void* gu_scratch, void* ws,
                                 int64_t ws_bytes, int dtype, srgpt_stream_t stream) {
  return gemm_swiglu_run(A, WOperand{Wgu, nullptr, nullptr}, out, M, I, K, gu_scratch, ws, ws_bytes, dtype, stream);
}

extern "C" int srgpt_gemm_w4_swiglu(const void* A, const void* Wgu4, const void* wscale8, void* out, int M, int I, int K,
                                    void* gu_scratch, void* expand, void* ws, int64_t ws_bytes, srgpt_stream_t stream) {
  SRGPT_TRY(w4_args("srgpt_gemm_w4_swiglu", Wgu4, wscale8));
  return gemm_swiglu_run(A, WOperand{Wgu4, wscale8, expand, false}, out, M, I, K, gu_scratch, ws, ws_bytes, SRGPT_BF16, stream);
}

extern "C" int srgpt_gemm_w4_swiglu_direct(const void* A, const void* Wgu4, const void* wscale8, void* out, int M, int I, int K,
                                           void* gu_scratch, void* expand, void* ws, int64_t ws_bytes, srgpt_stream_t stream) {
  SRGPT_TRY(w4_args("srgpt_gemm_w4_swiglu_direct", Wgu4, wscale8));
  return gemm_swiglu_run(A, WOperand{Wgu4, wscale8, expand, true}, out, M, I, K, gu_scratch, ws, ws_bytes, SRGPT_BF16, stream);
}

// host only: 1 when the W4 entry point of this shape multiplies the codes in its kernel on this device, 0 when it expands them first
// (N = I with swiglu: srgpt_gemm_w4_swiglu)
extern "C" int srgpt_gemm_w4_in_kernel(int M, int N, int K, int swiglu, int have_ws, int64_t ws_bytes) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 32 != 0) return 0;
  const int cus = srgpt_device_cus();
  if (swiglu) return gemm_swiglu_w4_in_kernel(M, N, K, cus, have_ws != 0, ws_bytes) ? 1 : 0;
  return gemm_w4_in_kernel(gemm_route(M, N, K, cus, have_ws != 0, ws_bytes), K) ? 1 : 0;
}

// the same question for the `_direct` entry points
extern "C" int srgpt_gemm_w4_direct_in_kernel(int M, int N, int K, int swiglu, int have_ws, int64_t ws_bytes) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 32 != 0) return 0;
  const int cus = srgpt_device_cus();
  if (swiglu) return gemm_swiglu_w4_direct_in_kernel(M, N, K, cus, have_ws != 0, ws_bytes) ? 1 : 0;
  return gemm_w4_direct_in_kernel(gemm_route(M, N, K, cus, have_ws != 0, ws_bytes), K) ? 1 : 0;
}

// C = epilogue((A @ fp8(W8)^T) * wscale): bf16 activations, OCP e4m3fn weight bytes, one fp32 scale per weight row -- the
// prefill-side companion of srgpt_gemv_w8 (BASELINE config 5).  Always the 256 x 256 kernel (W tile staged as bytes, widened
// to bf16 between LDS and the MFMA operands); K splits (deterministic slabs) when the tiles do not fill the chip.
extern "C" int srgpt_gemm_w8(const void* A, const void* W8, const float* wscale, const void* bias, const void* residual,
                             void* C, int M, int N, int K, int lda, int ldc, int act, int out_f32, void* ws,
                             int64_t ws_bytes, srgpt_stream_t stream) {
  SRGPT_CHECK(A && W8 && wscale && C, SRGPT_ERR_ARG, "srgpt_gemm_w8: null pointer");
  SRGPT_CHECK(M > 0 && N > 0 && K > 0, SRGPT_ERR_ARG, "srgpt_gemm_w8: bad shape M=%d N=%d K=%d", M, N, K);
  SRGPT_CHECK(lda >= K, SRGPT_ERR_ARG, "srgpt_gemm_w8: lda < K");
  SRGPT_CHECK(ldc >= N, SRGPT_ERR_ARG, "srgpt_gemm_w8: ldc < N");
  Epilogue e = plain_epilogue(C, M, N, ldc);
  e.bias = bias, e.residual = residual, e.act = act, e.out_f32 = out_f32, e.wscale = wscale;
  hipStream_t s = as_stream(stream);
  if (K % 64 != 0 || lda % 8 != 0 || ((uintptr_t)A % 16) || ((uintptr_t)W8 % 16)) {  // odd geometries: the scalar kernel
    hipLaunchKernelGGL(gemm_w8_simple, dim3(cdiv(N, 64), cdiv(M, 64)), dim3(256), 0, s, (const bf16_t*)A,
                       (const unsigned char*)W8, K, lda, e);
    SRGPT_LAUNCH_CHECK();
    return SRGPT_OK;
  }
  srgpt_splitk_apply(e, gemm_route_fp8(M, N, K / 64, 8, srgpt_device_cus(), ws != nullptr, ws_bytes), ws);
  SRGPT_TRY(srgpt_gemm256_launch(A, W8, K, lda, e, s));
  return srgpt_splitk_finish(e, s, nullptr);
}
