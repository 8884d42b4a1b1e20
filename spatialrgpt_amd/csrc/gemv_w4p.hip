// The packed MXFP4 decode layout (include/srgpt.h, "Additions under ABI 9"): pack / unpack, the MFMA product over it
// (srgpt_gemv_w4p -> skinny_kernel's W4 mode, skinny.hip) and the binding table that hands such copies to the decode steps.
//
// A cell is one granule (G = W4_GRANULE_ROWS weight rows) x W4_CELL_K = 128 k: 64 G code bytes [g = k / 8 % 4][row][16 bytes] --
// dword s of a lane's 16 bytes = its 8 codes of MFMA k step s -- followed by 4 G scale bytes [row][k step].  A wave reads the codes of
// a cell with ONE instruction (G = 16: 1 KiB contiguous) and the scales with one more (64 bytes right behind them).
#include <stdlib.h>

#include "common.h"
#include "gemv_route.h"
#include "internal.h"
#include "mxfp4_bind.h"

static_assert(W4_GRANULE_ROWS == SRGPT_MXFP4_GRANULE, "gemv_route.h rounds cw to the granule of include/srgpt.h");

namespace {

constexpr int G = W4_GRANULE_ROWS;
constexpr int CELLB = 68 * G;  // bytes of a cell

// one thread per (cell, g, row in granule): the 16 code bytes of lane (row, g); the g == 0 thread also moves the row's 4 scale bytes.
// PACK: row-major -> packed (rows past the matrix: code 0, scale byte 127); else packed -> row-major (rows past it: nothing)
template <bool PACK>
__global__ __launch_bounds__(256) void mxfp4_repack_kernel(unsigned char* __restrict__ W4, unsigned char* __restrict__ wscale8,
                                                           unsigned char* __restrict__ packed, int rows, int K, long long nslot) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nslot) return;
  const int r = (int)(i % G), g = (int)(i / G % 4);
  const long long cell = i / (4 * G);
  const int ncell = K / W4_CELL_K, kb = (int)(cell % ncell);
  const long long n = cell / ncell * G + r;
  unsigned char* pc = packed + (size_t)cell * CELLB + (size_t)(g * G + r) * 16;
  unsigned char* ps = packed + (size_t)cell * CELLB + 64 * G + (size_t)r * 4;
  unsigned char* src = W4 + ((size_t)n * K + (size_t)kb * W4_CELL_K + 8 * g) / 2;  // the 4 code bytes of k step s: + 16 s
  unsigned char* ssrc = wscale8 + (size_t)n * (K / 32) + (size_t)kb * 4;
  if (PACK) {
    u32x4 v = {0u, 0u, 0u, 0u};
    unsigned int sc = 0x7f7f7f7fu;
    if (n < rows) {
#pragma unroll
      for (int s = 0; s < 4; ++s) v[s] = *reinterpret_cast<const unsigned int*>(src + 16 * s);
      sc = *reinterpret_cast<const unsigned int*>(ssrc);
    }
    *reinterpret_cast<u32x4*>(pc) = v;
    if (g == 0) *reinterpret_cast<unsigned int*>(ps) = sc;
  } else if (n < rows) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(pc);
#pragma unroll
    for (int s = 0; s < 4; ++s) *reinterpret_cast<unsigned int*>(src + 16 * s) = v[s];
    if (g == 0) *reinterpret_cast<unsigned int*>(ssrc) = *reinterpret_cast<const unsigned int*>(ps);
  }
}

Mxfp4Table& table() {
  static Mxfp4Table t;
  return t;
}

// the layout's domain, on the host before any launch
int check_shape(const char* fn, int N, int K, int swiglu) {
  SRGPT_CHECK(N > 0 && K > 0, SRGPT_ERR_ARG, "%s: bad shape", fn);
  SRGPT_CHECK(K % W4_CELL_K == 0, SRGPT_ERR_ARG, "%s: K=%d must be a multiple of %d (whole cells)", fn, K, W4_CELL_K);
  SRGPT_CHECK(!swiglu || N % G == 0, SRGPT_ERR_ARG, "%s: a SwiGLU matrix needs whole granules per half (N=%d, %d rows per granule)", fn, N, G);
  SRGPT_CHECK((long long)N * (swiglu ? 2 : 1) <= 0x7fffffffLL / 2, SRGPT_ERR_ARG, "%s: N=%d too large", fn, N);
  return SRGPT_OK;
}

template <bool PACK>
int repack(const char* fn, void* W4, void* wscale8, void* packed, int N, int K, int swiglu, srgpt_stream_t stream) {
  SRGPT_CHECK(W4 && wscale8 && packed, SRGPT_ERR_ARG, "%s: null pointer", fn);
  SRGPT_TRY(check_shape(fn, N, K, swiglu));
  const int rows = swiglu ? 2 * N : N;
  const long long nslot = gemv_w4p_packed_bytes(rows, K) / CELLB * (4 * G);
  hipLaunchKernelGGL(mxfp4_repack_kernel<PACK>, dim3((unsigned)((nslot + 255) / 256)), dim3(256), 0, as_stream(stream), (unsigned char*)W4,
                     (unsigned char*)wscale8, (unsigned char*)packed, rows, K, nslot);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

}  // namespace

bool srgpt_mxfp4_lookup(const void* W4, int N, int K, int swiglu, Mxfp4Binding* out) { return table().lookup(W4, N, K, swiglu, out); }

extern "C" size_t srgpt_mxfp4_packed_bytes(int N, int K, int swiglu) {
  if (N <= 0 || K <= 0 || K % W4_CELL_K != 0 || (swiglu && N % G != 0) || (long long)N * (swiglu ? 2 : 1) > 0x7fffffffLL / 2) return 0;
  return (size_t)gemv_w4p_packed_bytes((long long)N * (swiglu ? 2 : 1), K);
}

extern "C" int srgpt_pack_mxfp4(const void* W4, const void* wscale8, void* packed, int N, int K, int swiglu, srgpt_stream_t stream) {
  return repack<true>("srgpt_pack_mxfp4", const_cast<void*>(W4), const_cast<void*>(wscale8), packed, N, K, swiglu, stream);
}

extern "C" int srgpt_unpack_mxfp4(const void* packed, void* W4, void* wscale8, int N, int K, int swiglu, srgpt_stream_t stream) {
  return repack<false>("srgpt_unpack_mxfp4", W4, wscale8, const_cast<void*>(packed), N, K, swiglu, stream);
}

// srgpt_gemv_rowss's contract over a packed MXFP4 array: srgpt_decode_product's passes of up to 16 rows (gemv_w4_step_route's MFMA
// leg), every pass with its rows of x, residual, out and both statistics tables
static int gemv_w4p_impl(const void* x, const void* packed, const void* norm_w, float norm_eps, const void* residual, void* out,
                         int batch, int N, int K, int swiglu, int out_f32, const float* rowss_in, float* rowss_out, int pass_rows,
                         srgpt_stream_t stream) {
  SRGPT_CHECK(x && packed && out, SRGPT_ERR_ARG, "srgpt_gemv_w4p: null pointer");
  SRGPT_CHECK(batch > 0, SRGPT_ERR_ARG, "srgpt_gemv_w4p: bad shape");
  SRGPT_TRY(check_shape("srgpt_gemv_w4p", N, K, swiglu));
  SRGPT_CHECK(!(swiglu && (residual || out_f32)), SRGPT_ERR_ARG, "srgpt_gemv_w4p: swiglu excludes residual/out_f32");
  SRGPT_CHECK(!rowss_in || norm_w, SRGPT_ERR_ARG, "srgpt_gemv_w4p: published row statistics are the RMSNorm's input (norm_w is NULL)");
  SRGPT_CHECK(!rowss_out || (!swiglu && !out_f32), SRGPT_ERR_ARG, "srgpt_gemv_w4p: row statistics are published for plain bf16 outputs only");
  SRGPT_CHECK((!rowss_in && !rowss_out) || 2 * srgpt_device_cus() <= GEMV_ROWSS_SLOTS, SRGPT_ERR_UNSUPPORTED,
              "srgpt_gemv_w4p: %d CUs do not fit the %d row-statistics slots", srgpt_device_cus(), GEMV_ROWSS_SLOTS);
  // the MFMA leg's route, whatever the call holds
  return srgpt_decode_product(DecodeProduct{x, packed, nullptr, norm_w, norm_eps, residual, out, batch, N, K, swiglu, out_f32, SRGPT_BF16,
                                            0, rowss_in, rowss_out, W4_GRANULE_ROWS, 1},
                              gemv_wide_route(batch, K, false, W4_GRANULE_ROWS, true, norm_w != nullptr, swiglu != 0, pass_rows),
                              as_stream(stream));
}

extern "C" int srgpt_gemv_w4p(const void* x, const void* packed, const void* norm_w, float norm_eps, const void* residual, void* out,
                              int batch, int N, int K, int swiglu, int out_f32, const float* rowss_in, float* rowss_out,
                              srgpt_stream_t stream) {
  return gemv_w4p_impl(x, packed, norm_w, norm_eps, residual, out, batch, N, K, swiglu, out_f32, rowss_in, rowss_out, 16, stream);
}

// The same product with chunks of 17 - 32 rows in ONE weight pass (gemv_wide_route); 16 rows or fewer: srgpt_gemv_w4p itself
extern "C" int srgpt_gemv_w4p_wide(const void* x, const void* packed, const void* norm_w, float norm_eps, const void* residual, void* out,
                                   int batch, int N, int K, int swiglu, int out_f32, const float* rowss_in, float* rowss_out,
                                   srgpt_stream_t stream) {
  return gemv_w4p_impl(x, packed, norm_w, norm_eps, residual, out, batch, N, K, swiglu, out_f32, rowss_in, rowss_out, GEMV_WIDE_ROWS,
                       stream);
}

extern "C" int srgpt_mxfp4_bind(const void* W4, const void* packed, int N, int K, int swiglu) {
  SRGPT_CHECK(W4 && packed, SRGPT_ERR_ARG, "srgpt_mxfp4_bind: null pointer");
  SRGPT_TRY(check_shape("srgpt_mxfp4_bind", N, K, swiglu));
  table().bind(W4, Mxfp4Binding{packed, N, K, swiglu != 0 ? 1 : 0});
  return SRGPT_OK;
}

extern "C" int srgpt_mxfp4_unbind(const void* W4) { return table().unbind(W4) ? 1 : 0; }

extern "C" int srgpt_mxfp4_bound(const void* W4) { return table().bound(W4) ? 1 : 0; }
