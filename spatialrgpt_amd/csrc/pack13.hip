// The 13-bit lossless code of a bf16 matrix (pack13.h) on the device: the pack kernel (load time), its exact inverse (tests and
// debugging), and the binding table (pack13_bind.h) through which the packed copies reach the batch-1 decode step.
#include "common.h"
#include "internal.h"
#include "pack13.h"
#include "pack13_bind.h"

namespace {

// one block per row (grid-strided): scan the row's exponents, publish the meta word, then every thread encodes (group, lane) pieces
__global__ __launch_bounds__(256) void pack13_kernel(const uint16_t* __restrict__ W, int N, int K, unsigned char* __restrict__ packed,
                                                     uint32_t* __restrict__ meta) {
  __shared__ int s_max[4], s_min[4], s_bad[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int groups = p13_groups(K);
  const size_t row_bytes = p13_row_bytes(K);
  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    const uint16_t* row = W + (size_t)n * K;
    int emax = 0, emin = 255, bad = 0;
    for (int c = tid; c < K / 8; c += 256) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(row + (size_t)c * 8);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int e = (v[q] >> (16 * half + 7)) & 0xff;
          emax = max(emax, e);
          emin = min(emin, e);
          bad |= (e == 0 || e == 255) ? 1 : 0;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
      emax = max(emax, __shfl_xor(emax, off));
      emin = min(emin, __shfl_xor(emin, off));
      bad |= __shfl_xor(bad, off);
    }
    __syncthreads();  // the row before has been encoded by every thread
    if (lane == 0) {
      s_max[wave] = emax;
      s_min[wave] = emin;
      s_bad[wave] = bad;
    }
    __syncthreads();
    emax = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    emin = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
    bad = s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3];
    const uint32_t m = p13_meta(emax, emin, bad != 0);
    if (tid == 0) {
      meta[n] = m;
      if (m == P13_EXCEPTION) atomicAdd(&meta[N], 1u);  // the count the entry reads back
    }
    unsigned char* prow = packed + (size_t)n * row_bytes;
    for (int idx = tid; idx < groups * 64; idx += 256) {
      const int g = idx >> 6, l = idx & 63;
      const P13Lane o = m == P13_EXCEPTION ? P13Lane{} : p13_encode_lane(row, K, m, g, l);
      *reinterpret_cast<uint32_t*>(prow + p13_sign_off(g, l)) = o.sign;
      *reinterpret_cast<u32x4*>(prow + p13_nib_off(g, l)) = u32x4{o.nib[0], o.nib[1], o.nib[2], o.nib[3]};
      *reinterpret_cast<u32x4*>(prow + p13_low_off(g, 0, l)) = u32x4{o.low[0], o.low[1], o.low[2], o.low[3]};
      *reinterpret_cast<u32x4*>(prow + p13_low_off(g, 1, l)) = u32x4{o.low[4], o.low[5], o.low[6], o.low[7]};
    }
  }
}

// the inverse: a coded row from its planes (the product's own decode, p13_high4 / p13_f32_bits), an exception row from the raw matrix
__global__ __launch_bounds__(256) void unpack13_kernel(const unsigned char* __restrict__ packed, const uint32_t* __restrict__ meta,
                                                       const uint16_t* __restrict__ W, int N, int K, uint16_t* __restrict__ out) {
  const int tid = threadIdx.x;
  const int groups = p13_groups(K);
  const size_t row_bytes = p13_row_bytes(K);
  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    const uint32_t m = meta[n];
    uint16_t* orow = out + (size_t)n * K;
    if (m == P13_EXCEPTION) {
      for (int c = tid; c < K / 8; c += 256)
        *reinterpret_cast<u32x4*>(orow + (size_t)c * 8) = *reinterpret_cast<const u32x4*>(W + (size_t)n * K + (size_t)c * 8);
      continue;
    }
    const unsigned char* prow = packed + (size_t)n * row_bytes;
    for (int idx = tid; idx < groups * 64; idx += 256) {
      const int g = idx >> 6, l = idx & 63;
      const uint32_t sign = *reinterpret_cast<const uint32_t*>(prow + p13_sign_off(g, l));
      const u32x4 nib = *reinterpret_cast<const u32x4*>(prow + p13_nib_off(g, l));
      const u32x4 low[2] = {*reinterpret_cast<const u32x4*>(prow + p13_low_off(g, 0, l)),
                            *reinterpret_cast<const u32x4*>(prow + p13_low_off(g, 1, l))};
#pragma unroll
      for (int t = 0; t < P13_GROUP_ITS; ++t) {
        const long long k0 = ((long long)(P13_GROUP_ITS * g + t) * 64 + l) * 8;
        if (k0 >= K) continue;  // padding of the row's last group (K % 8 == 0: whole chunks)
        u32x4 o;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint32_t high = p13_high4(sign, nib[t], m, t, h), lo = low[t >> 1][2 * (t & 1) + h];
          o[2 * h] = (p13_f32_bits(high, lo, 0) >> 16) | (p13_f32_bits(high, lo, 1) & 0xffff0000u);
          o[2 * h + 1] = (p13_f32_bits(high, lo, 2) >> 16) | (p13_f32_bits(high, lo, 3) & 0xffff0000u);
        }
        *reinterpret_cast<u32x4*>(orow + k0) = o;
      }
    }
  }
}

Pack13Table& table() {
  static Pack13Table t;
  return t;
}

int check_shape(const char* fn, int N, int K) {
  SRGPT_CHECK(N > 0 && K > 0, SRGPT_ERR_ARG, "%s: bad shape", fn);
  SRGPT_CHECK(p13_eligible(N, K), SRGPT_ERR_ARG, "%s: K=%d must be a multiple of 512 (whole 64-lane chunk iterations)", fn, K);
  return SRGPT_OK;
}

}  // namespace

bool srgpt_pack13_lookup(const void* W_raw, int rows, int K, Pack13Binding* out) { return table().lookup(W_raw, rows, K, out); }

extern "C" size_t srgpt_pack13_bytes(int N, int K, size_t* meta_bytes) {
  if (!p13_eligible(N, K)) {
    if (meta_bytes) *meta_bytes = 0;
    return 0;
  }
  if (meta_bytes) *meta_bytes = p13_meta_bytes(N);
  return p13_packed_bytes(N, K);
}

extern "C" int srgpt_pack13(const void* W, int N, int K, void* packed, void* flags, srgpt_stream_t stream) {
  SRGPT_CHECK(W && packed && flags, SRGPT_ERR_ARG, "srgpt_pack13: null pointer");
  SRGPT_TRY(check_shape("srgpt_pack13", N, K));
  hipStream_t s = as_stream(stream);
  uint32_t* meta = reinterpret_cast<uint32_t*>(flags);
  SRGPT_HIP_TRY(hipMemsetAsync(meta + N, 0, sizeof(uint32_t), s), "srgpt_pack13: hipMemsetAsync");
  const int cap = srgpt_device_cus() * 8;
  hipLaunchKernelGGL(pack13_kernel, dim3(N < cap ? N : cap), dim3(256), 0, s, (const uint16_t*)W, N, K, (unsigned char*)packed, meta);
  SRGPT_LAUNCH_CHECK();
  uint32_t count = 0;
  SRGPT_HIP_TRY(hipMemcpyAsync(&count, meta + N, sizeof(uint32_t), hipMemcpyDeviceToHost, s), "srgpt_pack13: hipMemcpyAsync");
  SRGPT_HIP_TRY(hipStreamSynchronize(s), "srgpt_pack13: hipStreamSynchronize");
  return (int)count;
}

extern "C" int srgpt_unpack13(const void* packed, const void* flags, const void* W_raw, int N, int K, void* out, srgpt_stream_t stream) {
  SRGPT_CHECK(packed && flags && W_raw && out, SRGPT_ERR_ARG, "srgpt_unpack13: null pointer");
  SRGPT_TRY(check_shape("srgpt_unpack13", N, K));
  const int cap = srgpt_device_cus() * 8;
  hipLaunchKernelGGL(unpack13_kernel, dim3(N < cap ? N : cap), dim3(256), 0, as_stream(stream), (const unsigned char*)packed,
                     (const uint32_t*)flags, (const uint16_t*)W_raw, N, K, (uint16_t*)out);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

extern "C" int srgpt_pack13_bind(const void* W_raw, const void* packed, const void* flags, int N, int K) {
  SRGPT_CHECK(W_raw && packed && flags, SRGPT_ERR_ARG, "srgpt_pack13_bind: null pointer");
  SRGPT_TRY(check_shape("srgpt_pack13_bind", N, K));
  table().bind(W_raw, Pack13Binding{packed, flags, N, K});
  return SRGPT_OK;
}

extern "C" int srgpt_pack13_unbind(const void* W_raw) { return table().unbind(W_raw) ? 1 : 0; }

extern "C" int srgpt_pack13_bound(const void* W_raw) { return table().bound(W_raw) ? 1 : 0; }
