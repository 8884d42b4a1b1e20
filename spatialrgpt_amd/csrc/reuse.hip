// Prefix reuse across requests: how much of the LAST request is the head of this one, judged on the device.
//
// The reference's callers re-send the whole conversation every turn -- the same image and depth tensors, a mask tensor that grew at
// its end, ids that begin with last turn's prompt and answer.  Whether the retained tower features and the live KV cache of the
// last request still serve is a comparison of BYTES and of row descriptors; nothing here hashes, so nothing can collide: a miss
// costs a full request, a false hit would be a wrong answer.
//   srgpt_rows_match    leading rows of two byte matrices that are equal byte for byte (images and depths: one row; the masks of an
//                       image: one row per region -> the leading regions whose embeddings are still valid)
//   srgpt_splice_match  leading rows of this prompt's splice table (srgpt_splice_plan) that name the sources the cached rows came
//                       from: the last prompt's table, then the ids it generated
// Integer and byte work only; both results are a minimum over "first row that differs", so they do not depend on scheduling.
#include "common.h"

namespace {

constexpr int RM_NT = 256;
constexpr int SM_NT = 1024;

// first differing byte of two loaded units, counted from the unit's lowest address (little endian); U = sizeof(V)
template <typename V>
__device__ __forceinline__ int first_diff_byte(const V& x, const V& y);
template <>
__device__ __forceinline__ int first_diff_byte<unsigned char>(const unsigned char& x, const unsigned char& y) { return x != y ? 0 : -1; }
template <>
__device__ __forceinline__ int first_diff_byte<unsigned short>(const unsigned short& x, const unsigned short& y) {
  const unsigned int d = (unsigned int)(x ^ y);
  return d ? (__ffs(d) - 1) >> 3 : -1;
}
template <>
__device__ __forceinline__ int first_diff_byte<unsigned int>(const unsigned int& x, const unsigned int& y) {
  const unsigned int d = x ^ y;
  return d ? (__ffs(d) - 1) >> 3 : -1;
}
template <>
__device__ __forceinline__ int first_diff_byte<u32x2>(const u32x2& x, const u32x2& y) {
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const unsigned int d = x[k] ^ y[k];
    if (d) return 4 * k + ((__ffs(d) - 1) >> 3);
  }
  return -1;
}
template <>
__device__ __forceinline__ int first_diff_byte<u32x4>(const u32x4& x, const u32x4& y) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned int d = x[k] ^ y[k];
    if (d) return 4 * k + ((__ffs(d) - 1) >> 3);
  }
  return -1;
}

__global__ void rows_match_init_kernel(int rows, int* __restrict__ out) { out[0] = rows; }

// The two matrices as flat byte strings of n bytes: `head` single bytes up to the first address where a and b are BOTH aligned to
// sizeof(V) (the host picks the widest V for which such an address exists), `nvec` units of V, single bytes to the end.  Work items
// are numbered in address order and a thread walks its items in increasing order, so the first difference a thread meets is its
// lowest; the minimum over threads of that byte's row goes to out[0] (set to `rows` by the launch in front).
template <typename V>
__global__ __launch_bounds__(RM_NT) void rows_match_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                           long long n, long long head, long long nvec, long long row_bytes,
                                                           int* __restrict__ out) {
  constexpr int U = (int)sizeof(V);
  const long long tail0 = head + nvec * U;        // first byte behind the vector body
  const long long items = head + nvec + (n - tail0);
  const long long stride = (long long)gridDim.x * RM_NT;
  long long diff = -1;
  for (long long i = (long long)blockIdx.x * RM_NT + threadIdx.x; i < items; i += stride) {
    if (i < head) {
      if (a[i] != b[i]) diff = i;
    } else if (i < head + nvec) {
      const long long off = head + (i - head) * U;
      const V x = *reinterpret_cast<const V*>(a + off), y = *reinterpret_cast<const V*>(b + off);
      const int k = first_diff_byte<V>(x, y);
      if (k >= 0) diff = off + k;
    } else {
      const long long off = tail0 + (i - head - nvec);
      if (a[off] != b[off]) diff = off;
    }
    if (diff >= 0) break;
  }
  if (diff >= 0) atomicMin(out, (int)(diff / row_bytes));
}

constexpr int SPL_MASK = 2, SPL_DEPTH = 3;  // row kinds of srgpt_splice_plan (splice.hip)

__global__ __launch_bounds__(SM_NT) void splice_match_kernel(const int* __restrict__ desc_new, int len_new, const int* __restrict__ desc_old,
                                                             int n_old_rows, const int64_t* __restrict__ gen_old, int n_gen_old,
                                                             int n_regions_common, int* __restrict__ out) {
  __shared__ int red[SM_NT / 64];
  const long long len_old = (long long)n_old_rows + n_gen_old;
  const int len = (int)(len_old < len_new ? len_old : len_new);
  int first = len;
  for (int r = threadIdx.x; r < len; r += SM_NT) {
    const int key = desc_new[2 * r];
    // a generated id is a text row: kind 0, src = the id (64-bit: an id beyond the descriptor's 30 bits equals no key)
    const long long old = r < n_old_rows ? (long long)desc_old[2 * r] : (long long)gen_old[r - n_old_rows] * 4;
    const int kind = key & 3, src = key >> 2;
    const bool stale = (kind == SPL_MASK || kind == SPL_DEPTH) && src >= n_regions_common;
    if ((long long)key != old || stale) {
      first = r;
      break;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = first;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < SM_NT / 64; ++w) first = min(first, red[w]);
    out[0] = first;
  }
}

template <typename V>
void launch_rows_match(const unsigned char* a, const unsigned char* b, long long n, long long row_bytes, int* out, hipStream_t s) {
  constexpr long long U = (long long)sizeof(V);
  const long long mis = (long long)(reinterpret_cast<uintptr_t>(a) % U);  // == that of b: the host chose V so
  long long head = mis ? U - mis : 0;
  head = head < n ? head : n;
  const long long nvec = (n - head) / U;
  const long long items = head + nvec + (n - head - nvec * U);
  long long grid = (items + RM_NT * 4 - 1) / (RM_NT * 4);  // ~4 items per thread, at most 1024 blocks
  grid = grid < 1 ? 1 : (grid > 1024 ? 1024 : grid);
  hipLaunchKernelGGL(rows_match_kernel<V>, dim3((unsigned)grid), dim3(RM_NT), 0, s, a, b, n, head, nvec, row_bytes, out);
}

}  // namespace

extern "C" int srgpt_rows_match(const void* a, const void* b, int rows, int64_t row_bytes, int* out, srgpt_stream_t stream) {
  SRGPT_CHECK(a && b && out, SRGPT_ERR_ARG, "srgpt_rows_match: null pointer");
  SRGPT_CHECK(rows >= 0 && row_bytes >= 1, SRGPT_ERR_ARG, "srgpt_rows_match: bad shape (rows = %d, row_bytes = %lld)", rows,
              (long long)row_bytes);
  SRGPT_CHECK(row_bytes <= 0x7fffffffffffffffLL / (rows > 0 ? rows : 1), SRGPT_ERR_ARG, "srgpt_rows_match: rows * row_bytes overflows");
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(rows_match_init_kernel, dim3(1), dim3(1), 0, s, rows, out);
  SRGPT_LAUNCH_CHECK();
  if (rows == 0) return SRGPT_OK;
  const unsigned char *pa = static_cast<const unsigned char*>(a), *pb = static_cast<const unsigned char*>(b);
  const long long n = (long long)rows * row_bytes;
  // the widest unit at which a and b reach an aligned address TOGETHER: equal misalignment modulo the unit
  const uintptr_t d = reinterpret_cast<uintptr_t>(pa) ^ reinterpret_cast<uintptr_t>(pb);
  if ((d & 15) == 0) launch_rows_match<u32x4>(pa, pb, n, row_bytes, out, s);
  else if ((d & 7) == 0) launch_rows_match<u32x2>(pa, pb, n, row_bytes, out, s);
  else if ((d & 3) == 0) launch_rows_match<unsigned int>(pa, pb, n, row_bytes, out, s);
  else if ((d & 1) == 0) launch_rows_match<unsigned short>(pa, pb, n, row_bytes, out, s);
  else launch_rows_match<unsigned char>(pa, pb, n, row_bytes, out, s);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

extern "C" int srgpt_splice_match(const int* desc_new, int len_new, const int* desc_old, int n_old_rows, const int64_t* gen_old,
                                  int n_gen_old, int n_regions_common, int* out, srgpt_stream_t stream) {
  SRGPT_CHECK(desc_new && desc_old && gen_old && out, SRGPT_ERR_ARG, "srgpt_splice_match: null pointer");
  SRGPT_CHECK(len_new >= 0 && n_old_rows >= 0 && n_gen_old >= 0 && n_regions_common >= 0, SRGPT_ERR_ARG,
              "srgpt_splice_match: negative length (len_new = %d, n_old_rows = %d, n_gen_old = %d, n_regions_common = %d)", len_new,
              n_old_rows, n_gen_old, n_regions_common);
  hipLaunchKernelGGL(splice_match_kernel, dim3(1), dim3(SM_NT), 0, as_stream(stream), desc_new, len_new, desc_old, n_old_rows, gen_old,
                     n_gen_old, n_regions_common, out);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}
