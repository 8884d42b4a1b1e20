// Prints what spatialrgpt_amd/csrc/gemm_route.h decides for the `_direct` W4 products (tests/test_host_gemm_w4_direct_route.py):
//   gemm_w4_direct_route_cli CUS < queries
// One query per line, "ENTRY M N K HAVE_WS WS_BYTES" with ENTRY = gemm_w4 (srgpt_gemm_w4_direct and its norm / RoPE composites) or
// swiglu_w4 (srgpt_gemm_w4_swiglu_direct, N = the intermediate size).  One answer per line:
//   "FAMILY BM NBUF SPLITS TILES_PER_SPLIT NK IN_KERNEL DIRECT_IN_KERNEL FITS"
// FAMILY .. IN_KERNEL: the answer of tests/gemm_w4_route_cli.cpp for the plain entry (the route is gemm_route's, unchanged);
// DIRECT_IN_KERNEL: gemm_w4_direct_in_kernel / gemm_swiglu_w4_direct_in_kernel; FITS: gemm288_w4_scales_fit of the K tiles a block of
// that route covers (the fit rule the whole-M kernel's launcher shares).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gemm_route.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const int cus = atoi(argv[1]);
  static const char* const family[] = {"f32_simple", "whole_m_288", "tile_256", "glds"};
  char entry[32];
  int M, N, K, have_ws;
  long long ws_bytes;
  while (scanf("%31s %d %d %d %d %lld", entry, &M, &N, &K, &have_ws, &ws_bytes) == 6) {
    const int nk = (K + 63) / 64;
    const bool swiglu = !strcmp(entry, "swiglu_w4");
    if (!swiglu && strcmp(entry, "gemm_w4")) return 2;
    if (swiglu && gemm_swiglu_fused_shape(M, N, K, cus)) {
      printf("fused 0 0 1 0 %d %d %d %d\n", nk, (int)gemm_swiglu_w4_in_kernel(M, N, K, cus, have_ws != 0, ws_bytes),
             (int)gemm_swiglu_w4_direct_in_kernel(M, N, K, cus, have_ws != 0, ws_bytes), (int)gemm288_w4_scales_fit(nk));
      continue;
    }
    const int rows = swiglu ? 2 * N : N;
    const GemmRoute r = gemm_route(M, rows, K, cus, have_ws != 0, ws_bytes);
    const int in_kernel = swiglu ? gemm_swiglu_w4_in_kernel(M, N, K, cus, have_ws != 0, ws_bytes) : gemm_w4_in_kernel(r, K);
    const int direct = swiglu ? gemm_swiglu_w4_direct_in_kernel(M, N, K, cus, have_ws != 0, ws_bytes) : gemm_w4_direct_in_kernel(r, K);
    printf("%s %d %d %d %d %d %d %d %d\n", family[r.family], r.bm, r.nbuf, r.splits, r.tiles_per_split, nk, in_kernel, direct,
           (int)gemm288_w4_scales_fit(r.tiles_per_split));
  }
  return 0;
}
