// Prints the routes of spatialrgpt_amd/csrc/gemm_route.h (tests/test_host_gemm_route.py):  gemm_route_cli CUS < queries
// One query per line, "ENTRY M N K HAVE_WS WS_BYTES" with ENTRY = gemm (bf16 srgpt_gemm and its composites), gemm_w8, gemm_w8a8
// or swiglu (N = the intermediate size); one answer per line, "FAMILY BM NBUF SPLITS TILES_PER_SPLIT NK" (swiglu: "fused" / "unfused").
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
    GemmRoute r;
    int nk = (K + 63) / 64;
    if (!strcmp(entry, "gemm")) {
      r = gemm_route(M, N, K, cus, have_ws != 0, ws_bytes);
    } else if (!strcmp(entry, "gemm_w8")) {
      r = gemm_route_fp8(M, N, nk = K / 64, 8, cus, have_ws != 0, ws_bytes);
    } else if (!strcmp(entry, "gemm_w8a8")) {
      r = gemm_route_fp8(M, N, nk = K / 128, 4, cus, have_ws != 0, ws_bytes);
    } else if (!strcmp(entry, "swiglu")) {
      puts(gemm_swiglu_fused_shape(M, N, K, cus) ? "fused" : "unfused");
      continue;
    } else {
      return 2;
    }
    printf("%s %d %d %d %d %d\n", family[r.family], r.bm, r.nbuf, r.splits, r.tiles_per_split, nk);
  }
  return 0;
}
