// Prints the 13-bit packed decode product's routes of spatialrgpt_amd/csrc/gemv_route.h (tests/test_host_pack13.py):
//   gemv_p13_route_cli CUS < queries
// One query per line, "ROWS N K SWIGLU" (the launch does not depend on SWIGLU: a unit is then two rows); one answer per line: "raw" where the product is not eligible (more than one row, or K not a
// multiple of 512), else "gemv_p13 CHUNK | B NX LOADS GROUPS GRID LDS RAISE_LDS_LIMIT" (LOADS: per batch and row).
#include <stdio.h>
#include <stdlib.h>

#include "gemv_route.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const int cus = atoi(argv[1]);
  int rows, N, K, swiglu;
  while (scanf("%d %d %d %d", &rows, &N, &K, &swiglu) == 4) {
    if (!gemv_p13_eligible(rows, K)) {
      printf("raw\n");
      continue;
    }
    const GemvRoute r = gemv_p13_route();
    if (r.family != GEMV_P13 || r.chunk != 1) return 3;
    const GemvValuLaunch l = gemv_p13_launch(N, K, cus);
    printf("gemv_p13 %d | %d %d %d %d %d %lld %d\n", r.chunk, l.B, l.NX, l.UB, l.NIT, l.grid, l.lds, (int)l.raise_lds_limit);
  }
  return 0;
}
