// Prints the MXFP4 decode product's routes of spatialrgpt_amd/csrc/gemv_route.h (tests/test_mxfp4_abi.py):
//   gemv_w4_route_cli CUS < queries
// One query per line, "ROWS N K SWIGLU"; one answer per line: "gemv_w4 CHUNK UNIT_COLS" and then, for every weight pass of the call,
// " | ROWS B NX NIT GRID LDS RAISE_LDS_LIMIT".
#include <stdio.h>
#include <stdlib.h>

#include "gemv_route.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const int cus = atoi(argv[1]);
  int rows, N, K, swiglu;
  while (scanf("%d %d %d %d", &rows, &N, &K, &swiglu) == 4) {
    const GemvRoute r = gemv_w4_route(rows);
    if (r.family != GEMV_W4 || r.chunk < 1 || r.chunk > W4_MAX_ROWS) return 3;
    printf("gemv_w4 %d %d", r.chunk, W4_UNIT_COLS);
    for (int b0 = 0; b0 < rows; b0 += r.chunk) {
      const int nb = rows - b0 < r.chunk ? rows - b0 : r.chunk;
      const GemvValuLaunch l = gemv_w4_launch(nb, N, K, swiglu != 0, cus);
      printf(" | %d %d %d %d %d %lld %d", nb, l.B, l.NX, l.NIT, l.grid, l.lds, (int)l.raise_lds_limit);
    }
    printf("\n");
  }
  return 0;
}
