// Prints the routes of an MXFP4 engine's decode-shaped steps of spatialrgpt_amd/csrc/gemv_route.h (tests/test_host_gemv_w4_step_route.py):
//   gemv_w4_step_route_cli CUS < queries
// One query per line, "ROWS N K SWIGLU NORM SS_IN BOUND"; one answer per line: "FAMILY CHUNK" and then, for every weight pass of the
// call, " | ROWS B NX NIT GRID LDS RAISE_LDS_LIMIT" (gemv_w4: the VALU kernel) or " | ROWS NI NW PUB PK GRID CW GR_SHIFT LDS"
// (gemv_w4_mfma: the MFMA kernel over the packed copy).
#include <stdio.h>
#include <stdlib.h>

#include "gemv_route.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const int cus = atoi(argv[1]);
  int rows, N, K, swiglu, norm, ss_in, bound;
  while (scanf("%d %d %d %d %d %d %d", &rows, &N, &K, &swiglu, &norm, &ss_in, &bound) == 7) {
    const GemvRoute r = gemv_w4_step_route(rows, bound != 0);
    if ((r.family != GEMV_W4 && r.family != GEMV_W4_MFMA) || r.chunk < 1) return 3;
    printf("%s %d", r.family == GEMV_W4 ? "gemv_w4" : "gemv_w4_mfma", r.chunk);
    for (int b0 = 0; b0 < rows; b0 += r.chunk) {
      const int nb = rows - b0 < r.chunk ? rows - b0 : r.chunk;
      if (r.family == GEMV_W4) {
        const GemvValuLaunch l = gemv_w4_launch(nb, N, K, swiglu != 0, cus);
        printf(" | %d %d %d %d %d %lld %d", nb, l.B, l.NX, l.NIT, l.grid, l.lds, (int)l.raise_lds_limit);
      } else {
        const GemvSkinnyLaunch l = gemv_skinny_launch(nb, N, norm != 0, ss_in != 0, W4_GRANULE_ROWS, cus);
        printf(" | %d %d %d %d %d %d %d %d %d", nb, l.NI, l.NW, (int)l.PUB, (int)l.PK, l.grid, l.cw, l.gr_shift, l.lds);
      }
    }
    printf("\n");
  }
  return 0;
}
