// Prints the routes of spatialrgpt_amd/csrc/gemv_route.h (tests/test_host_gemv_route.py):  gemv_route_cli CUS < queries
// One query per line, "DTYPE ROWS N K NORM SWIGLU SS_IN PACKED" with DTYPE = bf16, f32 or fp8 (fp8 weights, bf16 activations); one
// answer per line: "FAMILY CHUNK ROWSS_SUPPORTED" (gemv_rowss_supported of the rows) and then, for every weight pass of the call,
// " | ROWS" and the launch --
//   VALU families:  B NX UB NIT GRID LDS RAISE_LDS_LIMIT          skinny:  NI NW PUB PK GRID CW GR_SHIFT LDS
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gemv_route.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const int cus = atoi(argv[1]);
  static const char* const family[] = {"gemv", "gemv_reg", "gemv_w8", "skinny"};
  char dtype[16];
  int rows, N, K, norm, swiglu, ss_in, packed;
  while (scanf("%15s %d %d %d %d %d %d %d", dtype, &rows, &N, &K, &norm, &swiglu, &ss_in, &packed) == 8) {
    const bool fp8 = !strcmp(dtype, "fp8"), bf16 = fp8 || !strcmp(dtype, "bf16");
    if (!bf16 && strcmp(dtype, "f32")) return 2;
    const GemvRoute r = gemv_route(rows, K, bf16, fp8, norm != 0);
    printf("%s %d %d", family[r.family], r.chunk, (int)gemv_rowss_supported(rows, bf16, fp8, cus));
    for (int b0 = 0; b0 < rows && r.chunk > 0; b0 += r.chunk) {
      const int nb = rows - b0 < r.chunk ? rows - b0 : r.chunk;
      if (r.family == GEMV_SKINNY) {
        const GemvSkinnyLaunch l = gemv_skinny_launch(nb, N, norm != 0, ss_in != 0, packed, cus);
        printf(" | %d %d %d %d %d %d %d %d %d", nb, l.NI, l.NW, (int)l.PUB, (int)l.PK, l.grid, l.cw, l.gr_shift, l.lds);
      } else {
        const GemvValuLaunch l = gemv_valu_launch(r.family, nb, N, K, bf16, swiglu != 0, cus);
        printf(" | %d %d %d %d %d %d %lld %d", nb, l.B, l.NX, l.UB, l.NIT, l.grid, l.lds, (int)l.raise_lds_limit);
      }
    }
    printf("\n");
  }
  return 0;
}
