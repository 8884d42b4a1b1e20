// Prints the wide routes of spatialrgpt_amd/csrc/gemv_route.h (tests/test_host_gemv_wide_route.py):  gemv_wide_route_cli CUS < queries
// One query per line, "FORMAT ROWS N K NORM SWIGLU SS_IN PACKED PASS_ROWS" with FORMAT = bf16, fp8 (fp8 weights, bf16 activations) or
// w4 (packed MXFP4, PACKED = 16); one answer per line in the form of gemv_route_cli: "FAMILY CHUNK ROWSS_SUPPORTED" and then, for every
// weight pass of the call as srgpt_decode_product cuts it, " | ROWS" and the launch --
//   VALU families:  B NX UB NIT GRID LDS RAISE_LDS_LIMIT          skinny, w4_mfma:  NI NW PUB PK GRID CW GR_SHIFT LDS
// A pass of 17 - 32 rows is gemv_wide_launch's, a pass of 16 rows or fewer gemv_skinny_launch's for its row count.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gemv_route.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const int cus = atoi(argv[1]);
  static const char* const family[] = {"gemv", "gemv_reg", "gemv_w8", "skinny", "gemv_w4", "gemv_p13", "w4_mfma"};
  char fmt[16];
  int rows, N, K, norm, swiglu, ss_in, packed, pass_rows;
  while (scanf("%15s %d %d %d %d %d %d %d %d", fmt, &rows, &N, &K, &norm, &swiglu, &ss_in, &packed, &pass_rows) == 9) {
    const bool fp8 = !strcmp(fmt, "fp8"), w4 = !strcmp(fmt, "w4");
    if (!fp8 && !w4 && strcmp(fmt, "bf16")) return 2;
    const GemvRoute r = gemv_wide_route(rows, K, fp8, packed, w4, norm != 0, swiglu != 0, pass_rows);
    printf("%s %d %d", family[r.family], r.chunk, (int)gemv_rowss_supported(rows, true, fp8, cus));
    for (int b0 = 0; b0 < rows && r.chunk > 0; b0 += r.chunk) {
      const int nb = rows - b0 < r.chunk ? rows - b0 : r.chunk;
      if (r.family == GEMV_SKINNY || r.family == GEMV_W4_MFMA) {
        const GemvSkinnyLaunch l = nb > 16 ? gemv_wide_launch(nb, N, norm != 0, ss_in != 0, packed, cus)
                                           : gemv_skinny_launch(nb, N, norm != 0, ss_in != 0, packed, cus);
        printf(" | %d %d %d %d %d %d %d %d %d", nb, l.NI, l.NW, (int)l.PUB, (int)l.PK, l.grid, l.cw, l.gr_shift, l.lds);
      } else {
        const GemvValuLaunch l = gemv_valu_launch(r.family, nb, N, K, true, swiglu != 0, cus);
        printf(" | %d %d %d %d %d %d %lld %d", nb, l.B, l.NX, l.UB, l.NIT, l.grid, l.lds, (int)l.raise_lds_limit);
      }
    }
    printf("\n");
  }
  return 0;
}
