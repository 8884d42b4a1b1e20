// Prints the multi-token decode route of spatialrgpt_amd/csrc/attn_route.h (tests/test_host_attn_route_multi.py):
//   attn_route_multi_cli < queries
// One query per line, one answer per line:
//   "DTYPE B T HQ HKV D MAX_POS" -> "STATUS FAMILY G T COLS NC NSPLIT KPB BLOCKS WS_FLOATS CAP"       (DTYPE = bf16 or f32)
#include <stdio.h>
#include <string.h>

#include "attn_route.h"

int main() {
  char dtype[16];
  int B, T, Hq, Hkv, D, max_pos;
  while (scanf("%15s %d %d %d %d %d %d", dtype, &B, &T, &Hq, &Hkv, &D, &max_pos) == 7) {
    const bool bf16 = !strcmp(dtype, "bf16");
    if (!bf16 && strcmp(dtype, "f32")) return 2;
    const AttnDecodeMultiRoute r = attn_decode_multi_route(bf16, B, T, Hq, Hkv, D, max_pos);
    printf("%s %s %d %d %d %d %d %d %d %zu %d\n", r.status == ATTN_OK ? "ok" : r.status == ATTN_TOO_MANY_COLUMNS ? "columns" : "?",
           r.family == ATTN_DECODE_MULTI_MFMA ? "multi_mfma" : r.family == ATTN_DECODE_MULTI_COMPOSED ? "composed" : "?", r.G, r.T, r.cols,
           r.nc, r.nsplit, r.kpb, r.blocks, r.ws_floats, attn_decode_multi_cap(r.G));
  }
  return 0;
}
