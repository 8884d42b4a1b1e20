// Prints the routes of spatialrgpt_amd/csrc/attn_route.h (tests/test_host_attn_route.py):  attn_route_cli CUS < queries
// One query per line, one answer per line:
//   "prefill DTYPE D TQ TK HQ B Q_BS Q_TS Q_HS K_BS K_TS K_HS V_BS V_TS V_HS QKV_ALIGNED16 O_ALIGNED8 SCALE_POSITIVE"
//        -> "FAMILY HDP GRID_X GRID_Y GRID_Z BLOCK"                                            (DTYPE = bf16 or f32)
//   "decode DTYPE B HQ HKV D MAX_POS"
//        -> "STATUS FAMILY G NSPLIT KPB N_ATTN PARTIAL_FLOATS TICKETS_RESERVED TICKETS_USED WS_FLOATS LAST_GROUP LAST_ROW LAST_TICKET"
//           (the offsets of the last (sequence, kv head) group, of its last (head, split) row inside it, and its ticket's index)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "attn_route.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const int cus = atoi(argv[1]);
  static const char* const family[] = {"flash", "one_wave", "decode_mfma", "decode_valu"};
  static const char* const status[] = {"ok", "max_pos", "head_dim", "group"};
  char what[16], dtype[16];
  while (scanf("%15s %15s", what, dtype) == 2) {
    const bool bf16 = !strcmp(dtype, "bf16");
    if (!bf16 && strcmp(dtype, "f32")) return 2;
    if (!strcmp(what, "prefill")) {
      int D, Tq, Tk, Hq, B, a16, o8, sp;
      long long s[9];
      if (scanf("%d %d %d %d %d %lld %lld %lld %lld %lld %lld %lld %lld %lld %d %d %d", &D, &Tq, &Tk, &Hq, &B, &s[0], &s[1], &s[2], &s[3],
                &s[4], &s[5], &s[6], &s[7], &s[8], &a16, &o8, &sp) != 17)
        return 2;
      const AttnPrefillRoute r =
          attn_prefill_route(bf16, D, Tq, Tk, Hq, B, s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], a16 != 0, o8 != 0, sp != 0);
      printf("%s %d %d %d %d %d\n", family[r.family], r.hdp, r.grid_x, r.grid_y, r.grid_z, r.block);
    } else if (!strcmp(what, "decode")) {
      int B, Hq, Hkv, D, max_pos;
      if (scanf("%d %d %d %d %d", &B, &Hq, &Hkv, &D, &max_pos) != 5) return 2;
      const AttnDecodeRoute r = attn_decode_route(bf16, B, Hq, Hkv, D, max_pos, cus);
      static int tickets[1];  // only its address is used
      printf("%s %s %d %d %d %d %zu %zu %zu %zu %zu %zu %zu\n", status[r.status], family[r.family], r.G, r.nsplit, r.kpb, r.n_attn,
             attn_ws_partial_floats(B, Hq, D), attn_ws_tickets_reserved(B, Hq), attn_ws_tickets_used(B, Hkv), attn_ws_floats(B, Hq, D),
             attn_ws_group(B - 1, Hkv - 1, Hkv, r.G, D), attn_ws_row(r.G - 1, r.nsplit - 1, D),
             (size_t)((char*)attn_ws_ticket(tickets, B - 1, Hkv - 1, Hkv) - (char*)tickets) / sizeof(int));
    } else {
      return 2;
    }
  }
  return 0;
}
