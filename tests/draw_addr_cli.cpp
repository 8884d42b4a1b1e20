// Answers queries about spatialrgpt_amd/csrc/draw_addr.h (tests/test_host_draw_addr.py):  draw_addr_cli < queries
// One query per line, one answer per line:
//   addr COUNTER B T steps[0] .. steps[B - 1]    ->  "m" and then, for every row r = b * T + t in order, " | CTR SEQ" (draw_addr)
//   adv B before[0 .. B) after[0 .. B)           ->  what the accept adds to the counter (draw_advance over draw_column of both)
// COUNTER and CTR are unsigned 64-bit decimals.  The header is compiled alone, no HIP; the static_asserts below are the rule at compile
// time, as device code sees it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "draw_addr.h"

constexpr int kSteps[3] = {5, 2, -1};
static_assert(draw_column(kSteps, 3) == 0 && draw_column(kSteps, 2) == 2, "m: the minimum, a negative count clamped to 0");
static_assert(draw_addr(100, kSteps, 2, 4, 3).ctr == 106 && draw_addr(100, kSteps, 2, 4, 3).seq == 0, "row (0, 3): 100 + (5 - 2) + 3");
static_assert(draw_addr(100, kSteps, 2, 4, 4).ctr == 100 && draw_addr(100, kSteps, 2, 4, 4).seq == 1, "row (1, 0): the column the counter names");
static_assert(draw_addr(0xFFFFFFFFull, kSteps, 2, 4, 0).ctr == 0x100000002ull, "the sum carries into the high word");
static_assert(draw_advance(3, 3) == 0 && draw_advance(3, 7) == 4, "the columns that filled up");

int main() {
  char cmd[8];
  int steps[64], after[64];
  while (scanf("%7s", cmd) == 1) {
    if (!strcmp(cmd, "addr")) {
      char num[32];
      int B, T;
      if (scanf("%31s %d %d", num, &B, &T) != 3 || B < 1 || B > 64 || T < 1) return 2;
      for (int b = 0; b < B; ++b)
        if (scanf("%d", &steps[b]) != 1) return 2;
      const uint64_t counter = strtoull(num, nullptr, 10);
      printf("%d", draw_column(steps, B));
      for (int r = 0; r < B * T; ++r) {
        const DrawAddr a = draw_addr(counter, steps, B, T, r);
        printf(" | %llu %d", (unsigned long long)a.ctr, a.seq);
      }
      printf("\n");
    } else if (!strcmp(cmd, "adv")) {
      int B;
      if (scanf("%d", &B) != 1 || B < 1 || B > 64) return 2;
      for (int b = 0; b < B; ++b)
        if (scanf("%d", &steps[b]) != 1) return 2;
      for (int b = 0; b < B; ++b)
        if (scanf("%d", &after[b]) != 1) return 2;
      printf("%llu\n", (unsigned long long)draw_advance(draw_column(steps, B), draw_column(after, B)));
    } else {
      return 2;
    }
  }
  return 0;
}
