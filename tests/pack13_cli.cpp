// Round-trips bf16 rows through the 13-bit code of spatialrgpt_amd/csrc/pack13.h on the host (tests/test_host_pack13.py):
//   pack13_cli            -> prints "rows R coded C zero Z special S below B" and exits 0, or names the first mismatch and exits 1
// Every one of the 65 536 bf16 bit patterns is placed in rows of 512 whose other half has one filler exponent, for a list of filler
// exponents that puts it inside the window, below it, above it (then it moves the window), and into the zero / denormal and the
// Inf / NaN classes; whether the row must be an exception row is worked out here, independently of the header.  Then rows of 512,
// 1024, 2560 (a padded last group) and 4096 pseudo-random weights of an LLM-like spread.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pack13.h"

static long g_rows, g_coded, g_zero, g_special, g_below;

// the row must come back bit for bit; `expect_exception` < 0: not checked
static int roundtrip(const std::vector<uint16_t>& row, int expect_exception, const char* what) {
  const int K = (int)row.size();
  std::vector<uint32_t> packed(p13_row_bytes(K) / 4 + 1, 0xdeadbeefu);  // one guard word behind the row
  const uint32_t meta = p13_pack_row(row.data(), K, reinterpret_cast<unsigned char*>(packed.data()));
  if (packed.back() != 0xdeadbeefu) return printf("%s: wrote past the packed row\n", what), 1;
  if (expect_exception >= 0 && (meta == P13_EXCEPTION) != (expect_exception != 0))
    return printf("%s: exception = %d, expected %d\n", what, meta == P13_EXCEPTION, expect_exception), 1;
  if (meta != P13_EXCEPTION && (p13_meta_base(meta) & 1 || p13_meta_base(meta) < 2 || p13_meta_base(meta) > 224))
    return printf("%s: base %d\n", what, p13_meta_base(meta)), 1;
  if (meta == P13_EXCEPTION)
    for (size_t i = 0; i + 1 < packed.size(); ++i)
      if (packed[i] != 0) return printf("%s: an exception row's packed bytes are not zero\n", what), 1;
  std::vector<uint16_t> back(K, 0xffff);
  p13_unpack_row(reinterpret_cast<const unsigned char*>(packed.data()), meta, row.data(), K, back.data());
  if (memcmp(back.data(), row.data(), (size_t)K * 2) != 0) {
    for (int k = 0; k < K; ++k)
      if (back[k] != row[k]) return printf("%s: k = %d: 0x%04x came back as 0x%04x (meta 0x%08x)\n", what, k, row[k], back[k], meta), 1;
  }
  ++g_rows;
  g_coded += meta != P13_EXCEPTION;
  return 0;
}

int main() {
  static const int fillers[] = {1, 2, 3, 30, 31, 32, 33, 34, 100, 126, 127, 158, 159, 200, 222, 223, 224, 253, 254};
  char what[96];
  for (int F : fillers)
    for (int e = 0; e < 256; ++e) {
      std::vector<uint16_t> row(512);
      for (int p = 0; p < 256; ++p) {  // all 2 x 128 patterns of exponent e, interleaved with the filler
        row[2 * p] = (uint16_t)(((p >> 7) << 15) | (e << 7) | (p & 127));
        row[2 * p + 1] = (uint16_t)((F << 7) | 0x55 | ((p & 1) << 15));
      }
      // independent expectation: window of 32 exponents ending at the row's largest, its base rounded up to even and at least 2
      const int emax = e > F ? e : F, emin = e < F ? e : F;
      int b = emax - 31 < 1 ? 1 : emax - 31;
      if (b % 2) ++b;
      const bool zero = e == 0, special = e == 255, below = !zero && !special && emin < b;
      g_zero += zero, g_special += special, g_below += below;
      snprintf(what, sizeof what, "filler exponent %d, exponent %d", F, e);
      if (roundtrip(row, zero || special || below, what)) return 1;
    }
  // LLM-like rows: exponents spread over ~ 20 values below 2^-3, random signs and mantissas
  uint64_t s = 0x9e3779b97f4a7c15ull;
  auto rnd = [&]() { return s = s * 6364136223846793005ull + 1442695040888963407ull, (uint32_t)(s >> 33); };
  for (int K : {512, 1024, 2560, 4096})
    for (int rep = 0; rep < 8; ++rep) {
      std::vector<uint16_t> row(K);
      for (int k = 0; k < K; ++k) {
        const uint32_t r = rnd();
        int drop = 0;
        for (uint32_t bits = rnd(); (bits & 1) && drop < 20; bits >>= 1) ++drop;  // geometric: most values near the top
        row[k] = (uint16_t)(((r & 1) << 15) | ((124 - drop) << 7) | ((r >> 1) & 127));
      }
      snprintf(what, sizeof what, "random row K = %d #%d", K, rep);
      if (roundtrip(row, 0, what)) return 1;
      row[(size_t)rnd() % K] = 0;  // one exact zero: an exception row, still lossless
      if (roundtrip(row, 1, what)) return 1;
    }
  printf("rows %ld coded %ld zero %ld special %ld below %ld\n", g_rows, g_coded, g_zero, g_special, g_below);
  return 0;
}
