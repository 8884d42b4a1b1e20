// Exercises the binding table of spatialrgpt_amd/csrc/mxfp4_bind.h on the host (tests/test_host_mxfp4_bind.py): bind, rebind, unbind,
// a lookup with another shape at the same (recycled) address, and binds / lookups from several threads.  Prints "ok" and exits 0, or
// names the failed check.
#include <stdio.h>

#include <thread>
#include <vector>

#include "mxfp4_bind.h"

#define CHECK(c)                                  \
  do {                                            \
    if (!(c)) return printf("failed: %s\n", #c), 1; \
  } while (0)

int main() {
  Mxfp4Table t;
  char codes[4] = {}, packed_a[1] = {}, packed_b[1] = {};
  Mxfp4Binding b{};
  CHECK(!t.bound(codes) && !t.lookup(codes, 16, 128, 0, &b) && !t.unbind(codes));
  t.bind(codes, Mxfp4Binding{packed_a, 16, 128, 0});
  CHECK(t.bound(codes) && t.size() == 1);
  CHECK(t.lookup(codes, 16, 128, 0, &b) && b.packed == packed_a && b.N == 16 && b.K == 128 && b.swiglu == 0);
  // shape / fusion / address mismatch
  CHECK(!t.lookup(codes, 8, 128, 0, &b) && !t.lookup(codes, 16, 256, 0, &b) && !t.lookup(codes, 16, 128, 1, &b) &&
        !t.lookup(codes + 1, 16, 128, 0, &b));
  t.bind(codes, Mxfp4Binding{packed_b, 32, 256, 1});  // rebind replaces
  CHECK(t.size() == 1 && !t.lookup(codes, 16, 128, 0, &b));
  CHECK(t.lookup(codes, 32, 256, 1, &b) && b.packed == packed_b && t.lookup(codes, 32, 256, 7, &b));  // swiglu is a flag
  // a recycled address: the matrix was freed WITHOUT an unbind and another one of another shape now lives there -- never matched
  CHECK(!t.lookup(codes, 64, 256, 0, &b) && !t.lookup(codes, 16, 256, 1, &b));
  t.bind(codes + 1, Mxfp4Binding{packed_a, 16, 128, 0});
  CHECK(t.size() == 2 && t.unbind(codes) && !t.bound(codes) && t.bound(codes + 1) && !t.unbind(codes));
  CHECK(t.lookup(codes + 1, 16, 128, 0, &b) && b.packed == packed_a);
  CHECK(t.unbind(codes + 1) && t.size() == 0);
  // several threads on their own keys and one shared key
  std::vector<char> keys(64);
  std::vector<std::thread> th;
  for (int i = 0; i < 8; ++i)
    th.emplace_back([&, i] {
      for (int rep = 0; rep < 200; ++rep)
        for (int j = 0; j < 8; ++j) {
          const char* k = &keys[8 * i + j];
          Mxfp4Binding got{};
          t.bind(k, Mxfp4Binding{k, i + 1, 128 * (j + 1), j & 1});
          t.bind(codes, Mxfp4Binding{k, 1, 128, 0});
          if (!t.lookup(k, i + 1, 128 * (j + 1), j & 1, &got) || got.packed != k) keys[8 * i + j] = 1;
          if (rep % 2) t.unbind(k);
        }
    });
  for (auto& x : th) x.join();
  for (char c : keys) CHECK(c == 0);
  CHECK(t.bound(codes) && t.size() == 1);  // the last repetition unbound every thread's own keys; the shared one stays
  return printf("ok\n"), 0;
}
