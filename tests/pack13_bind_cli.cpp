// Exercises the binding table of spatialrgpt_amd/csrc/pack13_bind.h on the host (tests/test_host_pack13.py): bind, rebind, unbind,
// a lookup with another shape, and binds / lookups from several threads.  Prints "ok" and exits 0, or names the failed check.
#include <stdio.h>

#include <thread>
#include <vector>

#include "pack13_bind.h"

#define CHECK(c)                                  \
  do {                                            \
    if (!(c)) return printf("failed: %s\n", #c), 1; \
  } while (0)

int main() {
  Pack13Table t;
  char raw[4] = {}, packed_a[1] = {}, packed_b[1] = {}, meta_a[1] = {}, meta_b[1] = {};
  Pack13Binding b{};
  CHECK(!t.bound(raw) && !t.lookup(raw, 8, 512, &b) && !t.unbind(raw));
  t.bind(raw, Pack13Binding{packed_a, meta_a, 8, 512});
  CHECK(t.bound(raw) && t.size() == 1);
  CHECK(t.lookup(raw, 8, 512, &b) && b.packed == packed_a && b.meta == meta_a && b.rows == 8 && b.K == 512);
  CHECK(!t.lookup(raw, 4, 512, &b) && !t.lookup(raw, 8, 1024, &b) && !t.lookup(raw + 1, 8, 512, &b));  // shape / address mismatch
  t.bind(raw, Pack13Binding{packed_b, meta_b, 16, 1024});  // rebind replaces
  CHECK(t.size() == 1 && !t.lookup(raw, 8, 512, &b));
  CHECK(t.lookup(raw, 16, 1024, &b) && b.packed == packed_b && b.meta == meta_b);
  t.bind(raw + 1, Pack13Binding{packed_a, meta_a, 8, 512});
  CHECK(t.size() == 2 && t.unbind(raw) && !t.bound(raw) && t.bound(raw + 1) && !t.unbind(raw));
  CHECK(t.lookup(raw + 1, 8, 512, &b) && b.packed == packed_a);
  CHECK(t.unbind(raw + 1) && t.size() == 0);
  // several threads on their own keys and one shared key
  std::vector<char> keys(64);
  std::vector<std::thread> th;
  for (int i = 0; i < 8; ++i)
    th.emplace_back([&, i] {
      for (int rep = 0; rep < 200; ++rep)
        for (int j = 0; j < 8; ++j) {
          const char* k = &keys[8 * i + j];
          Pack13Binding got{};
          t.bind(k, Pack13Binding{k, k, i + 1, 512 * (j + 1)});
          t.bind(raw, Pack13Binding{k, k, 1, 512});
          if (!t.lookup(k, i + 1, 512 * (j + 1), &got) || got.packed != k) keys[8 * i + j] = 1;
          if (rep % 2) t.unbind(k);
        }
    });
  for (auto& x : th) x.join();
  for (char c : keys) CHECK(c == 0);
  CHECK(t.bound(raw) && t.size() == 1);  // the last repetition unbound every thread's own keys; the shared one stays
  return printf("ok\n"), 0;
}
