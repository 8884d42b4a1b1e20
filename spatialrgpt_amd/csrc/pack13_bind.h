// Which raw bf16 matrices have a 13-bit packed copy (pack13.h) the batch-1 decode step may stream instead: a BindTable keyed by the
// raw matrix's address, filled by srgpt_pack13_bind and consulted by model.hip's decode-layer sequence.
// Plain C++ (no HIP): tests/test_host_pack13.py compiles this header into a stand-alone program.
#pragma once
#include "bind_table.h"

struct Pack13Binding {
  const void* packed;  // p13_packed_bytes(rows, K)
  const void* meta;    // p13_meta_bytes(rows)
  int rows, K;         // rows of the matrix (a SwiGLU matrix: gate rows + up rows)
  bool same_shape(int rows_, int K_) const { return rows == rows_ && K == K_; }
};

using Pack13Table = BindTable<Pack13Binding>;  // lookup(raw, rows, K, &binding)
