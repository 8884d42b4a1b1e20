// Which MXFP4 code arrays have a packed copy in MFMA-operand order (srgpt_pack_mxfp4, include/srgpt.h) that a decode-shaped step of
// 2+ rows may multiply instead: a BindTable keyed by the code array's address, filled by srgpt_mxfp4_bind and consulted by model.hip's
// DecodeStep.
// Plain C++ (no HIP): tests/test_host_mxfp4_bind.py compiles this header into a stand-alone program.
#pragma once
#include "bind_table.h"

struct Mxfp4Binding {
  const void* packed;  // srgpt_mxfp4_packed_bytes(N, K, swiglu)
  int N, K, swiglu;    // swiglu: the matrix is N gate rows followed by N up rows
  bool same_shape(int N_, int K_, int swiglu_) const { return N == N_ && K == K_ && (swiglu != 0) == (swiglu_ != 0); }  // swiglu is a flag
};

using Mxfp4Table = BindTable<Mxfp4Binding>;  // lookup(codes, N, K, swiglu, &binding)
