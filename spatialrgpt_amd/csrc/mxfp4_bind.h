// Which MXFP4 code arrays have a packed copy in MFMA-operand order (srgpt_pack_mxfp4, include/srgpt.h) that a decode-shaped step of
// 2+ rows may multiply instead: a host-side table keyed by the code array's address, filled by srgpt_mxfp4_bind and consulted by
// model.hip's DecodeStep on the host only, at eager launch and at graph capture.  srgpt_llm_weights cannot grow (its layout is the
// ABI), so the copies reach the step this way -- the rules of pack13_bind.h.
// Plain C++ (no HIP): tests/test_host_mxfp4_bind.py compiles this header into a stand-alone program.
#pragma once
#include <mutex>
#include <unordered_map>

struct Mxfp4Binding {
  const void* packed;  // srgpt_mxfp4_packed_bytes(N, K, swiglu)
  int N, K, swiglu;    // swiglu: the matrix is N gate rows followed by N up rows
};

class Mxfp4Table {
 public:
  // a second bind of the same code array replaces the first
  void bind(const void* codes, const Mxfp4Binding& b) {
    std::lock_guard<std::mutex> g(mu_);
    map_[codes] = b;
  }
  bool unbind(const void* codes) {
    std::lock_guard<std::mutex> g(mu_);
    return map_.erase(codes) != 0;
  }
  bool bound(const void* codes) const {
    std::lock_guard<std::mutex> g(mu_);
    return map_.count(codes) != 0;
  }
  // the binding of `codes` if it was made for exactly this shape: a matrix of another shape at a recycled address never matches
  bool lookup(const void* codes, int N, int K, int swiglu, Mxfp4Binding* out) const {
    std::lock_guard<std::mutex> g(mu_);
    const auto it = map_.find(codes);
    if (it == map_.end() || it->second.N != N || it->second.K != K || (it->second.swiglu != 0) != (swiglu != 0)) return false;
    *out = it->second;
    return true;
  }
  size_t size() const {
    std::lock_guard<std::mutex> g(mu_);
    return map_.size();
  }

 private:
  mutable std::mutex mu_;
  std::unordered_map<const void*, Mxfp4Binding> map_;
};
