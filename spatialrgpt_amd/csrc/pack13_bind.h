// Which raw bf16 matrices have a 13-bit packed copy (pack13.h) the batch-1 decode step may stream instead: a host-side table keyed
// by the raw matrix's address, filled by srgpt_pack13_bind and consulted by model.hip's decode-layer sequence on the host only, at
// eager launch and at graph capture.  srgpt_llm_weights cannot grow (its layout is the ABI), so the copies reach the step this way.
// Plain C++ (no HIP): tests/test_host_pack13.py compiles this header into a stand-alone program.
#pragma once
#include <mutex>
#include <unordered_map>

struct Pack13Binding {
  const void* packed;  // p13_packed_bytes(rows, K)
  const void* meta;    // p13_meta_bytes(rows)
  int rows, K;         // rows of the matrix (a SwiGLU matrix: gate rows + up rows)
};

class Pack13Table {
 public:
  // a second bind of the same raw address replaces the first
  void bind(const void* raw, const Pack13Binding& b) {
    std::lock_guard<std::mutex> g(mu_);
    map_[raw] = b;
  }
  bool unbind(const void* raw) {
    std::lock_guard<std::mutex> g(mu_);
    return map_.erase(raw) != 0;
  }
  bool bound(const void* raw) const {
    std::lock_guard<std::mutex> g(mu_);
    return map_.count(raw) != 0;
  }
  // the binding of `raw` if it was made for exactly this shape: a matrix of another shape at a recycled address never matches
  bool lookup(const void* raw, int rows, int K, Pack13Binding* out) const {
    std::lock_guard<std::mutex> g(mu_);
    const auto it = map_.find(raw);
    if (it == map_.end() || it->second.rows != rows || it->second.K != K) return false;
    *out = it->second;
    return true;
  }
  size_t size() const {
    std::lock_guard<std::mutex> g(mu_);
    return map_.size();
  }

 private:
  mutable std::mutex mu_;
  std::unordered_map<const void*, Pack13Binding> map_;
};
