// A host-side table from a weight matrix's address to the binding of its repacked copy (pack13_bind.h, mxfp4_bind.h): filled by a
// bind entry point of the C ABI and consulted by model.hip's decode steps on the host only, at eager launch and at graph capture.
// srgpt_llm_weights cannot grow (its layout is the ABI), so the copies reach the steps this way.
// A Binding names the shape it was made for with `bool same_shape(shape...) const`; lookup takes that shape between the key and the
// result.  Plain C++ (no HIP): the host tests compile the two headers into stand-alone programs.
#pragma once
#include <mutex>
#include <unordered_map>

template <class Binding, class SameShape = decltype(&Binding::same_shape)>
class BindTable;

template <class Binding, class... Shape>
class BindTable<Binding, bool (Binding::*)(Shape...) const> {
 public:
  // a second bind of the same address replaces the first
  void bind(const void* key, const Binding& b) {
    std::lock_guard<std::mutex> g(mu_);
    map_[key] = b;
  }
  bool unbind(const void* key) {
    std::lock_guard<std::mutex> g(mu_);
    return map_.erase(key) != 0;
  }
  bool bound(const void* key) const {
    std::lock_guard<std::mutex> g(mu_);
    return map_.count(key) != 0;
  }
  // the binding of `key` if it was made for exactly this shape: a matrix of another shape at a recycled address never matches
  bool lookup(const void* key, Shape... shape, Binding* out) const {
    std::lock_guard<std::mutex> g(mu_);
    const auto it = map_.find(key);
    if (it == map_.end() || !it->second.same_shape(shape...)) return false;
    *out = it->second;
    return true;
  }
  size_t size() const {
    std::lock_guard<std::mutex> g(mu_);
    return map_.size();
  }

 private:
  mutable std::mutex mu_;
  std::unordered_map<const void*, Binding> map_;
};
