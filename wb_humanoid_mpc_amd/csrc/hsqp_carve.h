// Cutting one byte buffer into arrays (plain C++17, no HIP: tests/carve/carve_check.cpp builds it with a host compiler).
//
// A layout function states the regions of a buffer once, in order, through a Carve, and is run twice: on Carve{} (the sizing pass: every
// pointer null, bytes() what to allocate) and on Carve{buffer} (the binding pass: the typed pointers).  Every region starts on a 256-byte
// boundary of the buffer.
#pragma once
#include <cstddef>

class Carve {
 public:
  explicit Carve(void* base = nullptr) : base_(static_cast<char*>(base)) {}
  // `count` elements of T; an absent region (present == false) is null and takes no space
  template <class T>
  T* take(size_t count, bool present = true) {
    if (!present) return nullptr;
    const size_t at = used_;
    used_ += align256(count * sizeof(T));
    return base_ ? reinterpret_cast<T*>(base_ + at) : nullptr;
  }
  size_t bytes() const { return used_; }

 private:
  static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
  char* base_;
  size_t used_ = 0;
};
