// gdd_carve.hpp — workspace carving: 256-byte aligned sub-allocations out of one caller buffer.
// Host-only (no HIP): the same carve measures a layout (null base) and lays it out.
#pragma once

#include <cstddef>

namespace gdd {

struct Carver {
  char* base;
  size_t cap;
  size_t off = 0;
  Carver(void* b, size_t c) : base(static_cast<char*>(b)), cap(c) {}
  template <class T>
  T* take(size_t count) {
    off = (off + 255) & ~size_t(255);
    T* p = reinterpret_cast<T*>(base ? base + off : nullptr);
    off += count * sizeof(T);
    return p;
  }
  bool ok() const { return off <= cap; }
};
// size-only variant used by the *_ws_bytes queries
inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

}  // namespace gdd
