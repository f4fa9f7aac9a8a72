// carve.hip -- a scratch buffer's layout, written once as a list of take()
// calls and run twice: over a counting Carve (base null) for the entries to
// reserve, then over the buffer for the pointers.  The size asked for is so
// the sum of what is carved, by construction.  Entries are 8 bytes.  Host
// code without HIP calls: tests/cpp/carve_test.cpp includes this file alone.
#pragma once
#include <cstdint>

struct Carve {
  uint64_t *base;  // the buffer; null: counting only
  uint64_t n = 0;  // entries taken so far
  explicit Carve(uint64_t *p = nullptr) : base(p) {}
  uint64_t *take(uint64_t k) {
    uint64_t *r = base ? base + n : nullptr;
    n += k;
    return r;
  }
  // k 32-bit values, two per entry, in whole entries
  uint32_t *take32(uint64_t k) { return reinterpret_cast<uint32_t *>(take((k + 1) / 2)); }
};
