// The context scratch carver (csrc/carve.hip) on the host, no GPU and no
// library: for a few layouts with odd counts, run once counting and once
// over a buffer of exactly the counted size, the count is the sum of the
// takes (32-bit arrays in whole 8-byte entries), consecutive arrays do not
// overlap and the last ends at the buffer's end.  Built with
// -fsanitize=address,undefined: the test writes every array end to end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../capnproto-java_amd/csrc/carve.hip"

namespace {
int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

struct Arr {
  uint8_t *p;
  uint64_t bytes;  // what the user of the array writes
};

// one layout: 64-bit arrays of a[] entries and 32-bit arrays of b[] values, interleaved
std::vector<Arr> lay(Carve &c, const std::vector<uint64_t> &a, const std::vector<uint64_t> &b) {
  std::vector<Arr> out;
  for (size_t i = 0; i < a.size() || i < b.size(); ++i) {
    if (i < a.size()) out.push_back({reinterpret_cast<uint8_t *>(c.take(a[i])), a[i] * 8});
    if (i < b.size()) out.push_back({reinterpret_cast<uint8_t *>(c.take32(b[i])), b[i] * 4});
  }
  return out;
}

void check(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b) {
  uint64_t sum = 0;
  for (uint64_t k : a) sum += k;
  for (uint64_t k : b) sum += (k + 1) / 2;
  Carve count;
  for (const Arr &r : lay(count, a, b)) CHECK(r.p == nullptr);  // (counting hands out no pointer)
  CHECK(count.n == sum);
  // exactly the counted size, on the heap: a take past it is the sanitizer's
  uint64_t *buf = static_cast<uint64_t *>(std::malloc(sum ? sum * 8 : 1));
  Carve c(buf);
  const std::vector<Arr> arrs = lay(c, a, b);
  CHECK(c.n == sum);
  uint8_t *at = reinterpret_cast<uint8_t *>(buf);
  for (size_t i = 0; i < arrs.size(); ++i) {
    const Arr &r = arrs[i];
    CHECK(r.p >= at);                                // after the one before it
    CHECK((reinterpret_cast<uintptr_t>(r.p) & 7) == 0);  // whole entries
    std::memset(r.p, (int)(i + 1), r.bytes);
    at = r.p + r.bytes;
  }
  CHECK(at <= reinterpret_cast<uint8_t *>(buf + sum));
  // every array still holds its own fill: none was written over by a later one
  for (size_t i = 0; i < arrs.size(); ++i)
    for (uint64_t k = 0; k < arrs[i].bytes; ++k)
      if (arrs[i].p[k] != (uint8_t)(i + 1)) {
        CHECK(!"arrays overlap");
        break;
      }
  std::free(buf);
}
}  // namespace

int main() {
  check({}, {});
  check({1}, {1});
  check({0, 3}, {0, 5});
  check({7, 1, 13}, {3, 64, 1});             // odd 32-bit counts between 64-bit arrays
  check({5, 9, 9, 1}, {515, 7});
  check({514 + 1, 514 + 1}, {514});          // cpk_read_message's head
  check({61, 61, 62, 1, 1}, {61, 64});       // cpk_decode_messages with 61 messages
  check({33, 27, 60, 33, 2}, {33, 64, 1});   // a message batch of 33 segments in 27 messages
  if (failures) return 1;
  std::puts("all passed");
  return 0;
}
