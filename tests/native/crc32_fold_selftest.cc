// uda::Crc32Running and crc32_fold_state (uda/ifile.h) against crc32_ieee of the whole stream: random buffers cut
// at random points, zero-length segments included, each segment appended as a register from zero (what the
// device's state mode computes) or as host bytes. Built with csrc/engine/ifile_checksum.cc alone, under sanitizers
// (tests/test_crc32_fold_cpu.py).
#include <cstdio>
#include <random>
#include <vector>
#include "uda/ifile.h"
using namespace uda;
int main() {
  std::mt19937_64 rng(5);
  int fails = 0, checks = 0;
  for (int it = 0; it < 200; ++it) {
    std::vector<uint8_t> buf((size_t)(rng() % 700000) + 1);
    for (auto& b : buf) b = (uint8_t)rng();
    Crc32Running run;
    size_t at = 0;
    while (at < buf.size()) {
      size_t n = rng() % 4 == 0 ? 0 : (size_t)(rng() % (buf.size() - at + 1));
      if (rng() & 1) run.append_bytes(buf.data() + at, n);
      else run.append_state(~crc32_ieee(buf.data() + at, n, 0xFFFFFFFFu), (int64_t)n);  // register from zero
      at += n;
    }
    ++checks;
    if (run.value() != crc32_ieee(buf.data(), buf.size()) || run.bytes() != (int64_t)buf.size()) ++fails;
  }
  ++checks; if (crc32_fold_state(0, 0, (1ll << 40)) != 0) ++fails;
  ++checks; if (crc32_fold_state(0x12345678u, 0, 0) != 0x12345678u) ++fails;
  std::printf("%d checks, %d failures\n", checks, fails);
  return fails != 0;
}
