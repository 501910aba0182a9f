// Stand-alone self test of csrc/engine/ifile_checksum.cc (host CRC32, crc32_combine, the trailer split),
// built with -fsanitize=address,undefined by tests/test_ifile_checksum_cpu.py. Never loaded into Python.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "uda/ifile.h"

namespace {
int failures = 0;
void expect(bool ok, const char* what, long a = 0, long b = 0) {
  if (ok) return;
  ++failures;
  std::printf("FAIL %s (%ld, %ld)\n", what, a, b);
}

// the definition: bit by bit
uint32_t crc_bitwise(const uint8_t* p, size_t n, uint32_t crc = 0) {
  crc = ~crc;
  for (size_t i = 0; i < n; ++i) {
    crc ^= p[i];
    for (int k = 0; k < 8; ++k) crc = (crc & 1) ? 0xEDB88320u ^ (crc >> 1) : crc >> 1;
  }
  return ~crc;
}
}  // namespace

int main() {
  using namespace uda;
  expect(crc32_ieee(nullptr, 0) == 0, "crc of nothing");
  expect(crc32_ieee(reinterpret_cast<const uint8_t*>("123456789"), 9) == 0xCBF43926u, "check value");
  std::vector<uint8_t> buf(9000);
  uint64_t x = 88172645463325252ull;
  for (auto& b : buf) {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    b = (uint8_t)(x >> 24);
  }
  // every length 0..70 at every alignment of the first byte, exact-size heap copies (ASan sees one byte over)
  for (size_t off = 0; off < 9; ++off)
    for (size_t n = 0; n <= 70; ++n) {
      std::vector<uint8_t> c(buf.begin() + (long)off, buf.begin() + (long)(off + n));
      expect(crc32_ieee(c.data(), n) == crc_bitwise(c.data(), n), "length sweep", (long)off, (long)n);
    }
  for (size_t n : {4095u, 4096u, 4097u, 8191u}) {
    std::vector<uint8_t> c(buf.begin() + 3, buf.begin() + 3 + (long)n);
    expect(crc32_ieee(c.data(), n, 0xDEADBEEFu) == crc_bitwise(c.data(), n, 0xDEADBEEFu), "seeded", (long)n);
    // the seed is the CRC of what came before
    expect(crc32_ieee(c.data() + 100, n - 100, crc32_ieee(c.data(), 100)) == crc32_ieee(c.data(), n), "running", (long)n);
  }
  for (size_t total : {0u, 1u, 9u, 4096u, 9000u})
    for (size_t cut : {(size_t)0, (size_t)1, total / 2, total}) {
      if (cut > total) continue;
      const uint32_t a = crc32_ieee(buf.data(), cut), b = crc32_ieee(buf.data() + cut, total - cut);
      expect(crc32_combine(a, b, (int64_t)(total - cut)) == crc32_ieee(buf.data(), total), "combine", (long)total, (long)cut);
    }
  // zeros: the length shift alone
  std::vector<uint8_t> z(70000, 0);
  expect(crc32_combine(crc32_ieee(z.data(), 1), crc32_ieee(z.data(), 69999), 69999) == crc32_ieee(z.data(), 70000),
         "combine of zeros");
  // a length beyond 32 bits only multiplies
  expect(crc32_combine(0, 0x12345678u, (int64_t)5 << 32) == 0x12345678u, "combine with crc_a 0");

  // the trailer split of an uncompressed partition
  expect(ifile_trailer_bytes(100, 104) == 4, "trailer present");
  expect(ifile_trailer_bytes(100, 100) == 0, "no trailer");
  expect(ifile_trailer_bytes(0, 4) == 0 && ifile_trailer_bytes(-1, 3) == 0, "an answer that does not say");
  expect(ifile_trailer_bytes(100, 60) == 0 && ifile_trailer_bytes(100, 103) == 0 && ifile_trailer_bytes(100, 105) == 0,
         "anything else");
  const uint8_t t[4] = {0xCB, 0xF4, 0x39, 0x26};
  expect(ifile_stored_checksum(t) == 0xCBF43926u, "big-endian trailer");
  expect(ifile_checksum_mismatch("attempt_x_m_000001_0", 0xCBF43926u, 1, 9) ==
             "IFile checksum mismatch in map output attempt_x_m_000001_0: stored 0xcbf43926, computed 0x00000001 over 9 bytes",
         "message");
  ChecksumMode m = ChecksumMode::kOff;
  expect(checksum_mode_from_conf("auto", &m) && m == ChecksumMode::kAuto, "auto");
  expect(checksum_mode_from_conf("off", &m) && m == ChecksumMode::kOff, "off");
  expect(!checksum_mode_from_conf("maybe", &m) && !checksum_mode_from_conf("", &m) && !checksum_mode_from_conf("AUTO", &m),
         "other values");
  std::printf("ifile checksum selftest: %d failures\n", failures);
  return failures != 0;
}
