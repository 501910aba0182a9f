// The IFile checksum trailer (uda/ifile.h): host CRC32, crc32_combine, the trailer split of an
// uncompressed partition and the mapred.uda.ifile.checksum values. Host C++ only (no HIP), so the
// stand-alone self test (tests/native/ifile_checksum_selftest.cc) links this file alone.
#include <cstdio>

#include "uda/ifile.h"

namespace uda {

namespace {
constexpr uint32_t kPoly = 0xEDB88320u;

// Slice-by-8 tables: t[0] is the byte table, t[k][b] = the state after byte b and k zero bytes.
struct CrcTables {
  uint32_t t[8][256];
  CrcTables() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? kPoly ^ (c >> 1) : c >> 1;
      t[0][i] = c;
    }
    for (int k = 1; k < 8; ++k)
      for (uint32_t i = 0; i < 256; ++i) t[k][i] = t[0][t[k - 1][i] & 0xFF] ^ (t[k - 1][i] >> 8);
  }
};
const CrcTables& tables() {
  static const CrcTables tb;
  return tb;
}

// a(x) * b(x) modulo the polynomial, reflected representation (bit 31 is x^0), as zlib's multmodp
uint32_t multmodp(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & 0x80000000u) p ^= b;
    a <<= 1;
    b = (b & 1) ? (b >> 1) ^ kPoly : b >> 1;
  }
  return p;
}

// x^(8 * n) by square and multiply over the bits of n, starting from x^8
uint32_t xpow8(uint64_t n) {
  uint32_t pw = 0x80000000u, sq = 0x00800000u;  // x^0, x^8
  for (; n; n >>= 1) {
    if (n & 1) pw = multmodp(pw, sq);
    sq = multmodp(sq, sq);
  }
  return pw;
}
}  // namespace

uint32_t crc32_ieee(const uint8_t* p, size_t n, uint32_t crc) {
  const CrcTables& tb = tables();
  crc = ~crc;
  while (n >= 8) {
    // bytes are taken one by one (no alignment or endianness assumption); the eight lookups are independent
    const uint32_t a = crc ^ ((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
    crc = tb.t[7][a & 0xFF] ^ tb.t[6][(a >> 8) & 0xFF] ^ tb.t[5][(a >> 16) & 0xFF] ^ tb.t[4][a >> 24] ^
          tb.t[3][p[4]] ^ tb.t[2][p[5]] ^ tb.t[1][p[6]] ^ tb.t[0][p[7]];
    p += 8;
    n -= 8;
  }
  for (; n; --n) crc = tb.t[0][(crc ^ *p++) & 0xFF] ^ (crc >> 8);
  return ~crc;
}

uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, int64_t len_b) {
  if (len_b <= 0) return crc_a ^ crc_b;  // (crc of no bytes is 0)
  return multmodp(xpow8((uint64_t)len_b), crc_a) ^ crc_b;
}

// (the map is linear, so it is the same on raw registers as on finalized CRCs: the presets cancel there)
uint32_t crc32_fold_state(uint32_t state, uint32_t seg_state, int64_t seg_len) {
  if (seg_len <= 0) return state ^ seg_state;  // (the state of no bytes is 0)
  return multmodp(xpow8((uint64_t)seg_len), state) ^ seg_state;
}

int ifile_trailer_bytes(int64_t raw_len, int64_t part_len) {
  return raw_len > 0 && part_len == raw_len + kIFileChecksumBytes ? kIFileChecksumBytes : 0;
}

uint32_t ifile_stored_checksum(const uint8_t* t) {
  return ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3];
}

std::string ifile_checksum_mismatch(const std::string& map_id, uint32_t stored, uint32_t computed, int64_t n) {
  char v[96];
  std::snprintf(v, sizeof(v), ": stored 0x%08x, computed 0x%08x over %lld bytes", stored, computed, (long long)n);
  return "IFile checksum mismatch in map output " + map_id + v;
}

bool checksum_mode_from_conf(const std::string& v, ChecksumMode* mode) {
  if (v == "auto") {
    *mode = ChecksumMode::kAuto;
    return true;
  }
  if (v == "off") {
    *mode = ChecksumMode::kOff;
    return true;
  }
  return false;
}

bool checksum_over_budget_from_conf(const std::string& v, bool* verify) {
  if (v != "skip" && v != "verify") return false;
  *verify = v == "verify";
  return true;
}

}  // namespace uda
