// Compile-time tables of the device CRC32 (crc32.hip). Polynomials are in the reflected representation
// of zlib's crc32 (bit 31 is x^0, polynomial 0xEDB88320). A CRC state s followed by n zero bytes becomes
// s * x^(8n) modulo the polynomial; everything here is such a multiplication tabulated per byte.
#pragma once
#include <cstdint>

namespace uda {
namespace gpu {
namespace crc32tab {

constexpr uint32_t kPoly = 0xEDB88320u;
constexpr int kLanes = 64;
constexpr int kWordBytes = 16;                      // one lane's load
constexpr int kRowBytes = kLanes * kWordBytes;      // one wave's load: 1 KiB
constexpr int64_t kChunkBytes = 256 << 10;          // one wave's chunk: 256 rows
constexpr int kDataTables = 16, kShiftTables = 4;   // byte tables staged in LDS: 20 KiB
constexpr int kTables = kDataTables + kShiftTables;

// a(x) * b(x) modulo the polynomial (zlib's multmodp)
constexpr uint32_t mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & 0x80000000u) p ^= b;
    a <<= 1;
    b = (b & 1) ? (b >> 1) ^ kPoly : b >> 1;
  }
  return p;
}
// x^(2^k)
constexpr uint32_t xpow2(int k) {
  uint32_t v = 0x40000000u;  // x^1
  for (int i = 0; i < k; ++i) v = mul(v, v);
  return v;
}

struct ByteTables {
  // t[k][b], k < 16: the state after byte b and k zero bytes (slice-by-16: the word's byte i takes t[15 - i])
  // t[16 + k][b]: (b << 8k) * x^(8 * kRowBytes): a lane's state carried over the row's other lanes' bytes
  uint32_t t[kTables][256];
};
constexpr ByteTables make_byte_tables() {
  ByteTables tb{};
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? kPoly ^ (c >> 1) : c >> 1;
    tb.t[0][i] = c;
  }
  for (int k = 1; k < kDataTables; ++k)
    for (uint32_t i = 0; i < 256; ++i) tb.t[k][i] = tb.t[0][tb.t[k - 1][i] & 0xFF] ^ (tb.t[k - 1][i] >> 8);
  const uint32_t row = xpow2(13);  // x^(8 * 1024)
  static_assert(8 * kRowBytes == 1 << 13, "shift tables are built for 1 KiB rows");
  for (int k = 0; k < kShiftTables; ++k) {
    tb.t[kDataTables + k][0] = 0;
    for (uint32_t i = 1; i < 256; ++i) {
      const uint32_t low = i & (~i + 1);  // multiplication is linear: one mul per bit, the rest by xor
      tb.t[kDataTables + k][i] = low == i ? mul(i << (8 * k), row) : tb.t[kDataTables + k][i ^ low] ^ tb.t[kDataTables + k][low];
    }
  }
  return tb;
}

struct FoldTables {
  uint32_t lane[kLanes];       // x^(8 * 16 * d): a lane's state carried to the end of the row, d words on
  uint32_t chunk[kLanes + 1];  // x^(8 * kChunkBytes * d): a chunk's state carried d chunks on
};
constexpr FoldTables make_fold_tables() {
  FoldTables f{};
  const uint32_t w = xpow2(7);  // x^128
  static_assert(8 * kWordBytes == 1 << 7, "lane constants are built for 16-byte words");
  f.lane[0] = 0x80000000u;
  for (int d = 1; d < kLanes; ++d) f.lane[d] = mul(f.lane[d - 1], w);
  const uint32_t c = xpow2(21);  // x^(8 * 256 KiB)
  static_assert(8 * kChunkBytes == 1 << 21, "chunk constants are built for 256 KiB chunks");
  f.chunk[0] = 0x80000000u;
  for (int d = 1; d <= kLanes; ++d) f.chunk[d] = mul(f.chunk[d - 1], c);
  return f;
}

}  // namespace crc32tab
}  // namespace gpu
}  // namespace uda
