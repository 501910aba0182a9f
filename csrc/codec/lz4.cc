// In-tree LZ4 block-format encoder/decoder (host). Hadoop's Lz4Codec puts the raw LZ4 *block* format
// into every chunk: no frame header, no stored length. The reference has no LZ4 (its getCompAlg
// throws on it); this is written from the format description:
//   sequence := token [literal-length extension] literals offset(2 B LE) [match-length extension]
//   token    := (literal length << 4) | (match length - 4); a nibble of 15 is followed by extension
//               bytes, each 255 adding 255, the first byte below 255 ending the run
//   the last sequence ends after its literals and has no offset.
// The decoder is the safe variant: every read and write is bounds checked, and the only accepted
// ending is the input running out right after a literal run. The encoder is a greedy single-probe
// hash compressor that keeps the format's end-of-block rules (the last 5 bytes are literals, no match
// starts in the last 12 bytes), so a stock liblz4 decoder accepts its output.
#include <cstring>

#include "uda/codec.h"

namespace uda {

namespace {
constexpr size_t kMinMatch = 4;
constexpr size_t kLastLiterals = 5;  // the last 5 bytes of a block are literals
constexpr size_t kMfLimit = 12;      // no match starts in the last 12 bytes
constexpr size_t kMaxOffset = 65535;

inline uint32_t load32(const uint8_t* p) {
  uint32_t v;
  std::memcpy(&v, p, 4);
  return v;
}

uint8_t* emit_length(uint8_t* op, size_t rest) {  // the extension run of a nibble of 15
  while (rest >= 255) {
    *op++ = 255;
    rest -= 255;
  }
  *op++ = (uint8_t)rest;
  return op;
}

// One sequence: `lit_len` literals, then (m_len != 0) a match. Returns the new output position.
uint8_t* emit_sequence(uint8_t* op, const uint8_t* lit, size_t lit_len, size_t m_off, size_t m_len) {
  uint8_t* token = op++;
  const size_t ml = m_len ? m_len - kMinMatch : 0;
  *token = (uint8_t)((lit_len >= 15 ? 15 : lit_len) << 4 | (ml >= 15 ? 15 : ml));
  if (lit_len >= 15) op = emit_length(op, lit_len - 15);
  std::memcpy(op, lit, lit_len);
  op += lit_len;
  if (m_len) {
    *op++ = (uint8_t)m_off;
    *op++ = (uint8_t)(m_off >> 8);
    if (ml >= 15) op = emit_length(op, ml - 15);
  }
  return op;
}
}  // namespace

size_t lz4_max_compressed_length(size_t n) { return n + n / 255 + 16; }

size_t lz4_compress(const uint8_t* src, size_t n, uint8_t* dst) {
  uint8_t* op = dst;
  constexpr int kBits = 14;
  static thread_local uint32_t table[1 << kBits];
  size_t ip = 0, lit = 0;
  if (n > kMfLimit) {
    std::memset(table, 0xFF, sizeof(table));
    const size_t mf_end = n - kMfLimit;       // a match starts below this
    const size_t m_end = n - kLastLiterals;   // and ends at or below this
    while (ip < mf_end) {
      const uint32_t h = (load32(src + ip) * 2654435761u) >> (32 - kBits);
      const uint32_t cand = table[h];
      table[h] = (uint32_t)ip;
      if (cand != 0xFFFFFFFFu && ip - cand <= kMaxOffset && load32(src + cand) == load32(src + ip)) {
        size_t len = kMinMatch;
        while (ip + len < m_end && src[cand + len] == src[ip + len]) ++len;
        op = emit_sequence(op, src + lit, ip - lit, ip - cand, len);
        ip += len;
        lit = ip;
      } else {
        ++ip;
      }
    }
  }
  return (size_t)(emit_sequence(op, src + lit, n - lit, 0, 0) - dst);
}

bool lz4_decompress(const uint8_t* in, size_t in_len, uint8_t* out, size_t cap, size_t* out_len) {
  size_t ip = 0, op = 0;
  for (;;) {
    if (ip >= in_len) return false;  // the input ends where a token is due
    const uint32_t token = in[ip++];
    size_t len = token >> 4;
    if (len == 15) {
      uint32_t b;
      do {
        if (ip >= in_len) return false;
        b = in[ip++];
        len += b;
      } while (b == 255);
    }
    // lengths are compared against what is left, so a long extension run cannot wrap
    if (len > in_len - ip || len > cap - op) return false;
    if (len) std::memcpy(out + op, in + ip, len);
    ip += len;
    op += len;
    if (ip == in_len) break;  // the one valid ending: right after a literal run
    if (in_len - ip < 2) return false;
    const size_t off = (size_t)in[ip] | ((size_t)in[ip + 1] << 8);
    ip += 2;
    if (off == 0 || off > op) return false;
    len = token & 15;
    if (len == 15) {
      uint32_t b;
      do {
        if (ip >= in_len) return false;
        b = in[ip++];
        len += b;
      } while (b == 255);
    }
    len += kMinMatch;
    if (len > cap - op) return false;
    const uint8_t* m = out + op - off;
    for (size_t i = 0; i < len; ++i) out[op + i] = m[i];  // overlapping copy
    op += len;
  }
  *out_len = op;
  return true;
}

}  // namespace uda
