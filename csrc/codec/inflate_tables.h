// Deflate (RFC 1951) code-length validation and decode-table construction, shared by the host inflater
// (csrc/codec/inflate.cc) and the device inflate kernel (csrc/gpu/inflate.hip): the same code builds the
// tables on both sides, so the host tests and the stand-alone sanitizer program cover what the kernel runs.
//
// Table layout (uint16 entries, bits taken LSB first as deflate packs them):
//   root entry t[bits & ((1 << root) - 1)]:
//     0                                  no code starts with these bits (incomplete code)
//     (sym << 4) | len                   a code of `len` <= root bits for symbol `sym`
//     0x8000 | (off << 4) | sub          codes longer than root: t[off + ((bits >> root) & ((1 << sub) - 1))]
//                                        is 0 or (sym << 4) | len with the code's whole length
// Sub-tables reach to the longest code below their root prefix, as zlib's inftrees does, so its bounds
// hold: 852 entries for 286 literal/length symbols at root 9, 592 for 30 distance symbols at root 6.
// Every function takes its scratch from the caller (no local arrays: on the device they live in LDS).
#pragma once
#include <cstdint>

#if defined(__HIP__)  // clang HIP language mode (.hip translation units)
#define UDA_INFLATE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define UDA_INFLATE_HD inline
#endif

namespace uda {
namespace inflate {

constexpr int kMaxBits = 15;
constexpr int kLitRoot = 9, kDistRoot = 6, kClRoot = 7;
constexpr int kLitCap = 1024, kDistCap = 640, kClCap = 128;  // table entries (see the bounds above)
constexpr int kMaxLit = 288, kMaxDist = 32, kClSyms = 19;    // the fixed code has 288 / 32 lengths
constexpr int kWork = 32;                                    // uint16 scratch entries of build_table
constexpr int kEndOfBlock = 256;
constexpr uint32_t kAdlerMod = 65521;

// Order in which a dynamic header stores the code-length code's lengths.
UDA_INFLATE_HD int cl_order(int i) {
  // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each, packed into two words
  const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                      6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
  const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  return i < 12 ? (int)((lo >> (5 * i)) & 31) : (int)((hi >> (5 * (i - 12))) & 31);
}

// Length symbol 257..285 -> base length and extra bits; distance code 0..29 -> base distance and extra bits.
UDA_INFLATE_HD void length_code(int sym, uint32_t* base, uint32_t* extra) {
  const uint32_t c = (uint32_t)(sym - 257);
  if (c < 8) {
    *base = 3 + c;
    *extra = 0;
  } else if (c == 28) {
    *base = 258;
    *extra = 0;
  } else {
    const uint32_t e = (c - 4) >> 2;
    *base = 3 + ((4 + (c & 3)) << e);
    *extra = e;
  }
}
UDA_INFLATE_HD void dist_code(int code, uint32_t* base, uint32_t* extra) {
  const uint32_t d = (uint32_t)code;
  if (d < 4) {
    *base = 1 + d;
    *extra = 0;
  } else {
    const uint32_t e = (d - 2) >> 1;
    *base = 1 + ((2 + (d & 1)) << e);
    *extra = e;
  }
}

UDA_INFLATE_HD uint32_t bit_reverse(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; ++i) {
    r = (r << 1) | (v & 1);
    v >>= 1;
  }
  return r;
}

UDA_INFLATE_HD void first_codes(const uint16_t* count, uint16_t* next) {
  uint32_t code = 0;
  next[0] = 0;
  for (int len = 1; len <= kMaxBits; ++len) {
    code = (code + count[len - 1]) << 1;
    next[len] = (uint16_t)code;
  }
}

// Build the decode table of `n` code lengths (each 0..15). `work` holds kWork entries. Refuses, as zlib's
// inflate_table does, an over-subscribed set and an incomplete one, except that a set with exactly one
// code of one bit is accepted when allow_single (a block with a single distance code; not the code-length
// code), and one with no code at all always (a block of literals only has no distance code: every lookup
// then finds no code). false = refused, or the table would not fit `cap`.
UDA_INFLATE_HD bool build_table(const uint8_t* lens, int n, int root, bool allow_single, uint16_t* table, int cap,
                        uint16_t* work) {
  uint16_t* count = work;       // [16]
  uint16_t* next = work + 16;   // [16]
  for (int i = 0; i < 16; ++i) count[i] = 0;
  for (int i = 0; i < n; ++i) {
    if (lens[i] > kMaxBits) return false;
    ++count[lens[i]];
  }
  const int used = n - count[0];
  int left = 1;
  for (int len = 1; len <= kMaxBits; ++len) {
    left <<= 1;
    left -= (int)count[len];
    if (left < 0) return false;  // over-subscribed
  }
  if (left > 0 && used != 0 && !(allow_single && used == 1 && count[1] == 1)) return false;  // incomplete
  if ((1 << root) > cap) return false;
  for (int i = 0; i < (1 << root); ++i) table[i] = 0;
  count[0] = 0;  // (lengths of zero take no code)
  // pass 1: short codes fill the root; long ones leave the longest length below their root prefix there
  first_codes(count, next);
  for (int sym = 0; sym < n; ++sym) {
    const int len = lens[sym];
    if (len == 0) continue;
    const uint32_t rev = bit_reverse(next[len]++, len);
    if (len <= root) {
      for (uint32_t i = rev; i < (1u << root); i += 1u << len) table[i] = (uint16_t)((sym << 4) | len);
    } else {
      const uint32_t pre = rev & ((1u << root) - 1);
      const uint16_t sub = (uint16_t)(len - root);
      if ((table[pre] & 0x8000) == 0 || (table[pre] & 15) < sub) table[pre] = (uint16_t)(0x8000 | sub);
    }
  }
  // pass 2: a sub-table for every such prefix
  int top = 1 << root;
  for (int pre = 0; pre < (1 << root); ++pre) {
    if ((table[pre] & 0x8000) == 0) continue;
    const int sub = table[pre] & 15;
    if (top + (1 << sub) > cap || top > 0x7FF) return false;
    for (int i = 0; i < (1 << sub); ++i) table[top + i] = 0;
    table[pre] = (uint16_t)(0x8000 | (top << 4) | sub);
    top += 1 << sub;
  }
  // pass 3: the long codes into their sub-tables
  first_codes(count, next);
  for (int sym = 0; sym < n; ++sym) {
    const int len = lens[sym];
    if (len == 0) continue;
    const uint32_t rev = bit_reverse(next[len]++, len);
    if (len <= root) continue;
    const uint16_t link = table[rev & ((1u << root) - 1)];
    const uint32_t off = (link >> 4) & 0x7FF, sub = link & 15;
    for (uint32_t i = rev >> root; i < (1u << sub); i += 1u << (len - root)) table[off + i] = (uint16_t)((sym << 4) | len);
  }
  return true;
}

// Look a code up in the next bits (at least kMaxBits of them, zeros past the input's end).
// Returns (sym << 4) | len, or 0 when no code matches. Every index is masked into the table built above.
UDA_INFLATE_HD uint32_t lookup(const uint16_t* table, int root, uint32_t bits) {
  uint32_t e = table[bits & ((1u << root) - 1)];
  if (e & 0x8000) {
    const uint32_t off = (e >> 4) & 0x7FF, sub = e & 15;
    e = table[off + ((bits >> root) & ((1u << sub) - 1))];
  }
  return e;
}

// Lengths of the fixed code (BTYPE 1): 288 literal/length lengths at lens[0..288), 32 distance lengths behind
// (symbols 286, 287 and distance codes 30, 31 take part in the code and are refused when they turn up).
UDA_INFLATE_HD void fixed_lengths(uint8_t* lens) {
  for (int i = 0; i < 144; ++i) lens[i] = 8;
  for (int i = 144; i < 256; ++i) lens[i] = 9;
  for (int i = 256; i < 280; ++i) lens[i] = 7;
  for (int i = 280; i < 288; ++i) lens[i] = 8;
  for (int i = 0; i < 32; ++i) lens[288 + i] = 5;
}

// zlib header (RFC 1950): deflate, window <= 32 KiB, check bits, no preset dictionary.
UDA_INFLATE_HD bool zlib_header_ok(uint32_t cmf, uint32_t flg) {
  return (cmf & 15) == 8 && (cmf >> 4) <= 7 && ((cmf << 8) | flg) % 31 == 0 && (flg & 0x20) == 0;
}

}  // namespace inflate
}  // namespace uda
