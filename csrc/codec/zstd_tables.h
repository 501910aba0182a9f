// Zstandard (RFC 8878) entropy tables: FSE decoding tables, the reader of an FSE table description, the three
// predefined distributions and the Huffman literal table, written so that host and device code can share them
// (the host decoder csrc/codec/zstd.cc uses them today; see inflate_tables.h for the same arrangement).
//
// FSE table entry (uint32): symbol | nbits << 8 | baseline << 16. The next state is baseline + nbits fresh bits.
// Huffman table entry (uint16): symbol | nbits << 8, indexed by the next `max_bits` bits of the backward stream,
// first-read bit highest.
// Every builder checks the capacity it is given and refuses what the format forbids: probabilities that do not sum
// to the table size, an accuracy log above the format's maximum, weights that do not complete a power of two.
// (libzstd refuses these too; where the decoders built on this header and libzstd 1.4.8 are known to part ways is
// listed in docs/ARCHITECTURE.md, "zstd map outputs".)
// Every function takes its scratch from the caller (no local arrays).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIP__)  // clang HIP language mode (.hip translation units)
#define UDA_ZSTD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define UDA_ZSTD_HD inline
#endif

namespace uda {
namespace zstd {

constexpr int kLlMaxLog = 9, kOfMaxLog = 8, kMlMaxLog = 9;     // accuracy-log maxima of the sequence tables
constexpr int kLlMaxSym = 35, kOfMaxSym = 31, kMlMaxSym = 52;  // highest code of each
constexpr int kLlCap = 1 << kLlMaxLog, kOfCap = 1 << kOfMaxLog, kMlCap = 1 << kMlMaxLog;
constexpr int kHufMaxBits = 11, kHufCap = 1 << kHufMaxBits;  // literal codes are at most 11 bits long
constexpr int kHufMaxSyms = 256;
constexpr int kWeightMaxLog = 6, kWeightMaxSym = 12, kWeightCap = 1 << kWeightMaxLog;  // FSE-compressed weights
constexpr int kMaxSyms = 53;                                                           // norm / work entries of an FSE build
constexpr uint32_t kBlockMax = 128 * 1024;

UDA_ZSTD_HD int highbit(uint32_t v) { return 31 - __builtin_clz(v); }  // v != 0

UDA_ZSTD_HD uint32_t fse_sym(uint32_t e) { return e & 0xFF; }
UDA_ZSTD_HD uint32_t fse_nbits(uint32_t e) { return (e >> 8) & 0xFF; }
UDA_ZSTD_HD uint32_t fse_base(uint32_t e) { return e >> 16; }

// The decoding table of a normalised distribution norm[0, nsym) (-1 = "less than one": a single cell at the
// table's end) with accuracy log `alog`. work: nsym uint16. false: the table does not fit `cap`, or the
// probabilities do not sum to 1 << alog.
UDA_ZSTD_HD bool fse_build(const int16_t* norm, int nsym, int alog, uint32_t* table, int cap, uint16_t* work) {
  if (alog < 0 || alog > 15 || nsym < 1 || nsym > 256) return false;
  const int size = 1 << alog;
  if (size > cap) return false;
  int sum = 0;
  for (int s = 0; s < nsym; ++s) {
    if (norm[s] < -1) return false;
    sum += norm[s] == -1 ? 1 : norm[s];
  }
  if (sum != size) return false;
  int high = size - 1;
  for (int s = 0; s < nsym; ++s) {
    if (norm[s] == -1) {
      table[high--] = (uint32_t)s;
      work[s] = 1;
    } else {
      work[s] = (uint16_t)norm[s];
    }
  }
  const int step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
  int pos = 0;
  for (int s = 0; s < nsym; ++s) {
    for (int i = 0; i < norm[s]; ++i) {
      table[pos] = (uint32_t)s;
      do pos = (pos + step) & mask;
      while (pos > high);
    }
  }
  if (pos != 0) return false;
  for (int u = 0; u < size; ++u) {
    const uint32_t s = table[u] & 0xFF;
    const uint32_t next = work[s]++;
    const int nbits = alog - highbit(next);
    table[u] = s | (uint32_t)nbits << 8 | (((next << nbits) - (uint32_t)size) & 0xFFFF) << 16;
  }
  return true;
}

// A table of one cell for `sym` (RLE mode): no bits are ever read.
UDA_ZSTD_HD void fse_build_rle(uint32_t sym, uint32_t* table) { table[0] = sym & 0xFF; }

// Reads an FSE table description from src[0, n) (forward bits, LSB first). norm holds max_sym + 1 entries.
// false: truncated, an accuracy log above max_log, a symbol above max_sym, or probabilities that overshoot.
UDA_ZSTD_HD bool fse_read_description(const uint8_t* src, size_t n, int max_log, int max_sym, int16_t* norm, int* nsym,
                                      int* alog, size_t* used) {
  uint64_t bit = 0;
  const uint64_t end = (uint64_t)n * 8;
  bool ok = true;
  auto take = [&](int nb) -> uint32_t {
    if (bit + (uint64_t)nb > end) {
      ok = false;
      return 0;
    }
    uint32_t v = 0;
    for (int i = 0; i < nb; ++i, ++bit) v |= (uint32_t)((src[bit >> 3] >> (bit & 7)) & 1) << i;
    return v;
  };
  const int log = 5 + (int)take(4);
  if (!ok || log > max_log) return false;
  int remaining = 1 << log, sym = 0;
  while (remaining > 0 && sym <= max_sym) {
    const int bits = highbit((uint32_t)remaining + 1) + 1;
    uint32_t val = take(bits);
    if (!ok) return false;
    const uint32_t lower = (1u << (bits - 1)) - 1;
    const uint32_t threshold = (1u << bits) - 1 - ((uint32_t)remaining + 1);
    if ((val & lower) < threshold) {
      --bit;
      val &= lower;
    } else if (val > lower) {
      val -= threshold;
    }
    const int proba = (int)val - 1;
    const int cost = proba < 0 ? 1 : proba;
    if (cost > remaining) return false;
    remaining -= cost;
    norm[sym++] = (int16_t)proba;
    if (proba == 0) {
      uint32_t rep = take(2);
      for (;;) {
        if (!ok) return false;
        for (uint32_t i = 0; i < rep; ++i) {
          if (sym > max_sym) return false;
          norm[sym++] = 0;
        }
        if (rep != 3) break;
        rep = take(2);
      }
    }
  }
  if (remaining != 0) return false;  // more symbols than the table has (the description overshoots)
  *nsym = sym;
  *alog = log;
  *used = (size_t)((bit + 7) >> 3);
  return true;
}

// The predefined distributions (RFC 8878, 3.1.1.3.2.2).
UDA_ZSTD_HD int predefined_ll(int16_t* norm, int* alog) {
  for (int i = 0; i < 36; ++i) norm[i] = i == 0 ? 4 : i == 1 || i == 25 ? 3 : i < 13 ? 2 : i < 16 ? 1 : i < 25 ? 2 : i == 26 ? 2 : i < 32 ? 1 : -1;
  *alog = 6;
  return 36;
}
UDA_ZSTD_HD int predefined_ml(int16_t* norm, int* alog) {
  for (int i = 0; i < 53; ++i) norm[i] = i == 0 ? 1 : i == 1 ? 4 : i == 2 ? 3 : i < 9 ? 2 : i < 46 ? 1 : -1;
  *alog = 6;
  return 53;
}
UDA_ZSTD_HD int predefined_of(int16_t* norm, int* alog) {
  for (int i = 0; i < 29; ++i) norm[i] = i < 6 ? 1 : i < 9 ? 2 : i < 24 ? 1 : -1;
  *alog = 5;
  return 29;
}

// Baseline and extra bits of a literal-length / match-length code.
UDA_ZSTD_HD uint32_t ll_bits(uint32_t c) {
  return c < 16 ? 0 : c < 20 ? 1 : c < 22 ? 2 : c < 24 ? 3 : c == 24 ? 4 : c - 19;
}
UDA_ZSTD_HD uint32_t ll_base(uint32_t c) {
  return c < 16 ? c : c < 20 ? 16 + 2 * (c - 16) : c < 22 ? 24 + 4 * (c - 20) : c < 24 ? 32 + 8 * (c - 22) : c == 24 ? 48 : 1u << (c - 19);
}
UDA_ZSTD_HD uint32_t ml_bits(uint32_t c) {
  return c < 32 ? 0 : c < 36 ? 1 : c < 38 ? 2 : c < 40 ? 3 : c < 42 ? 4 : c == 42 ? 5 : c - 36;
}
UDA_ZSTD_HD uint32_t ml_base(uint32_t c) {
  return c < 32 ? c + 3 : c < 36 ? 35 + 2 * (c - 32) : c < 38 ? 43 + 4 * (c - 36) : c < 40 ? 51 + 8 * (c - 38) :
         c < 42 ? 67 + 16 * (c - 40) : c == 42 ? 99 : (1u << (c - 36)) + 3;
}

// The Huffman table of weights[0, nw): the last symbol's weight is not stored and completes the sum to a power of
// two. weights must hold nw + 1 entries; rank: 16 uint32 of scratch. false: more than 255 stored weights, a weight above 11, a sum
// that needs codes longer than 11 bits, a rest that is no power of two, or fewer than two symbols of weight 1.
UDA_ZSTD_HD bool huf_build(uint8_t* weights, int nw, uint16_t* table, int cap, int* max_bits, uint32_t* rank) {
  if (nw < 1 || nw > kHufMaxSyms - 1) return false;
  uint32_t sum = 0;
  for (int i = 0; i < nw; ++i) {
    if (weights[i] > kHufMaxBits) return false;
    if (weights[i]) sum += 1u << (weights[i] - 1);
  }
  if (sum == 0) return false;
  const int bits = highbit(sum) + 1;
  if (bits > kHufMaxBits || (1 << bits) > cap) return false;
  const uint32_t left = (1u << bits) - sum;
  if (left & (left - 1)) return false;  // (left >= 1: sum < 1 << bits)
  weights[nw] = (uint8_t)(highbit(left) + 1);
  const int nsym = nw + 1;
  for (int w = 0; w < 16; ++w) rank[w] = 0;
  for (int i = 0; i < nsym; ++i) ++rank[weights[i]];
  if (rank[1] < 2 || (rank[1] & 1)) return false;
  uint32_t pos = 0;
  for (int w = 1; w <= bits; ++w) {  // rank[w] becomes where weight w's cells start
    const uint32_t count = rank[w];
    rank[w] = pos;
    pos += count << (w - 1);
  }
  if (pos != (1u << bits)) return false;
  for (int s = 0; s < nsym; ++s) {
    const int w = weights[s];
    if (!w) continue;
    const uint32_t len = 1u << (w - 1), e = (uint32_t)s | (uint32_t)(bits + 1 - w) << 8;
    for (uint32_t i = 0; i < len; ++i) table[rank[w] + i] = (uint16_t)e;
    rank[w] += len;
  }
  *max_bits = bits;
  return true;
}

// Backward bitstream: nb bits at [bit - nb, bit) of p[0, n); bits below the stream's first read as zero.
UDA_ZSTD_HD uint64_t back_bits(const uint8_t* p, size_t n, int64_t bit, int nb) {
  if (nb <= 0) return 0;
  int64_t lo = bit - nb;
  int shift = 0;
  if (lo < 0) {
    if (-lo >= nb) return 0;
    shift = (int)-lo;
    nb -= shift;
    lo = 0;
  }
  const size_t byte = (size_t)(lo >> 3);
  uint64_t w = 0;
  for (size_t i = 0; i < 8 && byte + i < n; ++i) w |= (uint64_t)p[byte + i] << (8 * i);
  w >>= (lo & 7);
  return (w & ((1ull << nb) - 1)) << shift;  // nb <= 32 here
}
// Where a backward stream's first bit lies: below the highest set bit of its last byte (0 there = corrupt: -1).
UDA_ZSTD_HD int64_t back_start(const uint8_t* p, size_t n) {
  if (n == 0 || p[n - 1] == 0) return -1;
  return (int64_t)(n - 1) * 8 + highbit(p[n - 1]);
}

// Scratch of huf_read_description (on the device it lives in LDS).
struct HufScratch {
  uint8_t weights[kHufMaxSyms];
  int16_t norm[kWeightMaxSym + 1];
  uint16_t work[kWeightMaxSym + 1];
  uint32_t fse[kWeightCap];
  uint32_t rank[16];
};
enum HufStatus : int { kHufOk = 0, kHufTruncated = 1, kHufBadWeights = 2, kHufIncomplete = 3 };
// The Huffman tree description at p[0, n): direct 4-bit weights (header byte >= 128) or FSE-compressed weights
// decoded by two interleaved states. Builds `table`; *used = the description's bytes, *fse_coded = which encoding.
UDA_ZSTD_HD int huf_read_description(const uint8_t* p, size_t n, uint16_t* table, int cap, int* bits, size_t* used,
                                     bool* fse_coded, HufScratch* w) {
  if (n < 1) return kHufTruncated;
  int nw = 0;
  const uint32_t h = p[0];
  if (h >= 128) {
    nw = (int)h - 127;
    *used = 1 + (size_t)(nw + 1) / 2;
    if (*used > n) return kHufTruncated;
    for (int i = 0; i < nw; ++i) w->weights[i] = i & 1 ? p[1 + i / 2] & 15 : p[1 + i / 2] >> 4;
    *fse_coded = false;
  } else {
    *used = 1 + (size_t)h;
    if (h == 0 || *used > n) return kHufTruncated;
    int nsym = 0, alog = 0;
    size_t hdr = 0;
    if (!fse_read_description(p + 1, h, kWeightMaxLog, kWeightMaxSym, w->norm, &nsym, &alog, &hdr)) return kHufBadWeights;
    if (!fse_build(w->norm, nsym, alog, w->fse, kWeightCap, w->work)) return kHufBadWeights;
    const uint8_t* b = p + 1 + hdr;
    const size_t bn = h - hdr;
    int64_t bit = back_start(b, bn);
    if (bit < 0) return kHufBadWeights;
    const uint32_t mask = (1u << alog) - 1;
    uint32_t s1 = (uint32_t)back_bits(b, bn, bit, alog);
    bit -= alog;
    uint32_t s2 = (uint32_t)back_bits(b, bn, bit, alog);
    bit -= alog;
    if (bit < 0) return kHufBadWeights;
    for (;;) {  // every turn stores at least one weight and takes the streams toward their start
      if (nw > kHufMaxSyms - 3) return kHufBadWeights;
      uint32_t e = w->fse[s1 & mask];
      w->weights[nw++] = (uint8_t)fse_sym(e);
      s1 = fse_base(e) + (uint32_t)back_bits(b, bn, bit, (int)fse_nbits(e));
      bit -= fse_nbits(e);
      e = w->fse[s2 & mask];
      if (bit < 0) {
        w->weights[nw++] = (uint8_t)fse_sym(e);
        break;
      }
      w->weights[nw++] = (uint8_t)fse_sym(e);
      s2 = fse_base(e) + (uint32_t)back_bits(b, bn, bit, (int)fse_nbits(e));
      bit -= fse_nbits(e);
      if (bit < 0) {
        w->weights[nw++] = (uint8_t)fse_sym(w->fse[s1 & mask]);
        break;
      }
    }
    *fse_coded = true;
  }
  return huf_build(w->weights, nw, table, cap, bits, w->rank) ? kHufOk : kHufIncomplete;
}

// The 1-based repeat-offset rule: `value` is the decoded Offset_Value; rep the three recent offsets. Returns the
// offset to use and updates rep.
UDA_ZSTD_HD uint32_t apply_offset(uint32_t value, uint32_t ll, uint32_t* rep) {
  uint32_t off;
  if (value > 3) {
    off = value - 3;
    rep[2] = rep[1];
    rep[1] = rep[0];
    rep[0] = off;
    return off;
  }
  const uint32_t idx = value + (ll == 0 ? 1 : 0);  // 1..4
  if (idx == 1) return rep[0];
  if (idx == 4) {
    off = rep[0] - 1;
    if (off == 0) off = 1;  // (as libzstd does with this corrupt value)
  } else {
    off = idx == 2 ? rep[1] : rep[2];
  }
  if (idx != 2) rep[2] = rep[1];
  rep[1] = rep[0];
  rep[0] = off;
  return off;
}

}  // namespace zstd
}  // namespace uda
