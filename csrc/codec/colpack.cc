// colpack host side: the reference encoder and the decoder the delivery consumers use (BMI2 pdep or
// portable scalar). Format: codec/colpack.h. Both versions run through one encoder, one header check
// and one pair of decoders: version 1 is "every group byte-aligned, no key".
#include "codec/colpack.h"

#include <cstring>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace uda {

namespace {

typedef unsigned __int128 u128;

inline int bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

inline u128 key_mask(int key_len) { return key_len >= 16 ? ~(u128)0 : (((u128)1 << (8 * key_len)) - 1); }

// A key field of n <= 16 bytes as a big-endian integer. From 8 bytes on: two (overlapping) 8-byte
// accesses, the field's first and last 8 bytes, both inside it.
inline u128 load_be(const uint8_t* p, int n) {
  if (n >= 8) {
    uint64_t hi, lo;
    std::memcpy(&hi, p, 8);
    std::memcpy(&lo, p + n - 8, 8);
    return ((u128)__builtin_bswap64(hi) << (8 * (n - 8))) | __builtin_bswap64(lo);
  }
  u128 v = 0;
  for (int k = 0; k < n; ++k) v = (v << 8) | p[k];
  return v;
}

inline void store_be(uint8_t* p, int n, u128 v) {
  if (n >= 8) {
    const uint64_t hi = __builtin_bswap64((uint64_t)(v >> (8 * (n - 8)))), lo = __builtin_bswap64((uint64_t)v);
    std::memcpy(p, &hi, 8);
    std::memcpy(p + n - 8, &lo, 8);
    return;
  }
  for (int k = n - 1; k >= 0; --k, v >>= 8) p[k] = (uint8_t)v;
}

// Per-group decode tables of an opened piece: byte offset of the load that holds the group's word
// and the word's shift in it, bytes the word touches from there, bit offset of every column in the
// word, columns in the group.
struct Layout {
  int groups = 0;
  int off[kColpackMaxGroups];
  int sh[kColpackMaxGroups];
  int nbytes[kColpackMaxGroups];
  int cols[kColpackMaxGroups];
  uint8_t shift[kColpackMaxGroups][8];
};

Layout layout_of(const ColpackHeader& h, int L) {
  Layout lo;
  lo.groups = colpack_groups(L);
  int bits[kColpackMaxGroups];
  uint16_t bo[kColpackMaxGroups];
  for (int g = 0; g < lo.groups; ++g) {
    lo.cols[g] = L - 8 * g < 8 ? L - 8 * g : 8;
    int sh = 0;
    for (int c = 0; c < 8; ++c) {
      lo.shift[g][c] = (uint8_t)sh;
      sh += __builtin_popcount((unsigned)((h.mask[g] >> (8 * c)) & 0xFF));
    }
    bits[g] = sh;
  }
  colpack_layout(bits, lo.groups, h.version == kColpackVersion, bo);
  for (int g = 0; g < lo.groups; ++g) {
    lo.off[g] = bo[g] >> 3;
    lo.sh[g] = bo[g] & 7;
    lo.nbytes[g] = (lo.sh[g] + bits[g] + 7) / 8;
  }
  return lo;
}

inline uint64_t load_le(const uint8_t* p, int n) {
  uint64_t x = 0;
  for (int k = 0; k < n; ++k) x |= (uint64_t)p[k] << (8 * k);
  return x;
}

// T(r) of a delta piece's row, from its key groups alone (a range that starts inside a buffer).
u128 key_delta_of_row(const ColpackHeader& h, const Layout& lo, const uint8_t* row, int key_off, int key_len) {
  u128 t = 0;
  for (int c = key_off; c < key_off + key_len; ++c) {
    const int g = c / 8, k = c % 8;
    const uint64_t word = load_le(row + lo.off[g], lo.nbytes[g]) >> lo.sh[g];
    const uint64_t m = (h.mask[g] >> (8 * k)) & 0xFF;
    t = (t << 8) | (uint8_t)(((word >> lo.shift[g][k]) & m) + ((h.base[g] >> (8 * k)) & 0xFF));
  }
  return t;
}

// The running key sum of a delta piece's range: rebuilds the key of each row, in dst, in row order.
struct KeyWalk {
  const uint8_t* table = nullptr;
  int64_t buf_records = 1;
  int64_t next_restart = 0;  // first row >= the current one that restarts the sum
  int key_off = 0, key_len = 0;
  u128 mask = 0, sum = 0;

  void start(const ColpackPiece& p, const ColpackHeader& h, const Layout& lo, int64_t row0) {
    table = p.table;
    buf_records = p.buf_records;
    key_off = p.key_off;
    key_len = p.key_len;
    mask = key_mask(key_len);
    const int64_t rs = row0 - row0 % buf_records;
    next_restart = rs;
    if (rs == row0) return;
    sum = load_be(table + rs / buf_records * kColpackRestartBytes, key_len);
    for (int64_t r = rs + 1; r < row0; ++r)
      sum = (sum + key_delta_of_row(h, lo, p.rows + r * p.stride, key_off, key_len)) & mask;
    next_restart = rs + buf_records;
  }
  // rec: the row `row` as the groups left it (key columns hold T)
  inline void fix(int64_t row, uint8_t* rec) {
    if (row == next_restart) {
      sum = load_be(table + row / buf_records * kColpackRestartBytes, key_len);
      next_restart += buf_records;
    } else {
      sum = (sum + load_be(rec + key_off, key_len)) & mask;
    }
    store_be(rec + key_off, key_len, sum);
  }
};

// One encoder for both versions. version 1: key_len 0, byte-aligned groups, gb[] in the header.
int64_t encode(const uint8_t* src, int64_t nrec, int L, int64_t buf_records, uint32_t version, int key_off,
               int key_len, uint8_t* dst) {
  if (L < 1 || L > kColpackMaxRecordBytes || nrec < 1) return 0;
  if (key_off < 0 || key_len < 0 || key_len > kColpackMaxKeyBytes || key_off + key_len > L) return 0;
  uint8_t mn[kColpackMaxRecordBytes], mx[kColpackMaxRecordBytes];
  uint8_t dmn[kColpackMaxKeyBytes], dmx[kColpackMaxKeyBytes];
  std::memset(mn, 0xFF, sizeof(mn));
  std::memset(mx, 0, sizeof(mx));
  std::memset(dmn, 0xFF, sizeof(dmn));
  std::memset(dmx, 0, sizeof(dmx));
  const bool keyed = key_len > 0 && buf_records >= 1;
  const u128 kmask = key_mask(key_len);
  u128 prev = 0;
  for (int64_t r = 0; r < nrec; ++r) {
    const uint8_t* rec = src + r * L;
    for (int c = 0; c < L; ++c) {
      if (rec[c] < mn[c]) mn[c] = rec[c];
      if (rec[c] > mx[c]) mx[c] = rec[c];
    }
    if (keyed) {
      const u128 k = load_be(rec + key_off, key_len);
      uint8_t t[kColpackMaxKeyBytes];
      store_be(t, key_len, r % buf_records == 0 ? (u128)0 : (k - prev) & kmask);
      prev = k;
      for (int c = 0; c < key_len; ++c) {
        if (t[c] < dmn[c]) dmn[c] = t[c];
        if (t[c] > dmx[c]) dmx[c] = t[c];
      }
    }
  }
  int64_t plain_bits = 0, delta_bits = 0;
  for (int c = 0; c < key_len; ++c) {
    plain_bits += bit_length((unsigned)(mx[key_off + c] - mn[key_off + c]));
    delta_bits += bit_length((unsigned)(dmx[c] - dmn[c]));
  }
  const bool delta = colpack2_choose_delta(plain_bits, delta_bits, nrec, buf_records, key_len);
  if (delta)
    for (int c = 0; c < key_len; ++c) {
      mn[key_off + c] = dmn[c];
      mx[key_off + c] = dmx[c];
    }
  ColpackHeader h;
  std::memset(&h, 0, sizeof(h));
  h.magic = kColpackMagic;
  h.version = version;
  h.record_bytes = (uint32_t)L;
  h.records = (uint64_t)nrec;
  h.buf_records = (uint32_t)buf_records;
  h.groups = (uint32_t)colpack_groups(L);
  h.key_off = (uint32_t)key_off;
  h.key_len = (uint32_t)key_len;
  uint8_t shift[kColpackMaxGroups][8];
  int bits[kColpackMaxGroups];
  uint16_t bo[kColpackMaxGroups];
  const int G = (int)h.groups;
  for (int g = 0; g < G; ++g) {
    int b = 0;
    for (int c = 0; c < 8 && 8 * g + c < L; ++c) {
      const int w = bit_length((unsigned)(mx[8 * g + c] - mn[8 * g + c]));
      shift[g][c] = (uint8_t)b;
      b += w;
      h.mask[g] |= (uint64_t)((1u << w) - 1) << (8 * c);
      h.base[g] |= (uint64_t)mn[8 * g + c] << (8 * c);
    }
    bits[g] = b;
  }
  const bool v1 = version == kColpackVersion;
  const int64_t S = colpack_layout(bits, G, v1, bo);
  for (int g = 0; g < G; ++g) {
    if (v1)
      h.gb[g] = (uint8_t)((bits[g] + 7) / 8);
    else
      h.bo[g] = bo[g];
  }
  h.stride = (uint32_t)S;
  const bool raw = colpack_is_raw(S, L);
  h.flags = (raw ? 0 : kColpackFlagPacked) | (delta ? kColpackFlagDelta : 0);
  std::memcpy(dst, &h, sizeof(h));
  if (raw) return (int64_t)kColpackHeaderBytes;
  const int64_t table_bytes = delta ? colpack2_table_bytes(nrec, buf_records) : 0;
  const int64_t total = v1 ? colpack_packed_bytes(S, nrec) : colpack2_packed_bytes(S, nrec, table_bytes);
  std::memset(dst + kColpackHeaderBytes, 0, (size_t)(total - (int64_t)kColpackHeaderBytes));
  if (delta)
    for (int64_t b = 0; b * buf_records < nrec; ++b)
      std::memcpy(dst + kColpackHeaderBytes + b * kColpackRestartBytes, src + b * buf_records * L + key_off,
                  (size_t)key_len);
  uint8_t* rows = dst + kColpackHeaderBytes + table_bytes;
  prev = 0;
  for (int64_t r = 0; r < nrec; ++r) {
    uint8_t rec[kColpackMaxRecordBytes];
    std::memcpy(rec, src + r * L, (size_t)L);
    if (delta) {
      const u128 k = load_be(rec + key_off, key_len);
      store_be(rec + key_off, key_len, r % buf_records == 0 ? (u128)0 : (k - prev) & kmask);
      prev = k;
    }
    uint8_t* row = rows + r * S;
    for (int g = 0; g < G; ++g) {
      uint64_t word = 0;
      for (int c = 0; c < 8 && 8 * g + c < L; ++c)
        word |= (uint64_t)(uint8_t)(rec[8 * g + c] - mn[8 * g + c]) << shift[g][c];
      // (bo & 7) + bits <= 64: the shifted word still fits 64 bits
      const int sh = bo[g] & 7, nb = (sh + bits[g] + 7) / 8;
      word <<= sh;
      for (int k = 0; k < nb; ++k) row[(bo[g] >> 3) + k] |= (uint8_t)(word >> (8 * k));
    }
  }
  return total;
}

}  // namespace

int64_t colpack_encode(const uint8_t* src, int64_t nrec, int L, int64_t buf_records, uint8_t* dst) {
  return encode(src, nrec, L, buf_records, kColpackVersion, 0, 0, dst);
}

int64_t colpack2_encode(const uint8_t* src, int64_t nrec, int L, int64_t buf_records, int key_off, int key_len,
                        uint8_t* dst) {
  if (key_off < 0 || key_len < 0 || key_len > kColpackMaxKeyBytes || key_off + key_len > L) return 0;
  // without buffer restarts there is nothing to take differences from: no key (as the device does)
  if (buf_records < 1 || buf_records > 0xFFFFFFFFll) key_len = 0;
  return encode(src, nrec, L, buf_records, kColpackVersion2, key_len > 0 ? key_off : 0, key_len, dst);
}

bool colpack_open(const uint8_t* piece, int64_t len, int expect_L, int64_t expect_records, ColpackPiece* out,
                  const char** why) {
  auto fail = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  if (!piece || len < (int64_t)kColpackHeaderBytes) return fail("piece shorter than its header");
  const ColpackHeader* h = reinterpret_cast<const ColpackHeader*>(piece);
  ColpackHeader hc;  // the piece may be unaligned: check a copy
  std::memcpy(&hc, piece, sizeof(hc));
  if (hc.magic != kColpackMagic) return fail("bad magic");
  if (hc.version != kColpackVersion && hc.version != kColpackVersion2) return fail("unknown version");
  const bool v1 = hc.version == kColpackVersion;
  const int L = (int)hc.record_bytes;
  if (hc.record_bytes < 1 || hc.record_bytes > (uint32_t)kColpackMaxRecordBytes) return fail("record length out of range");
  if (expect_L > 0 && L != expect_L) return fail("record length differs from the stream's");
  if (hc.records < 1 || hc.records > (uint64_t)1 << 40) return fail("record count out of range");
  if (expect_records > 0 && (int64_t)hc.records != expect_records) return fail("record count differs from the item's");
  if ((int)hc.groups != colpack_groups(L)) return fail("group count does not match the record length");
  int bits[kColpackMaxGroups];
  uint16_t bo[kColpackMaxGroups];
  const int G = (int)hc.groups;
  for (int g = 0; g < G; ++g) {
    bits[g] = 0;
    for (int c = 0; c < 8; ++c) {
      const unsigned m = (unsigned)((hc.mask[g] >> (8 * c)) & 0xFF);
      if (m & (m + 1)) return fail("column mask is not a width mask");
      if (8 * g + c >= L && m) return fail("mask past the tail group's columns");
      bits[g] += __builtin_popcount(m);
    }
    if (v1 && hc.gb[g] != (bits[g] + 7) / 8) return fail("group size does not match its widths");
  }
  const int64_t S = colpack_layout(bits, G, v1, bo);
  if (!v1)
    for (int g = 0; g < kColpackMaxGroups; ++g)
      if (hc.bo[g] != (g < G ? bo[g] : 0)) return fail("group offsets do not match the masks");
  if ((int64_t)hc.stride != S) return fail(v1 ? "row stride does not match the group sizes" : "row stride does not match the masks");
  const bool packed = (hc.flags & kColpackFlagPacked) != 0;
  const bool delta = !v1 && (hc.flags & kColpackFlagDelta) != 0;
  int64_t table_bytes = 0;
  if (!v1) {
    if (hc.flags & ~(kColpackFlagPacked | kColpackFlagDelta)) return fail("unknown flags");
    if (hc.key_len > (uint32_t)kColpackMaxKeyBytes || hc.key_off > (uint32_t)L || hc.key_off + hc.key_len > (uint32_t)L)
      return fail("key field outside the record");
    if (delta && hc.key_len == 0) return fail("delta piece without a key");
    if (delta && hc.buf_records < 1) return fail("delta piece without buffer restarts");
    if (delta) table_bytes = colpack2_table_bytes((int64_t)hc.records, (int64_t)hc.buf_records);
  }
  if (packed) {
    if (colpack_is_raw(S, L)) return fail("packed piece with a raw stride");
    const int64_t need = v1 ? colpack_packed_bytes(S, (int64_t)hc.records)
                            : colpack2_packed_bytes(S, (int64_t)hc.records, table_bytes);
    if (need > len) return fail(v1 ? "rows exceed the piece's length" : "table and rows exceed the piece's length");
  }
  out->hdr = h;
  out->table = piece + kColpackHeaderBytes;
  out->rows = piece + kColpackHeaderBytes + table_bytes;
  out->L = L;
  out->version = (int)hc.version;
  out->records = (int64_t)hc.records;
  out->stride = S;
  out->buf_records = (int64_t)hc.buf_records;
  out->key_off = v1 ? 0 : (int)hc.key_off;
  out->key_len = v1 ? 0 : (int)hc.key_len;
  out->packed = packed;
  out->delta = delta;
  return true;
}

void colpack_unpack_scalar(const ColpackPiece& p, int64_t row0, int64_t rows, uint8_t* dst) {
  if (row0 < 0 || rows <= 0 || row0 + rows > p.records) return;
  ColpackHeader h;  // the piece may be unaligned
  std::memcpy(&h, p.hdr, sizeof(h));
  const Layout lo = layout_of(h, p.L);
  KeyWalk kw;
  if (p.delta) kw.start(p, h, lo, row0);
  for (int64_t r = 0; r < rows; ++r) {
    const uint8_t* row = p.rows + (row0 + r) * p.stride;
    uint8_t* rec = dst + r * p.L;
    for (int g = 0; g < lo.groups; ++g) {
      const uint64_t word = load_le(row + lo.off[g], lo.nbytes[g]) >> lo.sh[g];
      for (int c = 0; c < lo.cols[g]; ++c) {
        const uint64_t m = (h.mask[g] >> (8 * c)) & 0xFF;
        rec[8 * g + c] = (uint8_t)(((word >> lo.shift[g][c]) & m) + ((h.base[g] >> (8 * c)) & 0xFF));
      }
    }
    if (p.delta) kw.fix(row0 + r, rec);
  }
}

bool colpack_have_bmi2() {
#if defined(__x86_64__)
  static const bool have = __builtin_cpu_supports("bmi2");
  return have;
#else
  return false;
#endif
}

#if defined(__x86_64__)
namespace {
// 8-byte loads run up to 7 bytes past a group's word: into the row's next groups, the next row or
// the piece's zero padding (>= 8 bytes after the last row).
// kFull: groups of 8 columns known at compile time (13: TeraSort records, unrolled), 0: from L.
// kDelta: the keys are rebuilt right after the row's groups are written.
template <int kFull, bool kDelta>
__attribute__((target("bmi2"))) void unpack_bmi2(const ColpackPiece& p, int64_t row0, int64_t rows, uint8_t* dst) {
  ColpackHeader h;  // the piece may be unaligned
  std::memcpy(&h, p.hdr, sizeof(h));
  const Layout lo = layout_of(h, p.L);
  const int full = kFull ? kFull : p.L / 8;  // a tail group (L % 8 columns) may follow
  const int tail = kFull ? 0 : p.L % 8;
  const int64_t S = p.stride;
  const int L = p.L;
  KeyWalk kw;
  if (kDelta) kw.start(p, h, lo, row0);
  const uint8_t* row = p.rows + row0 * S;
  for (int64_t r = 0; r < rows; ++r, row += S, dst += L) {
#pragma GCC unroll 16
    for (int g = 0; g < full; ++g) {
      uint64_t x;
      std::memcpy(&x, row + lo.off[g], 8);
      x = _pdep_u64(x >> lo.sh[g], h.mask[g]) + h.base[g];
      std::memcpy(dst + 8 * g, &x, 8);
    }
    if (tail) {
      uint64_t x;
      std::memcpy(&x, row + lo.off[full], 8);
      x = _pdep_u64(x >> lo.sh[full], h.mask[full]) + h.base[full];
      std::memcpy(dst + 8 * full, &x, (size_t)tail);
    }
    if (kDelta) kw.fix(row0 + r, dst);
  }
}
}  // namespace
#endif

bool colpack_unpack_bmi2(const ColpackPiece& p, int64_t row0, int64_t rows, uint8_t* dst) {
#if defined(__x86_64__)
  if (!colpack_have_bmi2()) return false;
  if (row0 < 0 || rows <= 0 || row0 + rows > p.records) return true;
  if (p.L == 104)
    p.delta ? unpack_bmi2<13, true>(p, row0, rows, dst) : unpack_bmi2<13, false>(p, row0, rows, dst);
  else
    p.delta ? unpack_bmi2<0, true>(p, row0, rows, dst) : unpack_bmi2<0, false>(p, row0, rows, dst);
  return true;
#else
  return false;
#endif
}

void colpack_unpack(const ColpackPiece& p, int64_t row0, int64_t rows, uint8_t* dst) {
  if (!colpack_unpack_bmi2(p, row0, rows, dst)) colpack_unpack_scalar(p, row0, rows, dst);
}

}  // namespace uda
