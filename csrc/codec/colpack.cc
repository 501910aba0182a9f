// colpack host side: the reference encoder and the decoder the delivery consumers use (BMI2 pdep or
// portable scalar). Format: codec/colpack.h.
#include "codec/colpack.h"

#include <cstring>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace uda {

namespace {

inline int bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

// Per-group decode tables of an opened piece: byte offset of the group's word in a row, bit offset
// of every column in the word, columns in the group.
struct Layout {
  int groups = 0;
  int off[kColpackMaxGroups];
  int cols[kColpackMaxGroups];
  uint8_t shift[kColpackMaxGroups][8];
};

Layout layout_of(const ColpackHeader& h, int L) {
  Layout lo;
  lo.groups = colpack_groups(L);
  int off = 0;
  for (int g = 0; g < lo.groups; ++g) {
    lo.off[g] = off;
    lo.cols[g] = L - 8 * g < 8 ? L - 8 * g : 8;
    int sh = 0;
    for (int c = 0; c < 8; ++c) {
      lo.shift[g][c] = (uint8_t)sh;
      sh += __builtin_popcount((unsigned)((h.mask[g] >> (8 * c)) & 0xFF));
    }
    off += h.gb[g];
  }
  return lo;
}

inline uint64_t load_le(const uint8_t* p, int n) {
  uint64_t x = 0;
  for (int k = 0; k < n; ++k) x |= (uint64_t)p[k] << (8 * k);
  return x;
}

}  // namespace

int64_t colpack_encode(const uint8_t* src, int64_t nrec, int L, int64_t buf_records, uint8_t* dst) {
  if (L < 1 || L > kColpackMaxRecordBytes || nrec < 1) return 0;
  uint8_t mn[kColpackMaxRecordBytes], mx[kColpackMaxRecordBytes];
  std::memset(mn, 0xFF, sizeof(mn));
  std::memset(mx, 0, sizeof(mx));
  for (int64_t r = 0; r < nrec; ++r) {
    const uint8_t* rec = src + r * L;
    for (int c = 0; c < L; ++c) {
      if (rec[c] < mn[c]) mn[c] = rec[c];
      if (rec[c] > mx[c]) mx[c] = rec[c];
    }
  }
  ColpackHeader h;
  std::memset(&h, 0, sizeof(h));
  h.magic = kColpackMagic;
  h.version = kColpackVersion;
  h.record_bytes = (uint32_t)L;
  h.records = (uint64_t)nrec;
  h.buf_records = (uint32_t)buf_records;
  h.groups = (uint32_t)colpack_groups(L);
  uint8_t shift[kColpackMaxGroups][8];
  int off[kColpackMaxGroups];
  int64_t S = 0;
  for (int g = 0; g < (int)h.groups; ++g) {
    int bits = 0;
    for (int c = 0; c < 8 && 8 * g + c < L; ++c) {
      const int w = bit_length((unsigned)(mx[8 * g + c] - mn[8 * g + c]));
      shift[g][c] = (uint8_t)bits;
      bits += w;
      h.mask[g] |= (uint64_t)((1u << w) - 1) << (8 * c);
      h.base[g] |= (uint64_t)mn[8 * g + c] << (8 * c);
    }
    h.gb[g] = (uint8_t)((bits + 7) / 8);
    off[g] = (int)S;
    S += h.gb[g];
  }
  h.stride = (uint32_t)S;
  const bool raw = colpack_is_raw(S, L);
  h.flags = raw ? 0 : kColpackFlagPacked;
  std::memcpy(dst, &h, sizeof(h));
  if (raw) return (int64_t)kColpackHeaderBytes;
  uint8_t* rows = dst + kColpackHeaderBytes;
  for (int64_t r = 0; r < nrec; ++r) {
    const uint8_t* rec = src + r * L;
    uint8_t* row = rows + r * S;
    for (int g = 0; g < (int)h.groups; ++g) {
      uint64_t word = 0;
      for (int c = 0; c < 8 && 8 * g + c < L; ++c)
        word |= (uint64_t)(uint8_t)(rec[8 * g + c] - mn[8 * g + c]) << shift[g][c];
      for (int k = 0; k < h.gb[g]; ++k) row[off[g] + k] = (uint8_t)(word >> (8 * k));
    }
  }
  const int64_t total = colpack_packed_bytes(S, nrec);
  std::memset(rows + S * nrec, 0, (size_t)(total - (int64_t)kColpackHeaderBytes - S * nrec));
  return total;
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
  if (hc.version != kColpackVersion) return fail("unknown version");
  const int L = (int)hc.record_bytes;
  if (hc.record_bytes < 1 || hc.record_bytes > (uint32_t)kColpackMaxRecordBytes) return fail("record length out of range");
  if (expect_L > 0 && L != expect_L) return fail("record length differs from the stream's");
  if (hc.records < 1 || hc.records > (uint64_t)1 << 40) return fail("record count out of range");
  if (expect_records > 0 && (int64_t)hc.records != expect_records) return fail("record count differs from the item's");
  if ((int)hc.groups != colpack_groups(L)) return fail("group count does not match the record length");
  int64_t S = 0;
  for (int g = 0; g < (int)hc.groups; ++g) {
    int bits = 0;
    for (int c = 0; c < 8; ++c) {
      const unsigned m = (unsigned)((hc.mask[g] >> (8 * c)) & 0xFF);
      if (m & (m + 1)) return fail("column mask is not a width mask");
      if (8 * g + c >= L && m) return fail("mask past the tail group's columns");
      bits += __builtin_popcount(m);
    }
    if (hc.gb[g] != (bits + 7) / 8) return fail("group size does not match its widths");
    S += hc.gb[g];
  }
  if ((int64_t)hc.stride != S) return fail("row stride does not match the group sizes");
  const bool packed = (hc.flags & kColpackFlagPacked) != 0;
  if (packed) {
    if (colpack_is_raw(S, L)) return fail("packed piece with a raw stride");
    if (colpack_packed_bytes(S, (int64_t)hc.records) > len) return fail("rows exceed the piece's length");
  }
  out->hdr = h;
  out->rows = piece + kColpackHeaderBytes;
  out->L = L;
  out->records = (int64_t)hc.records;
  out->stride = S;
  out->packed = packed;
  return true;
}

void colpack_unpack_scalar(const ColpackPiece& p, int64_t row0, int64_t rows, uint8_t* dst) {
  if (row0 < 0 || rows <= 0 || row0 + rows > p.records) return;
  ColpackHeader h;  // the piece may be unaligned
  std::memcpy(&h, p.hdr, sizeof(h));
  const Layout lo = layout_of(h, p.L);
  for (int64_t r = 0; r < rows; ++r) {
    const uint8_t* row = p.rows + (row0 + r) * p.stride;
    uint8_t* rec = dst + r * p.L;
    for (int g = 0; g < lo.groups; ++g) {
      const uint64_t word = load_le(row + lo.off[g], h.gb[g]);
      for (int c = 0; c < lo.cols[g]; ++c) {
        const uint64_t m = (h.mask[g] >> (8 * c)) & 0xFF;
        rec[8 * g + c] = (uint8_t)(((word >> lo.shift[g][c]) & m) + ((h.base[g] >> (8 * c)) & 0xFF));
      }
    }
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
template <int kFull>
__attribute__((target("bmi2"))) void unpack_bmi2(const ColpackPiece& p, int64_t row0, int64_t rows, uint8_t* dst) {
  ColpackHeader h;  // the piece may be unaligned
  std::memcpy(&h, p.hdr, sizeof(h));
  const Layout lo = layout_of(h, p.L);
  const int full = kFull ? kFull : p.L / 8;  // a tail group (L % 8 columns) may follow
  const int tail = kFull ? 0 : p.L % 8;
  const int64_t S = p.stride;
  const int L = p.L;
  const uint8_t* row = p.rows + row0 * S;
  for (int64_t r = 0; r < rows; ++r, row += S, dst += L) {
#pragma GCC unroll 16
    for (int g = 0; g < full; ++g) {
      uint64_t x;
      std::memcpy(&x, row + lo.off[g], 8);
      x = _pdep_u64(x, h.mask[g]) + h.base[g];
      std::memcpy(dst + 8 * g, &x, 8);
    }
    if (tail) {
      uint64_t x;
      std::memcpy(&x, row + lo.off[full], 8);
      x = _pdep_u64(x, h.mask[full]) + h.base[full];
      std::memcpy(dst + 8 * full, &x, (size_t)tail);
    }
  }
}
}  // namespace
#endif

bool colpack_unpack_bmi2(const ColpackPiece& p, int64_t row0, int64_t rows, uint8_t* dst) {
#if defined(__x86_64__)
  if (!colpack_have_bmi2()) return false;
  if (row0 < 0 || rows <= 0 || row0 + rows > p.records) return true;
  if (p.L == 104)
    unpack_bmi2<13>(p, row0, rows, dst);
  else
    unpack_bmi2<0>(p, row0, rows, dst);
  return true;
#else
  return false;
#endif
}

void colpack_unpack(const ColpackPiece& p, int64_t row0, int64_t rows, uint8_t* dst) {
  if (!colpack_unpack_bmi2(p, row0, rows, dst)) colpack_unpack_scalar(p, row0, rows, dst);
}

}  // namespace uda
