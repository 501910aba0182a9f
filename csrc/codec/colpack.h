// colpack: column-range bit-packing of fixed-length record streams.
//
// Within one piece (a run of whole records of length L) every byte position ("column") c takes values
// in [min_c, max_c]; it is stored as value - min_c in w_c = bit_length(max_c - min_c) bits (0 for a
// constant column, 8 when the range is 128 or more). Columns are taken in groups of 8 consecutive
// ones (the last group of a record whose length is no multiple of 8, the tail group, has L % 8
// columns): a group's word is the w_c low bits of value_c - min_c, c = 0..7, concatenated from the
// least significant bit up and stored little-endian in gb = ceil(sum(w_c) / 8) bytes. A packed row is
// its groups' words one after another (stride S = sum(gb), every group starts on a byte boundary),
// rows follow each other without gaps, and at least 8 zero bytes follow the last row; the piece's
// length is a multiple of 64.
//
//   piece   = header (kColpackHeaderBytes) | nrec rows of S bytes | zero padding
//   decode  = load64 -> pdep(x, mask) -> + base -> store64, per group (the add cannot carry between
//             bytes because value - min <= max - min)
//
// A piece whose stride would exceed 0.9 * L is "raw": its header says so and no rows follow (the
// sender ships the records as they are). The host encoder here is the reference for the device
// kernels (gpu/colpack.hip), which produce the same bytes.
//
// Version 2 (colpack2_encode) keeps the columns, groups and words of version 1 and changes two things:
//
//   piece   = header | restart table | nrec rows of S bytes | zero padding
//
// Key delta. The encoder is told a key field (key_off, key_len <= 16 bytes, big-endian integer K(r)).
// With T(r) = 0 where r % buf_records == 0 and (K(r) - K(r-1)) mod 2^(8 key_len) elsewhere, a "delta"
// piece (flags bit 1) stores T(r)'s big-endian bytes in the key columns instead of the key; sorted
// keys then need far fewer bits. The restart table (delta pieces only) has one 16-byte entry per
// delivery buffer: the key bytes of row b * buf_records as they stand in the record, zero-filled; it
// is padded to a multiple of 64, so rows stay 64-byte aligned. A piece is delta iff key_len > 0,
// buf_records >= 1 and delta_key_bits * nrec + 128 * entries < plain_key_bits * nrec (the key
// columns' widths taken both ways). The sum is modular, so unsorted records round-trip as well.
//
// Bit-contiguous rows. Groups are laid along a bit cursor bo (colpack_layout): a group of 0 bits takes
// nothing; a group whose word would not fit one 8-byte load, (bo & 7) + bits > 64, starts at the next
// byte boundary; S = ceil(bo / 8). The header holds every group's bit offset (bo[]) where version 1
// holds gb[] and pad[]. decode = load64(row + (bo >> 3)) >> (bo & 7) -> pdep -> + base -> store64.
// Version 1 is the same rule with every group byte-aligned and no key.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIP__)  // clang HIP language mode (.hip translation units)
#define UDA_COLPACK_HD __host__ __device__ inline
#else
#define UDA_COLPACK_HD inline
#endif

namespace uda {

constexpr uint32_t kColpackMagic = 0x4b504c43u;  // "CLPK"
constexpr uint32_t kColpackVersion = 1;
constexpr uint32_t kColpackVersion2 = 2;
constexpr int kColpackMaxRecordBytes = 256;
constexpr int kColpackMaxGroups = kColpackMaxRecordBytes / 8;
constexpr uint32_t kColpackFlagPacked = 1;  // flags bit 0: rows follow (else raw: header only)
constexpr uint32_t kColpackFlagDelta = 2;   // flags bit 1 (version 2): key columns hold key differences
constexpr int kColpackMaxKeyBytes = 16;
constexpr int kColpackRestartBytes = 16;    // one restart table entry

// Fixed-size piece header (little-endian host and device).
struct ColpackHeader {
  uint32_t magic;
  uint32_t version;
  uint32_t record_bytes;  // L
  uint32_t flags;
  uint64_t records;
  uint32_t buf_records;   // records per delivery buffer: buffer b starts at row b * buf_records
  uint32_t stride;        // S
  uint32_t groups;        // ceil(L / 8)
  uint32_t key_off;       // version 2: the key field (version 1: 0)
  uint32_t key_len;
  uint32_t reserved[5];
  uint64_t mask[kColpackMaxGroups];  // byte c: (1 << w_c) - 1 (0 past a tail group's columns)
  uint64_t base[kColpackMaxGroups];  // byte c: min_c (delta pieces, key columns: min of T's byte)
  union {
    struct {
      uint8_t gb[kColpackMaxGroups];  // version 1: packed bytes of the group's word
      uint8_t pad[32];
    };
    uint16_t bo[kColpackMaxGroups];   // version 2: bit offset of the group's word in a row
  };
};
constexpr size_t kColpackHeaderBytes = sizeof(ColpackHeader);
static_assert(kColpackHeaderBytes == 640 && kColpackHeaderBytes % 64 == 0, "header is 64-byte aligned");

UDA_COLPACK_HD int colpack_groups(int L) { return (L + 7) / 8; }
// Raw when S > 0.9 * L.
UDA_COLPACK_HD bool colpack_is_raw(int64_t S, int64_t L) { return 10 * S > 9 * L; }
// Largest stride a packed piece can have.
UDA_COLPACK_HD int64_t colpack_max_stride(int64_t L) { return 9 * L / 10; }
// Length of a packed piece: header, rows, >= 8 zero bytes, rounded up to 64.
UDA_COLPACK_HD int64_t colpack_packed_bytes(int64_t S, int64_t nrec) {
  return ((int64_t)kColpackHeaderBytes + S * nrec + 8 + 63) / 64 * 64;
}
// Upper bound of any piece's length (packed or header-only): what a sender reserves per piece.
UDA_COLPACK_HD int64_t colpack_bound(int64_t L, int64_t nrec) { return colpack_packed_bytes(colpack_max_stride(L), nrec); }


// The row layout both versions share. bits[g]: width of group g's word. align_all (version 1): every
// group starts on a byte boundary; else (version 2) only a group that one 8-byte load could not hold.
// bo[g]: the group's bit offset (the cursor's place for a group of 0 bits). Returns the stride.
UDA_COLPACK_HD int colpack_layout(const int* bits, int groups, bool align_all, uint16_t* bo) {
  int cur = 0;
  for (int g = 0; g < groups; ++g) {
    if (bits[g] > 0 && (align_all || (cur & 7) + bits[g] > 64)) cur = (cur + 7) & ~7;
    bo[g] = (uint16_t)cur;
    cur += bits[g];
  }
  return (cur + 7) / 8;
}
// Width of a group's word from its mask (popcount without a builtin: host and device).
UDA_COLPACK_HD int colpack_mask_bits(uint64_t m) {
  int n = 0;
  for (; m; m &= m - 1) ++n;
  return n;
}
// Version 2: restart table of a delta piece and the piece lengths.
UDA_COLPACK_HD int64_t colpack2_table_bytes(int64_t nrec, int64_t buf_records) {
  if (buf_records < 1) return 0;
  return ((nrec + buf_records - 1) / buf_records * kColpackRestartBytes + 63) / 64 * 64;
}
UDA_COLPACK_HD int64_t colpack2_packed_bytes(int64_t S, int64_t nrec, int64_t table_bytes) {
  return ((int64_t)kColpackHeaderBytes + table_bytes + S * nrec + 8 + 63) / 64 * 64;
}
// Upper bound of a version 2 piece: header, table, rows, padding.
UDA_COLPACK_HD int64_t colpack2_bound(int64_t L, int64_t nrec, int64_t buf_records) {
  return colpack2_packed_bytes(colpack_max_stride(L), nrec, colpack2_table_bytes(nrec, buf_records));
}
// delta iff the differences, with their restart table, take fewer bits than the keys
UDA_COLPACK_HD bool colpack2_choose_delta(int64_t plain_key_bits, int64_t delta_key_bits, int64_t nrec,
                                          int64_t buf_records, int key_len) {
  if (key_len <= 0 || buf_records < 1) return false;
  const int64_t entries = (nrec + buf_records - 1) / buf_records;
  return delta_key_bits * nrec + 128 * entries < plain_key_bits * nrec;
}

// Reference encoder: statistics over the nrec records at src, header and (unless raw) rows into dst,
// which holds colpack_bound(L, nrec) bytes. Returns the bytes written (header only for a raw piece);
// 0 when L is out of range or nrec < 1.
int64_t colpack_encode(const uint8_t* src, int64_t nrec, int L, int64_t buf_records, uint8_t* dst);
// Version 2: dst holds colpack2_bound(L, nrec, buf_records) bytes. Also 0 for a key field outside the
// record or longer than kColpackMaxKeyBytes. key_len 0: no key (never delta).
int64_t colpack2_encode(const uint8_t* src, int64_t nrec, int L, int64_t buf_records, int key_off, int key_len,
                        uint8_t* dst);

// A piece's header after its checks: magic, version (1 or 2), record length, record count, group
// count, the layout recomputed from the masks against the header's (group sizes or bit offsets, and
// the stride), the key field against L, buf_records >= 1 for a delta piece, table plus rows against
// the piece's length.
struct ColpackPiece {
  const ColpackHeader* hdr = nullptr;
  const uint8_t* table = nullptr;  // delta pieces: the restart table
  const uint8_t* rows = nullptr;
  int L = 0;
  int version = 0;
  int64_t records = 0;
  int64_t stride = 0;
  int64_t buf_records = 0;
  int key_off = 0, key_len = 0;
  bool packed = false;
  bool delta = false;
};
// piece: `len` readable bytes. expect_L / expect_records: what the receiver was told to expect
// (<= 0: any). Returns false (and a reason) for a header that fails a check; such a piece must not
// be unpacked.
bool colpack_open(const uint8_t* piece, int64_t len, int expect_L, int64_t expect_records, ColpackPiece* out,
                  const char** why = nullptr);

// Unpack rows [row0, row0 + rows) of an opened, packed piece into dst (rows * L bytes, not one more).
// A range that is not inside the piece unpacks nothing. Delta pieces: the keys are rebuilt in dst row
// by row from the restart entry of row0's buffer (a row0 that is no restart row costs a walk over the
// key groups from that buffer's first row).
// colpack_unpack picks the BMI2 path when the CPU has it (checked once), else the scalar one.
void colpack_unpack(const ColpackPiece& p, int64_t row0, int64_t rows, uint8_t* dst);
void colpack_unpack_scalar(const ColpackPiece& p, int64_t row0, int64_t rows, uint8_t* dst);
// false when this CPU has no BMI2 (nothing written).
bool colpack_unpack_bmi2(const ColpackPiece& p, int64_t row0, int64_t rows, uint8_t* dst);
bool colpack_have_bmi2();

}  // namespace uda
