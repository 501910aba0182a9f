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
constexpr int kColpackMaxRecordBytes = 256;
constexpr int kColpackMaxGroups = kColpackMaxRecordBytes / 8;
constexpr uint32_t kColpackFlagPacked = 1;  // flags bit 0: rows follow (else raw: header only)

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
  uint32_t reserved[7];
  uint64_t mask[kColpackMaxGroups];  // byte c: (1 << w_c) - 1 (0 past a tail group's columns)
  uint64_t base[kColpackMaxGroups];  // byte c: min_c
  uint8_t gb[kColpackMaxGroups];     // packed bytes of the group's word
  uint8_t pad[32];
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

// Reference encoder: statistics over the nrec records at src, header and (unless raw) rows into dst,
// which holds colpack_bound(L, nrec) bytes. Returns the bytes written (header only for a raw piece);
// 0 when L is out of range or nrec < 1.
int64_t colpack_encode(const uint8_t* src, int64_t nrec, int L, int64_t buf_records, uint8_t* dst);

// A piece's header after its checks: magic, version, record length, record count, group count and
// group sizes against the stride, the stride against the piece's length.
struct ColpackPiece {
  const ColpackHeader* hdr = nullptr;
  const uint8_t* rows = nullptr;
  int L = 0;
  int64_t records = 0;
  int64_t stride = 0;
  bool packed = false;
};
// piece: `len` readable bytes. expect_L / expect_records: what the receiver was told to expect
// (<= 0: any). Returns false (and a reason) for a header that fails a check; such a piece must not
// be unpacked.
bool colpack_open(const uint8_t* piece, int64_t len, int expect_L, int64_t expect_records, ColpackPiece* out,
                  const char** why = nullptr);

// Unpack rows [row0, row0 + rows) of an opened, packed piece into dst (rows * L bytes, not one more).
// A range that is not inside the piece unpacks nothing.
// colpack_unpack picks the BMI2 path when the CPU has it (checked once), else the scalar one.
void colpack_unpack(const ColpackPiece& p, int64_t row0, int64_t rows, uint8_t* dst);
void colpack_unpack_scalar(const ColpackPiece& p, int64_t row0, int64_t rows, uint8_t* dst);
// false when this CPU has no BMI2 (nothing written).
bool colpack_unpack_bmi2(const ColpackPiece& p, int64_t row0, int64_t rows, uint8_t* dst);
bool colpack_have_bmi2();

}  // namespace uda
