// Host side of the FIXED10 delivery, for the reduce tasks of the C ABI (device_reduce.h) and for ShuffleJob's
// consumer threads (device_engine.h) alike: what happens to one D2H piece once it has landed in the pinned ring. A piece stands for whole 104-byte records of one key-range round; it arrives either
// as those records or as a colpack piece (codec/colpack.h) that unpacks to them. Either way the sink gets
// the same buffers: <= kv_buf whole records each, the task's last one carrying the IFile EOF marker when
// it fits and a separate 2-byte buffer after it when it does not.
//
// No HIP here: the CPU tests and the sanitizer self-test (tests/native/fixed_delivery_selftest.cc) build
// this file with codec/colpack.cc alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>

namespace uda {
namespace gpu {

constexpr int64_t kFixedRecordBytes = 104;  // kTeraRecordBytes (kernels.h)
constexpr int64_t kFixedEofBytes = 2;       // the IFile EOF marker (-1, -1)

// mapred.uda.gpu.delivery.pack: "auto" -> 2 (colpack version 2), "v1" -> 1, "off" -> 0; any other value
// -> -1. UDA_DELIVERY_PACK=0 in the environment turns a valid value into 0.
int delivery_pack_version(const std::string& value);

// Geometry of a task's delivery: the pieces of a round, the pinned ring block (SdmaEngine::acquire_ring
// caches by exact size: the prewarm and the task must ask for the same) and, packed, the piece regions of
// the device ring the pieces are packed into.
struct FixedLayout {
  int pack_version = 0;
  int slots = 2;
  int64_t kv_buf_bytes = 0;
  int64_t buf_records = 1, buf_bytes = kFixedRecordBytes;  // whole records per delivery buffer
  int64_t piece = 0, piece_recs = 0;                      // a multiple of buf_bytes: pieces start on buffer bounds
  int64_t slot_bytes = 0;     // one ring slot: the piece, or the bound of its packed form where that is longer
  int64_t region_bytes = 0;   // packed: one piece region of the device ring of packed pieces (64-byte aligned)
  int64_t staging_bytes = 0;  // packed: one of the two unpack staging buffers behind the ring's slots
  size_t ring_bytes = 0;      // slots * slot_bytes (+ 2 * staging_bytes)
  // upper bound of a piece of nrec records in its packed form (version 1 or 2)
  int64_t piece_bound(int64_t nrec) const;
  // The length to copy for a piece of nrec records that the device packed into `packed_bytes`
  // (ColpackResult::bytes): that length, once it is known to hold a header and to fit the piece's bound
  // and a ring slot. Throws std::runtime_error otherwise.
  int64_t packed_copy_len(int64_t packed_bytes, int64_t nrec) const;
  uint8_t* slot(uint8_t* ring, int64_t k) const { return ring + (k % slots) * slot_bytes; }
  uint8_t* staging(uint8_t* ring, int i) const { return ring + (int64_t)slots * slot_bytes + (i & 1) * staging_bytes; }
};
FixedLayout fixed_layout(int64_t kv_buf_bytes, int64_t piece_bytes, int pinned_slots, int pack_version);

// One landed piece.
struct FixedPiece {
  const uint8_t* base = nullptr;
  int64_t copied = 0;        // bytes that crossed the link
  int64_t record_bytes = 0;  // record bytes it stands for (a multiple of 104)
  bool packed = false;       // a colpack piece (else the records themselves)
  bool last = false;         // the task's last piece: EOF follows its records
};
// Buffers the delivery builds in: `staging` (packed pieces are unpacked there, two alternating buffers of
// max(kv_buf, buf_bytes) + 16 bytes: in a hosted task part of the shareable pinned ring block) and `tail`
// (kv_buf + 16 bytes: an unpacked piece's EOF-carrying buffer and the separate EOF buffer).
struct FixedBuffers {
  uint8_t* staging[2] = {nullptr, nullptr};
  uint8_t* tail = nullptr;
  int64_t turn = 0;
};
struct FixedDeliveryCounters {
  int64_t buffers = 0;
  double unpack_ms = 0, sink_ms = 0;
  bool eof_sent = false;
};
using FixedSink = std::function<int(const uint8_t*, int64_t)>;

// Hand the piece's records to the sink in buffers of buf_bytes (the last may be short). A packed piece's
// header is checked first (colpack_open against record_bytes / 104 records): one that fails a check, or
// is not marked packed, throws std::runtime_error before the sink is called and is never unpacked. A
// nonzero sink return throws as well. An empty sink drops the piece: its header is checked and its
// buffers and EOF are counted as with a sink, but nothing is unpacked, copied or written to `bufs`.
void deliver_fixed_piece(const FixedPiece& p, int64_t buf_bytes, int64_t kv_buf_bytes, FixedBuffers& bufs,
                         const FixedSink& sink, FixedDeliveryCounters* c);

}  // namespace gpu
}  // namespace uda
