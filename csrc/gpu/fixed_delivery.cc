// Host side of the FIXED10 delivery. See fixed_delivery.h.
#include "fixed_delivery.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "codec/colpack.h"

namespace uda {
namespace gpu {

namespace {
double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
int64_t align64(int64_t v) { return (v + 63) / 64 * 64; }
}  // namespace

int delivery_pack_version(const std::string& value) {
  int v;
  if (value == "auto")
    v = (int)kColpackVersion2;
  else if (value == "v1")
    v = (int)kColpackVersion;
  else if (value == "off")
    v = 0;
  else
    return -1;
  if (const char* e = std::getenv("UDA_DELIVERY_PACK"))
    if (std::atoi(e) == 0) v = 0;
  return v;
}

int64_t FixedLayout::piece_bound(int64_t nrec) const {
  return pack_version == (int)kColpackVersion ? colpack_bound(kFixedRecordBytes, nrec)
                                              : colpack2_bound(kFixedRecordBytes, nrec, buf_records);
}

int64_t FixedLayout::packed_copy_len(int64_t packed_bytes, int64_t nrec) const {
  if (packed_bytes < (int64_t)kColpackHeaderBytes || packed_bytes > piece_bound(nrec) || packed_bytes > slot_bytes)
    throw std::runtime_error("fixed delivery: packed length outside the piece's region");
  return packed_bytes;
}

FixedLayout fixed_layout(int64_t kv_buf_bytes, int64_t piece_bytes, int pinned_slots, int pack_version) {
  FixedLayout l;
  l.pack_version = pack_version;
  l.slots = std::max(2, pinned_slots);
  l.kv_buf_bytes = kv_buf_bytes;
  l.buf_records = std::max<int64_t>(1, kv_buf_bytes / kFixedRecordBytes);
  l.buf_bytes = l.buf_records * kFixedRecordBytes;
  l.piece = std::max<int64_t>(1, piece_bytes / l.buf_bytes) * l.buf_bytes;
  l.piece_recs = l.piece / kFixedRecordBytes;
  l.slot_bytes = l.piece;
  if (pack_version != 0) {
    // a short piece is longer packed than plain (header and restart table): the bound decides, not the piece
    l.region_bytes = align64(l.piece_bound(l.piece_recs));
    l.slot_bytes = std::max(align64(l.piece), l.region_bytes);
    l.staging_bytes = align64(std::max(kv_buf_bytes, l.buf_bytes) + 16);
  }
  l.ring_bytes = (size_t)(l.slots * l.slot_bytes + 2 * l.staging_bytes);
  return l;
}

void deliver_fixed_piece(const FixedPiece& p, int64_t buf_bytes, int64_t kv_buf_bytes, FixedBuffers& bufs,
                         const FixedSink& sink, FixedDeliveryCounters* c) {
  if (buf_bytes < kFixedRecordBytes || buf_bytes % kFixedRecordBytes || p.record_bytes < 0 ||
      p.record_bytes % kFixedRecordBytes)
    throw std::runtime_error("fixed delivery: a piece or buffer that does not hold whole records");
  ColpackPiece pp;
  if (p.packed) {
    const char* why = "";
    if (!colpack_open(p.base, p.copied, (int)kFixedRecordBytes, p.record_bytes / kFixedRecordBytes, &pp, &why))
      throw std::runtime_error(std::string("packed piece rejected: ") + why);
    if (!pp.packed) throw std::runtime_error("packed piece rejected: not marked packed");
  } else if (p.copied != p.record_bytes) {
    throw std::runtime_error("fixed delivery: an unpacked piece of another length than its records");
  }
  const bool drop = !sink;  // no sink: the buffers are counted, none is built
  auto emit = [&](const uint8_t* b, int64_t len) {
    if (!drop) {
      const double a = now_ms();
      if (sink(b, len) != 0) throw std::runtime_error("dataFromUda callback failed");
      c->sink_ms += now_ms() - a;
    }
    c->buffers++;
  };
  for (int64_t off = 0; off < p.record_bytes; off += buf_bytes) {
    const int64_t len = std::min(buf_bytes, p.record_bytes - off);
    const bool eof_here = p.last && off + len >= p.record_bytes && len + kFixedEofBytes <= kv_buf_bytes;
    const uint8_t* out = p.base + off;
    if (drop) {
    } else if (p.packed) {  // this buffer's rows into a staging buffer; the sink gets that
      uint8_t* stg = bufs.staging[bufs.turn++ & 1];
      const double a = now_ms();
      colpack_unpack(pp, off / kFixedRecordBytes, len / kFixedRecordBytes, stg);
      c->unpack_ms += now_ms() - a;
      if (eof_here) stg[len] = stg[len + 1] = 0xFF;
      out = stg;
    } else if (eof_here) {
      std::memcpy(bufs.tail, p.base + off, (size_t)len);
      bufs.tail[len] = bufs.tail[len + 1] = 0xFF;
      out = bufs.tail;
    }
    emit(out, eof_here ? len + kFixedEofBytes : len);
    if (eof_here) c->eof_sent = true;
  }
  if (p.last && !c->eof_sent) {  // EOF did not fit (or no records): a buffer of its own
    if (!drop) bufs.tail[0] = bufs.tail[1] = 0xFF;
    emit(bufs.tail, kFixedEofBytes);
    c->eof_sent = true;
  }
}

}  // namespace gpu
}  // namespace uda
