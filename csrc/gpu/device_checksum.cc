#include "device_checksum.h"

#include <cstring>

#include "uda/error.h"
#include "uda/ifile.h"
#include "uda/trace.h"

namespace uda {
namespace gpu {

void DeviceChecksum::launch(std::vector<Item> items, hipStream_t s, bool states) {
  if (pending_) throw UdaError("DeviceChecksum: a launch is already pending");
  if (items.empty()) return;
  trace::Range tr("uda.ifile_checksum");
  items_ = std::move(items);
  const int n = (int)items_.size();
  // upload image: descs (16 B each) | chunk_first (8 B each, n + 1); then on the device only:
  // computed | stored (4 B each) | chunk states
  const size_t up = (size_t)n * sizeof(CrcDesc) + (size_t)(n + 1) * sizeof(int64_t);
  upload_.resize(up);
  auto* descs = reinterpret_cast<CrcDesc*>(upload_.data());
  auto* first = reinterpret_cast<int64_t*>(upload_.data() + (size_t)n * sizeof(CrcDesc));
  int64_t bytes = 0;
  for (int i = 0; i < n; ++i) {
    descs[i] = CrcDesc{items_[(size_t)i].body, items_[(size_t)i].len};
    bytes += items_[(size_t)i].len;
  }
  const int64_t chunks = crc32_chunk_plan(descs, n, first);
  const size_t res = (up + 15) & ~(size_t)15;
  const size_t ws = (res + (size_t)n * 8 + 15) & ~(size_t)15;
  const size_t total = ws + crc32_ws_bytes(chunks);
  if (scratch_.size() < total) scratch_.alloc_local(total + total / 2);
  uint8_t* d = scratch_.as<uint8_t>();
  t0_ = std::chrono::steady_clock::now();
  HIP_CHECK(hipMemcpyAsync(d, upload_.data(), up, hipMemcpyHostToDevice, s));
  auto* d_descs = reinterpret_cast<const CrcDesc*>(d);
  auto* d_first = reinterpret_cast<const int64_t*>(d + (size_t)n * sizeof(CrcDesc));
  auto* d_out = reinterpret_cast<uint32_t*>(d + res);
  if (states) launch_crc32_states(d_descs, n, d_first, chunks, d + ws, d_out, s);
  else launch_crc32(d_descs, n, d_first, chunks, d + ws, d_out, s);
  bool gather = false;
  for (const Item& it : items_) gather = gather || (!states && !it.stored_known);
  if (gather) launch_crc32_trailers(d_descs, n, d_out + n, s);
  HIP_CHECK(hipGetLastError());
  host_.assign((size_t)n * 2, 0);
  HIP_CHECK(hipMemcpyAsync(host_.data(), d_out, (size_t)n * (gather ? 8 : 4), hipMemcpyDeviceToHost, s));
  pending_ = true;
  states_ = states;
  if (states) return;
  partitions_ += n;
  bytes_ += bytes;
}

void DeviceChecksum::finish(hipStream_t s, bool synced, std::vector<uint32_t>* states) {
  if (!pending_) return;
  pending_ = false;
  if (!synced) HIP_CHECK(hipStreamSynchronize(s));
  ms_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count();
  const size_t n = items_.size();
  if (states_) {
    if (!states) throw UdaError("DeviceChecksum: a states launch is finished without a place for them");
    states->assign(host_.begin(), host_.begin() + (long)n);
    items_.clear();
    return;
  }
  for (size_t i = 0; i < n; ++i) {
    const Item& it = items_[i];
    const uint32_t stored = it.stored_known ? it.stored : host_[n + i];
    if (host_[i] != stored) throw UdaError(ifile_checksum_mismatch(it.map_id, stored, host_[i], it.len));
  }
  items_.clear();
}

}  // namespace gpu
}  // namespace uda
