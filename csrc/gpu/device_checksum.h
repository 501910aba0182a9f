// IFile checksum verification of device-resident partitions (uda/ifile.h): one batched launch of the
// CRC32 kernels (crc32.hip) over the partitions of a reduce task that carry a trailer, and the
// comparison with the stored values once the task's stream has been synchronized.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <string>
#include <vector>

#include "device_engine.h"
#include "kernels.h"

namespace uda {
namespace gpu {

class DeviceChecksum {
 public:
  struct Item {
    const uint8_t* body = nullptr;  // device address of the partition's bytes as fetched (compressed or not)
    int64_t len = 0;                // without the trailer
    std::string map_id;
    bool stored_known = false;      // false: the four trailer bytes lie at body + len on the device
    uint32_t stored = 0;
  };
  // Queues everything on s (descriptor upload, the kernels, the results' download) and returns; nothing
  // is allocated per call once the scratch has grown to the task's shape. One launch may be pending.
  // states: the items are consecutive slices of partitions, not partitions (an over-budget RPQ round): the
  // state kernel runs (launch_crc32_states; body and len alone are read, empty items are fine) and finish()
  // hands the raw states back for the host to fold (uda::crc32_fold_state). Such a launch counts toward ms()
  // only: which partitions it completes is the caller's to know.
  void launch(std::vector<Item> items, hipStream_t s, bool states = false);
  bool pending() const { return pending_; }
  // After s has been synchronized (synced: by the caller, since launch(); else here): throws UdaError
  // with ifile_checksum_mismatch() of the first partition whose CRC differs from its stored value. After a
  // states launch nothing is compared: *states gets one raw state per item, in the items' order.
  void finish(hipStream_t s, bool synced, std::vector<uint32_t>* states = nullptr);
  // totals over the launches since reset()
  int64_t partitions() const { return partitions_; }
  int64_t bytes() const { return bytes_; }
  double ms() const { return ms_; }  // wall time from a launch to its results being read
  void reset() {
    partitions_ = bytes_ = 0;
    ms_ = 0;
    pending_ = false;
  }
  int64_t device_bytes() const { return (int64_t)scratch_.held(); }

 private:
  DeviceBuffer scratch_;
  std::vector<Item> items_;
  std::vector<uint8_t> upload_;  // descriptors | chunk_first, kept until the launch has finished
  std::vector<uint32_t> host_;   // computed | stored
  bool pending_ = false, states_ = false;
  std::chrono::steady_clock::time_point t0_;
  int64_t partitions_ = 0, bytes_ = 0;
  double ms_ = 0;
};

}  // namespace gpu
}  // namespace uda
