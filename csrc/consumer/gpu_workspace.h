// What the GPU merge units (gpu_merge_staged.cc, gpu_merge_device.cc, gpu_prewarm.cc) share: the pooled
// device workspace of a merge, the early H2D stager, the per-device pools and admission gates, the
// device merge of host-resident runs and the piecewise D2H delivery of its output.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../gpu/block_decoder.h"
#include "../gpu/stream_decoder.h"
#include "../gpu/device_checksum.h"
#include "../gpu/device_ptr.h"
#include "../gpu/generic_merger.h"
#include "../gpu/generic_rounds.h"
#include "../gpu/hbm_ledger.h"
#include "../gpu/sdma.h"
#include "uda/codec.h"
#include "uda/combine.h"
#include "uda/compare.h"
#include "uda/error.h"
#include "uda/log.h"
#include "uda/trace.h"

namespace uda {

struct DeviceMergeOut {
  int64_t bytes = 0;           // merged records (no EOF), resident in the workspace's `out`
  std::vector<int64_t> cuts;   // whole-record boundaries, <= the requested spacing apart
  int64_t records = 0;
  int64_t records_in = 0;      // records merged (== records without a combiner)
  int64_t decoded_blocks = 0;
  int64_t decoded_streams = 0;  // zlib / gzip / zstd partitions decoded on the device (they have no blocks)
  // IFile checksum trailers (uda/ifile.h) found on the merge's runs and stripped; of those, verified
  int64_t trailers = 0, checksum_parts = 0, checksum_bytes = 0;
  double checksum_ms = 0;  // the device CRC, from launch to its result being read
  // ChecksumPolicy::slice_states: the raw CRC state (gpu::launch_crc32_states) of every input run, in order
  std::vector<uint32_t> slice_crc;
};

constexpr int64_t kPieceBytes = 64 << 20;  // D2H piece of the pinned double buffer (hipMemcpy fallback)
// stream_out's SDMA ring: a skewed task's delivery is the job's long pole (config #5: 60 GB in one task),
// and two 64 MiB pieces through hipMemcpyAsync left its consumer waiting on D2H for 815 of 2742 ms while
// 15 other tasks shared the link. Eight pieces of 16 MiB queued on the SDMA engines keep up to 128 MiB of
// the task's output moving ahead of its consumer, as the TeraSort delivery does (device_reduce.cc).
// (UDA_OUT_SLOTS / UDA_OUT_PIECE_MB: A/B of the ring's geometry)
extern const int kOutSlots;
extern const int64_t kOutPiece;

// Device buffers reused across the merges of one reduce task (LPQ groups, RPQ rounds): HBM is
// allocated once at the high-water mark instead of per merge (hipMalloc/hipFree of GBs costs ms and
// hipFree synchronizes the device).
struct DeviceWorkspace {
  int64_t pool_key = 0;  // input bytes of the task that last used it (DevicePool::acquire_fit)
  gpu::DeviceBuffer in, out, packed, out2;  // out2: second output of the generic key-range rounds
  gpu::DeviceBuffer fetched;  // device fetch: bytes of the partitions the providers declined as descriptors
  gpu::GenericMerger merger;
  gpu::DeviceBlockDecoder decoder;
  gpu::DeviceStreamDecoder inflater;  // zlib / gzip / zstd partitions: one stream each, no blocks
  gpu::PinnedBuffer ring;          // 2 x kPieceBytes, D2H staging of merged output
  gpu::GenericRoundsWs rounds;     // key-range round planner scratch (device fetch, generic keys)
  gpu::DeviceBuffer frame_scratch, frame_descs; // device framing walk of compressed partitions (device fetch)
  gpu::DeviceChecksum checksum;    // IFile checksum of the task's partitions (mapred.uda.ifile.checksum)
  hipEvent_t piece_ev[2] = {nullptr, nullptr};
  // SDMA delivery ring of stream_out: kOutSlots pieces of kOutPiece bytes on the GPU's NUMA node, each
  // with its completion signal
  gpu::SdmaEngine* oeng = nullptr;
  uint8_t* oring = nullptr;
  std::vector<hsa_signal_t> osig;
  bool sdma_out_ok = true;
  int out_ways = 1;  // SDMA engines each delivery piece is split over (the job's long pole: more)
  hsa_signal_t h2d_sig{};    // SDMA copies of this workspace: H2D of pinned spans (device_merge), LPQ spill D2H
  bool h2d_sdma_ok = true;
  double h2d_ms = 0, device_ms = 0, d2h_ms = 0, sink_ms = 0;
  ~DeviceWorkspace() {
    for (auto sg : osig) {
      try {
        gpu::SdmaEngine::wait(sg);  // a copy still in flight lands before the ring is reused
      } catch (...) {
      }
      oeng->destroy_signal(sg);
    }
    if (oring) oeng->release_ring(oring, (size_t)kOutSlots * kOutPiece);
    if (h2d_sig.handle) {
      try {
        gpu::SdmaEngine::wait(h2d_sig);
      } catch (...) {
      }
      (void)hsa_signal_destroy(h2d_sig);
    }
    for (auto e : piece_ev)
      if (e) (void)hipEventDestroy(e);
    if (cs) (void)hipStreamDestroy(cs);
  }
  void reset_stats() {
    h2d_ms = device_ms = d2h_ms = sink_ms = 0;
    out_ways = 1;
    checksum.reset();
  }
  // D2H stream of streamed deliveries (the merge stream is busy with the next round)
  hipStream_t copy_stream() {
    if (!cs) HIP_CHECK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    return cs;
  }
  hipStream_t cs = nullptr;
  static void ensure(gpu::DeviceBuffer& b, int64_t bytes) {
    bytes = std::max<int64_t>(bytes, 16);
    if ((int64_t)b.size() < bytes) b.alloc_local((size_t)(bytes + bytes / 8));
  }
  int64_t device_bytes() const {
    return (int64_t)(in.held() + out.held() + packed.held() + out2.held() + fetched.held() + frame_scratch.held() +
                     frame_descs.held()) +
           merger.workspace_bytes() + checksum.device_bytes() + inflater.scratch_bytes();
  }
};

// a task's stream from the device's pool (gpu::pooled_stream), handed back when the task is done
struct StreamGuard {
  hipStream_t s = nullptr;
  ~StreamGuard() { gpu::return_stream(s); }
};

// Merge host-resident runs on the device. `codec` != kNone: the runs are block-compressed streams
// decoded in HBM (falls back to a host decode when the framing needs it).
// Host spans of the runs to merge (pinned when they come from the arenas).
struct Span {
  const uint8_t* p;
  int64_t len;
  const uint8_t* dev = nullptr;  // device copy staged while the fetch went on (EarlyStager)
  // A fetched partition's IFile checksum (uda/ifile.h). Uncompressed: `tail` trailer bytes lie behind the
  // `len` body bytes, at p and at dev. Compressed: len counts the whole partition and the framing walk
  // finds the trailer; raw_len > 0 is what the body must decode to. id: index into ChecksumPolicy::map_ids.
  int tail = 0;
  int64_t raw_len = 0;
  int id = -1;
};

// device_merge verifies the trailers of its runs (verify) or only strips them; null: strips them
struct ChecksumPolicy {
  bool verify = true;
  const std::vector<std::string>* map_ids = nullptr;  // for the mismatch message
  // The runs are slices of partitions (an over-budget RPQ round over uncompressed, unstaged spans): nothing is
  // verified here; DeviceMergeOut::slice_crc gets every run's raw CRC state, computed where the slices were
  // just staged, for the caller to fold per partition over its rounds (uda::Crc32Running).
  bool slice_states = false;
};
// Host decode of one compressed partition whose framing the device cannot resolve. *tail = 4 when the
// blocks end four bytes ahead of the partition's end: those are its IFile checksum and are not decoded.
std::vector<uint8_t> host_decode_partition(Codec codec, const uint8_t* p, int64_t n, int* tail);

// Stages fetched partitions to HBM as soon as each one is complete in pinned memory, so the H2D
// copies overlap the remaining fetches (one issuing thread, one copy stream: the round-1 attempt
// issued from every drain thread and the copies contended). Device memory comes from a bump
// arena of 256 MiB blocks (a partition never straddles blocks); reset() recycles it once the
// group's merge has finished.
class EarlyStager {
 public:
  // SDMA (default, UDA_EARLY_H2D_SDMA=0 for hipMemcpyAsync): the copies run on a copy engine. A
  // hipMemcpyAsync H2D from pinned memory runs as a blit kernel whose host reads slowed the
  // concurrent fetch memcpys into the same arena about 8x when partitions were staged piecewise.
  explicit EarlyStager(int device) : device_(device) {
    s_ = gpu::pooled_stream();
    const char* e = std::getenv("UDA_EARLY_H2D_SDMA");
    if (!e || std::atoi(e) != 0) {
      try {
        sdma_ = &gpu::SdmaEngine::for_device(device);
        sig_ = sdma_->make_signal();
        gpu::SdmaEngine::arm(sig_, 0);
        for (auto& g : gsig_) {
          g = sdma_->make_signal();
          gpu::SdmaEngine::arm(g, 0);
        }
      } catch (const std::exception& ex) {
        UDA_LOG(kWarn, "early staging: no SDMA engine (%s); using hipMemcpyAsync", ex.what());
        sdma_ = nullptr;
      }
    }
    thr_ = std::thread([this] { loop(); });
  }
  ~EarlyStager() {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    thr_.join();
    (void)hipStreamSynchronize(s_);
    gpu::return_stream(s_);
    if (sdma_) {
      std::vector<hsa_signal_t> all{sig_};
      all.insert(all.end(), gsig_, gsig_ + kGroups);
      for (hsa_signal_t g : all) {
        try {
          gpu::SdmaEngine::wait(g);
        } catch (...) {
        }
        sdma_->destroy_signal(g);
      }
    }
  }
  const char* engine() const { return sdma_ ? "sdma" : "hip"; }
  // Device address the partition will be copied to; the copy is issued asynchronously.
  const uint8_t* submit(const uint8_t* host, int64_t len) {
    uint8_t* d = reserve(len);
    copy(host, d, len);
    return d;
  }
  // A partition's device span, filled piecewise by copy() as its bytes land in pinned memory.
  uint8_t* reserve(int64_t len) {
    std::lock_guard<std::mutex> g(mu_);
    return alloc(len);
  }
  // group >= 0 (SDMA only): the copy also counts toward flush_group(group), so a caller can wait for
  // one batch of copies (a progressive merge's phase) while later batches are still being queued.
  void copy(const uint8_t* host, uint8_t* dev, int64_t len, int group = -1) {
    if (len <= 0) return;
    std::lock_guard<std::mutex> g(mu_);
    if (group >= kGroups || (group >= 0 && !sdma_)) throw UdaError("early staging: bad copy group");
    if (group >= 0) ++gqueued_[group];
    q_.push_back(Job{host, dev, len, trace::host_enabled() ? trace::now_ns() : 0, group});
    cv_.notify_all();
  }
  static constexpr int kGroups = 16;
  bool sdma() const { return sdma_ != nullptr; }
  // Every copy of `group` queued so far has completed.
  void flush_group(int group) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return gqueued_[group] == 0 || !error_.empty(); });
    if (!error_.empty()) throw UdaError("early H2D staging failed: " + error_);
    lk.unlock();
    try {
      gpu::SdmaEngine::wait(gsig_[group]);
    } catch (const std::exception& ex) {
      gpu::SdmaEngine::arm(gsig_[group], 0);
      throw UdaError(std::string("early H2D staging failed: ") + ex.what());
    }
  }
  // Every submitted copy has completed.
  void flush() {
    const int64_t tf = trace::host_enabled() ? trace::now_ns() : 0;
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return q_.empty() && busy_ == 0; });
    lk.unlock();
    HIP_CHECK(hipStreamSynchronize(s_));
    if (sdma_) {
      for (int g = -1; g < kGroups; ++g) {
        hsa_signal_t sg = g < 0 ? sig_ : gsig_[g];
        try {
          gpu::SdmaEngine::wait(sg);
        } catch (const std::exception& ex) {
          gpu::SdmaEngine::arm(sg, 0);
          throw UdaError(std::string("early H2D staging failed: ") + ex.what());
        }
      }
    }
    if (!error_.empty()) throw UdaError("early H2D staging failed: " + error_);
    if (tf) trace::host_event("stage_flush", bytes_, copies_, tf, trace::now_ns());
  }
  void reset() {
    flush();
    std::lock_guard<std::mutex> g(mu_);
    for (auto& b : blocks_) b.used = 0;
    cur_ = 0;
    issue_ms_ = 0;
    copies_ = 0;
    bytes_ = 0;
  }
  // reset() and give the device blocks back (a task switching to direct RPQ rounds: its staged copies
  // are not used, and the rounds' workspaces need that HBM within the budget)
  void release_blocks() {
    reset();
    std::lock_guard<std::mutex> g(mu_);
    blocks_.clear();
  }
  double issue_ms() const { return issue_ms_; }
  int64_t copies() const { return copies_; }
  int64_t bytes() const { return bytes_; }
  int64_t device_bytes() {
    std::lock_guard<std::mutex> g(mu_);
    int64_t n = 0;
    for (const auto& b : blocks_) n += (int64_t)b.buf.held();
    return n;
  }

 private:
  struct Job {
    const uint8_t* host;
    uint8_t* dev;
    int64_t len;
    int64_t t_enq;  // trace: when the copy was queued
    int group;
  };
  struct Block {
    gpu::DeviceBuffer buf;
    int64_t used = 0;
  };
  uint8_t* alloc(int64_t len) {  // mu_ held
    len = (std::max<int64_t>(len, 1) + 255) & ~(int64_t)255;
    for (; cur_ < blocks_.size(); ++cur_)
      if ((int64_t)blocks_[cur_].buf.size() - blocks_[cur_].used >= len) break;
    if (cur_ == blocks_.size()) {
      blocks_.emplace_back();
      HIP_CHECK(hipSetDevice(device_));
      blocks_.back().buf.alloc((size_t)std::max<int64_t>(len, 256ll << 20));
    }
    Block& b = blocks_[cur_];
    uint8_t* p = b.buf.as<uint8_t>() + b.used;
    b.used += len;
    return p;
  }
  void loop() {
    (void)hipSetDevice(device_);
    for (;;) {
      Job j;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
        if (q_.empty()) return;
        j = q_.front();
        q_.pop_front();
        ++busy_;
      }
      const auto t0 = std::chrono::steady_clock::now();
      std::string err;
      if (sdma_) {
        hsa_signal_t sg = j.group >= 0 ? gsig_[j.group] : sig_;
        gpu::SdmaEngine::add(sg, 1);
        try {
          sdma_->copy_h2d(j.dev, j.host, (size_t)j.len, sg);
        } catch (const std::exception& ex) {
          gpu::SdmaEngine::add(sg, -1);
          err = ex.what();
        }
      } else {
        const hipError_t e = hipMemcpyAsync(j.dev, j.host, (size_t)j.len, hipMemcpyHostToDevice, s_);
        if (e != hipSuccess) err = hipGetErrorString(e);
      }
      issue_ms_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (j.t_enq) {
        trace::host_event("stage_wait", j.len, (int64_t)(uintptr_t)j.host, j.t_enq, trace::now_ns());
      }
      std::lock_guard<std::mutex> g(mu_);
      if (!err.empty() && error_.empty()) error_ = err;
      bytes_ += j.len;
      ++copies_;
      --busy_;
      if (j.group >= 0) --gqueued_[j.group];  // issued (its signal tracks completion)
      cv_.notify_all();
    }
  }
  int device_;
  hipStream_t s_ = nullptr;
  gpu::SdmaEngine* sdma_ = nullptr;
  hsa_signal_t sig_{};  // outstanding SDMA copies
  hsa_signal_t gsig_[kGroups]{};  // outstanding copies per group
  int64_t gqueued_[kGroups]{};    // queued, not yet issued, per group
  std::thread thr_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<Job> q_;
  int busy_ = 0;
  bool stop_ = false;
  std::string error_;
  std::vector<Block> blocks_;
  size_t cur_ = 0;
  double issue_ms_ = 0;
  int64_t copies_ = 0;
  int64_t bytes_ = 0;
};

// Process-wide cache of the per-device objects a GPU reduce task builds (HBM workspaces, the
// pinned D2H ring, the early-staging arena and its copy thread): one reducer process runs many
// reduce tasks in sequence, and building these costs tens of ms per task (pinning a 128 MiB ring,
// hipMalloc of GBs, hipFree synchronizing the device). An object goes back to the cache only
// after a task that used it ended cleanly.
template <class T>
class DevicePool {
 public:
  static DevicePool& get();  // one per process and T (gpu_workspace.cc)
  template <class Make>
  std::unique_ptr<T> acquire(int device, Make&& make) {
    {
      std::lock_guard<std::mutex> g(mu_);
      auto& v = idle_[device];
      if (!v.empty()) {
        std::unique_ptr<T> o = std::move(v.back());
        v.pop_back();
        return o;
      }
    }
    return make();
  }
  // The idle object last used by the task most like this one: the closest pool_key (the input bytes of
  // the task that used it; ties to the larger object), then tagged with `key`. The jobs of a wave repeat
  // their shapes, so a skewed task gets back the workspace it grew before. Handing it a small one makes
  // it grow again (and hipFree the old buffers, which synchronizes the device under every other task),
  // and what its size promises is no guide: tasks of any input size beyond one round size their
  // workspaces to the round (config #5, 100 GB: 16.6 GB/s last-in, 20-30 by size, see BENCHMARKS.md).
  template <class Make>
  std::unique_ptr<T> acquire_fit(int device, int64_t key, Make&& make) {
    {
      std::lock_guard<std::mutex> g(mu_);
      auto& v = idle_[device];
      if (!v.empty()) {
        size_t best = 0;
        for (size_t i = 1; i < v.size(); ++i) {
          const int64_t b = v[best]->pool_key, c = v[i]->pool_key;
          const int64_t db = b > key ? b - key : key - b, dc = c > key ? c - key : key - c;
          if (dc < db || (dc == db && v[i]->device_bytes() > v[best]->device_bytes())) best = i;
        }
        std::unique_ptr<T> o = std::move(v[best]);
        v.erase(v.begin() + (long)best);
        o->pool_key = key;
        return o;
      }
    }
    std::unique_ptr<T> o = make();
    o->pool_key = key;
    return o;
  }
  void release(int device, std::unique_ptr<T> o) {
    std::lock_guard<std::mutex> g(mu_);
    auto& v = idle_[device];
    if (v.size() < kMaxIdle) v.push_back(std::move(o));
  }
  int64_t trim(int device, int64_t want) {
    std::vector<std::unique_ptr<T>> drop;
    int64_t got = 0;
    {
      std::lock_guard<std::mutex> g(mu_);
      auto& v = idle_[device];
      std::sort(v.begin(), v.end(), [](const auto& a, const auto& b) { return a->device_bytes() < b->device_bytes(); });
      while (!v.empty() && got < want) {
        got += v.back()->device_bytes();
        drop.push_back(std::move(v.back()));
        v.pop_back();
      }
    }
    if (!drop.empty()) {
      int cur = 0;
      HIP_CHECK(hipGetDevice(&cur));
      HIP_CHECK(hipSetDevice(device));
      drop.clear();
      HIP_CHECK(hipSetDevice(cur));
    }
    return got;
  }
  int64_t idle(int device) {
    std::lock_guard<std::mutex> g(mu_);
    int64_t n = 0;
    for (auto& o : idle_[device]) n += o->device_bytes();
    return n;
  }

 private:
  // Idle objects are bounded in bytes by the device's HBM budget (trimmed under pressure); the count
  // bound only limits the host memory they pin (a workspace's D2H ring is 128 MiB of pinned DRAM).
  // 16 concurrent reduce tasks per GPU (the bench shape) must find their workspaces again: a dropped
  // one is freed, and hipFree synchronizes the whole device under the other tasks.
  static constexpr size_t kMaxIdle = 32;
  std::mutex mu_;
  std::map<int, std::vector<std::unique_ptr<T>>> idle_;
};

template <class T>
struct PoolLease {
  int device;
  std::unique_ptr<T> obj;
  bool clean = false;  // set when the task ended without an error
  ~PoolLease() {
    if (obj && clean) DevicePool<T>::get().release(device, std::move(obj));
  }
};

// a pooled object of `device`: an idle one, or built now
inline std::unique_ptr<DeviceWorkspace> pooled_workspace(int device) {
  return DevicePool<DeviceWorkspace>::get().acquire(device, [] { return std::make_unique<DeviceWorkspace>(); });
}
inline std::unique_ptr<EarlyStager> pooled_stager(int device) {
  return DevicePool<EarlyStager>::get().acquire(device, [device] { return std::make_unique<EarlyStager>(device); });
}

// Admission of staged GPU reduce tasks per device (mapred.uda.gpu.max.concurrent.merges, default 0 =
// no limit).
// Reduce tasks started together run their phases in lockstep: all fetch and copy to HBM at once (the
// H2D direction of PCIe busy, D2H idle), then all merge, then all deliver (D2H busy, H2D idle). With
// at most `cap` tasks admitted, in arrival order, a task's fetch and H2D overlap the merge and D2H of
// the tasks ahead of it, so both PCIe directions stay busy. Tasks wait in FIFO order of arrival.
class DeviceGate {
 public:
  // gate 0: staged GPU merges (mapred.uda.gpu.max.concurrent.merges); gate 1: device block decodes
  // of compressed descriptor tasks (mapred.uda.gpu.decode.slots)
  // gate 2: declined-partition byte fetches of device-fetch tasks (mapred.uda.gpu.fetch.bytes.slots)
  static DeviceGate& get(int which = 0);
  // false if `stopped` became true while waiting
  template <class Stop>
  bool acquire(int device, int cap, Stop&& stopped) {
    std::unique_lock<std::mutex> lk(mu_);
    Dev& d = devs_[device];
    const uint64_t me = d.next_ticket++;
    d.waiting.push_back(me);
    for (;;) {
      if (d.used < cap && d.waiting.front() == me) {
        d.waiting.pop_front();
        ++d.used;
        cv_.notify_all();
        return true;
      }
      if (stopped()) {
        d.waiting.erase(std::find(d.waiting.begin(), d.waiting.end(), me));
        cv_.notify_all();
        return false;
      }
      cv_.wait_for(lk, std::chrono::milliseconds(20));
    }
  }
  void release(int device) {
    std::lock_guard<std::mutex> g(mu_);
    --devs_[device].used;
    cv_.notify_all();
  }
  // host function enqueued behind a gated copy: frees the slot the moment the copy has landed (not when
  // the task comes back for it after consuming the previous piece)
  static void release_cb(void* device) { get().release((int)(intptr_t)device); }

 private:
  struct Dev {
    int used = 0;
    uint64_t next_ticket = 0;
    std::deque<uint64_t> waiting;
  };
  std::mutex mu_;
  std::condition_variable cv_;
  std::map<int, Dev> devs_;
};

// Staged GPU merges running per device (the progressive-phase default asks whether a task is alone).
std::atomic<int>& staged_merges(int device);
struct StagedCount {
  int device;
  explicit StagedCount(int d) : device(d) { staged_merges(device).fetch_add(1); }
  ~StagedCount() { staged_merges(device).fetch_sub(1); }
};

struct GateLease {
  int device = -1;
  int which = 0;
  ~GateLease() {
    if (device >= 0) DeviceGate::get(which).release(device);
  }
};

// on_round: deliver the merged output in key-range rounds while the device merges the next one
// (GenericMerger::merge); time spent in it is not counted as device time.
// pinned_src: the host spans are pinned (spill arenas): their H2D goes to an SDMA engine (not the
// delivery engine) instead of a blit kernel whose host reads would slow the merge kernels beside it.
DeviceMergeOut device_merge(DeviceWorkspace& ws, const std::vector<Span>& in_runs, Codec codec, KeyKind kind,
                            int64_t spacing, hipStream_t s, const gpu::GenericMerger::RoundFn& on_round = nullptr,
                            bool pinned_src = false, CombineOp combine = CombineOp::kNone,
                            int64_t round_bytes = 256ll << 20,  // on_round's rounds (mapred.uda.gpu.merge.round.bytes)
                            const ChecksumPolicy* ck = nullptr);

// piece boundaries (in cut indices) of a merged output: pieces of up to `limit` bytes ending on record
// boundaries; empty if a single cut interval is larger than `limit`
std::vector<size_t> piece_bounds(const std::vector<int64_t>& cuts, int64_t limit);

// Stream the merged output of `m` (in ws.out, complete on the device) to the host in pieces that end on
// record boundaries (the cuts): up to kOutSlots pieces of kOutPiece bytes queued on the GPU's SDMA
// engines ahead of the consumer, fn(piece k) running while pieces k+1.. land. fn(ptr, first_cut,
// last_cut) gets the bytes of cuts [first_cut, last_cut] (ptr = byte cuts[first_cut]). A record larger
// than a piece, or no SDMA engine: two 64 MiB pieces through hipMemcpyAsync on `s`.
template <typename Fn>
void stream_out(DeviceWorkspace& ws, const DeviceMergeOut& m, hipStream_t s, Fn&& fn, const uint8_t* src = nullptr) {
  const size_t nb = m.cuts.size() < 2 ? 0 : m.cuts.size() - 1;
  if (nb == 0) return;
  const uint8_t* out = src ? src : ws.out.as<uint8_t>();
  if (ws.sdma_out_ok && !ws.oring) {
    try {
      int dev = 0;
      HIP_CHECK(hipGetDevice(&dev));
      ws.oeng = &gpu::SdmaEngine::for_device(dev);
      ws.oring = static_cast<uint8_t*>(ws.oeng->acquire_ring((size_t)kOutSlots * kOutPiece));
      for (int i = 0; i < kOutSlots; ++i) ws.osig.push_back(ws.oeng->make_signal());
    } catch (const std::exception& e) {
      UDA_LOG(kInfo, "stream_out: no SDMA delivery ring (%s): hipMemcpyAsync pieces", e.what());
      ws.sdma_out_ok = false;
    }
  }
  if (ws.oring) {
    const std::vector<size_t> pb = piece_bounds(m.cuts, kOutPiece);
    if (!pb.empty()) {
      const size_t np = pb.size() - 1;
      gpu::SdmaEngine& eng = *ws.oeng;
      auto issue = [&](size_t k) {
        const int64_t b = m.cuts[pb[k]], len = m.cuts[pb[k + 1]] - b;
        hsa_signal_t sg = ws.osig[k % kOutSlots];
        gpu::SdmaEngine::arm(sg, eng.parts((size_t)len, ws.out_ways));
        eng.copy_d2h(ws.oring + (k % kOutSlots) * kOutPiece, out + b, (size_t)len, sg, ws.out_ways);
      };
      size_t issued = 0, k = 0;
      // a consumer that throws (a stopped task) leaves copies in flight into the ring: they land before
      // the ring and its signals serve the next output
      struct Drain {
        DeviceWorkspace& ws;
        size_t& issued;
        size_t& k;
        ~Drain() {
          for (size_t j = k; j < issued; ++j) {
            try {
              gpu::SdmaEngine::wait(ws.osig[j % kOutSlots]);
            } catch (...) {
            }
          }
        }
      } drain{ws, issued, k};
      for (; issued < std::min<size_t>(np, kOutSlots); ++issued) issue(issued);
      for (; k < np; ++k) {
        auto t0 = std::chrono::steady_clock::now();
        gpu::SdmaEngine::wait(ws.osig[k % kOutSlots]);
        auto t1 = std::chrono::steady_clock::now();
        ws.d2h_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
        const int64_t tp = trace::host_enabled() ? trace::now_ns() : 0;
        if (tp) trace::host_event("so_wait", (int64_t)(uintptr_t)&ws, 0, tp - (int64_t)(t1 - t0).count(), tp);
        fn(ws.oring + (k % kOutSlots) * kOutPiece, pb[k], pb[k + 1]);
        ws.sink_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
        if (tp) trace::host_event("so_sink", (int64_t)(uintptr_t)&ws, m.cuts[pb[k + 1]] - m.cuts[pb[k]], tp,
                                  trace::now_ns());
        if (k + kOutSlots < np) issue(issued++);  // its slot was just consumed
      }
      return;
    }
  }
  if (ws.ring.size() < (size_t)(2 * kPieceBytes)) {  // on the GPU's NUMA node, like the consumer copying out of it
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    ws.ring.alloc_on_node((size_t)(2 * kPieceBytes), gpu::device_numa_node(dev));
  }
  for (auto& e : ws.piece_ev)
    if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  // piece boundaries in cut indices
  std::vector<size_t> pb{0};
  while (pb.back() < nb) {
    size_t j = pb.back();
    const int64_t start = m.cuts[j];
    size_t k = j + 1;
    while (k < nb && m.cuts[k + 1] - start <= kPieceBytes) ++k;
    pb.push_back(k);
  }
  auto enqueue = [&](size_t piece) {
    const int slot = (int)(piece & 1);
    const int64_t b = m.cuts[pb[piece]], e = m.cuts[pb[piece + 1]];
    if (e - b > kPieceBytes) throw UdaError("record larger than the D2H piece");
    HIP_CHECK(hipMemcpyAsync(ws.ring.as<uint8_t>() + slot * kPieceBytes, out + b, (size_t)(e - b),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipEventRecord(ws.piece_ev[slot], s));
  };
  const size_t np = pb.size() - 1;
  enqueue(0);
  for (size_t piece = 0; piece < np; ++piece) {
    const int slot = (int)(piece & 1);
    auto t0 = std::chrono::steady_clock::now();
    HIP_CHECK(hipEventSynchronize(ws.piece_ev[slot]));
    auto t1 = std::chrono::steady_clock::now();
    ws.d2h_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
    const int64_t tp = trace::host_enabled() ? trace::now_ns() : 0;
    if (tp) trace::host_event("so_wait", (int64_t)(uintptr_t)&ws, 0, tp - (int64_t)(t1 - t0).count(), tp);
    if (piece + 1 < np) enqueue(piece + 1);
    fn(ws.ring.as<uint8_t>() + slot * kPieceBytes, pb[piece], pb[piece + 1]);
    ws.sink_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    if (tp) trace::host_event("so_sink", (int64_t)(uintptr_t)&ws, m.cuts[pb[piece + 1]] - m.cuts[pb[piece]], tp,
                              trace::now_ns());
  }
}

}  // namespace uda
