// Device and pinned-host allocators, the stream pool and the small device queries of the device engine.
// See device_engine.h.
#include "device_engine.h"
#include "device_ptr.h"
#include "hbm_ledger.h"
#include "sdma.h"
#include "uda/fault.h"
#include "uda/log.h"
#include "uda/thread_name.h"
#include "uda/trace.h"

#include <rccl/rccl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <stdexcept>

namespace uda {
namespace gpu {

void hip_check(hipError_t e, const char* what, const char* file, int line) {
  if (e != hipSuccess)
    throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e) + " in " + what +
                             " at " + file + ":" + std::to_string(line));
}

// ------------------------------------------------------------------------------------ buffers
DeviceBuffer::~DeviceBuffer() { reset(); }
namespace {
// UDA_DEVICE_GUARD=1 (debug): every device buffer gets a tail of kGuardByte past its size (local
// buffers: 64 KiB more; exportable ones: their IPC padding), checked when the buffer is freed. A kernel
// writing past the end of its buffer then shows as a logged violation instead of silently changing the
// next allocation's bytes.
constexpr size_t kGuardBytes = 64 << 10;
constexpr int kGuardByte = 0xA5;
std::atomic<int64_t> g_guard_violations{0};
bool guard_enabled() {
  const char* e = std::getenv("UDA_DEVICE_GUARD");
  return e && std::atoi(e) != 0;
}
}  // namespace

int64_t device_guard_violations() { return g_guard_violations.load(); }

void DeviceBuffer::alloc_impl(size_t bytes, bool resident, bool exportable) {
  reset();
  if (bytes == 0) return;
  if (fault_hit("DEVICE_ALLOC")) throw std::runtime_error("injected device allocation failure");
  // Blocks another process may map over hipIpc (our descriptor fetch, RCCL's peer registration of
  // send/receive buffers) must stay out of the size range that hangs the importer (device_ptr.h).
  const bool guard = guard_enabled();
  const size_t held = exportable ? ipc_safe_bytes(bytes + (guard ? 1 : 0)) : bytes + (guard ? kGuardBytes : 0);
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  HbmLedger::get().on_alloc(dev, (int64_t)held, resident);
  const int64_t tt = trace::host_enabled() ? trace::now_ns() : 0;
  const hipError_t e = hipMalloc(&ptr_, held);
  if (e != hipSuccess) {
    ptr_ = nullptr;
    HbmLedger::get().on_free(dev, (int64_t)held, resident);
    (void)hipGetLastError();
    const HbmLedger::Stats ls = HbmLedger::get().stats(dev);
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e) + " allocating " +
                             std::to_string(held) + " bytes on device " + std::to_string(dev) + " (" +
                             std::to_string(free_b) + " free of " + std::to_string(total_b) +
                             "; this process: used " + std::to_string(ls.used) + ", reserved " +
                             std::to_string(ls.reserved) + ", node " + std::to_string(ls.node_bytes) +
                             ", budget " + std::to_string(ls.budget) + (HbmLedger::get().bound() ? ", in a reservation" : "") +
                             ")");
  }
  if (tt) trace::host_event("device_alloc", (int64_t)bytes, 0, tt, trace::now_ns());
  size_ = bytes;
  held_ = held;
  dev_ = dev;
  resident_ = resident;
  guarded_ = guard && held > bytes;
  if (guarded_) {  // complete before any non-blocking stream writes near it
    HIP_CHECK(hipMemsetAsync(static_cast<uint8_t*>(ptr_) + bytes, kGuardByte, std::min(held - bytes, kGuardBytes), nullptr));
    HIP_CHECK(hipStreamSynchronize(nullptr));
  }
}
void DeviceBuffer::reset() {
  if (ptr_ && guarded_) {
    const size_t n = std::min(held_ - size_, kGuardBytes);
    std::vector<uint8_t> tail(n);
    if (hipMemcpy(tail.data(), static_cast<uint8_t*>(ptr_) + size_, n, hipMemcpyDeviceToHost) == hipSuccess) {
      size_t bad = 0, first = n;
      for (size_t i = 0; i < n; ++i)
        if (tail[i] != (uint8_t)kGuardByte) {
          ++bad;
          first = std::min(first, i);
        }
      if (bad) {
        g_guard_violations.fetch_add(1);
        UDA_LOG(kError, "device buffer of %zu bytes: %zu guard bytes overwritten, the first %zu past its end", size_,
                bad, first);
      }
    }
    guarded_ = false;
  }
  if (ptr_) note_device_free(ptr_);  // an exporter's cached IPC identity of this address is stale now
  if (ptr_ && trace::host_enabled()) {
    const int64_t tt = trace::now_ns();
    (void)hipFree(ptr_);
    trace::host_event("device_free", (int64_t)size_, 0, tt, trace::now_ns());
    ptr_ = nullptr;
  }
  if (ptr_) (void)hipFree(ptr_);
  if (held_) HbmLedger::get().on_free(dev_, (int64_t)held_, resident_);
  ptr_ = nullptr;
  size_ = held_ = 0;
}

PinnedBuffer::~PinnedBuffer() { pinned_host_free(ptr_); }
PinnedPool& PinnedPool::instance() {
  static PinnedPool* pool = new PinnedPool();  // leaked on purpose: outlives every user at exit
  return *pool;
}

PinnedPool::Block PinnedPool::acquire(size_t min_bytes) {
  {
    std::lock_guard<std::mutex> g(mu_);
    auto it = free_.lower_bound(min_bytes);
    if (it != free_.end() && it->first <= 2 * min_bytes + PinnedArena::kBlock) {
      Block b{it->second, it->first};
      cached_ -= it->first;
      free_.erase(it);
      return b;
    }
  }
  Block b;
  // 2 MiB granules; blocks above 64 MiB in 32 MiB granules, so the next task's slightly different
  // sizes (LPQ spills, partitions) find the cached block instead of pinning a new one (tens of ms)
  const size_t gran = min_bytes > ((size_t)64 << 20) ? ((size_t)32 << 20) : ((size_t)2 << 20);
  b.size = (min_bytes + gran - 1) & ~(gran - 1);
  void* p = nullptr;
  const int64_t tt = trace::host_enabled() ? trace::now_ns() : 0;
  try {
    p = pinned_host_alloc(b.size);
  } catch (const std::exception&) {
    // memory the reaper still holds, then the cache: trim and retry once
    drain_reaper();
    std::multimap<size_t, uint8_t*> drop;
    {
      std::lock_guard<std::mutex> g(mu_);
      drop.swap(free_);
      cached_ = 0;
    }
    for (auto& kv : drop) pinned_host_free(kv.second);
    try {
      p = pinned_host_alloc(b.size);
    } catch (const std::exception&) {
      throw std::runtime_error("pinned host allocation of " + std::to_string(b.size) + " bytes failed");
    }
  }
  if (tt) trace::host_event("pinned_alloc", (int64_t)b.size, (int64_t)min_bytes, tt, trace::now_ns());
  b.p = static_cast<uint8_t*>(p);
  return b;
}

void PinnedPool::release(Block b) {
  if (!b.p) return;
  std::lock_guard<std::mutex> g(mu_);
  if (cached_ + b.size > cap_) {
    // unpinning and unmapping GBs takes hundreds of ms (a 41.6 GB over-budget task spent 486 ms closing
    // on it): a reaper thread does it off the task's path
    reap_.push_back(b);
    if (!reaper_started_) {
      reaper_started_ = true;
      std::thread([this] { name_thread("uda-pin-reaper"); reaper_main(); }).detach();  // the pool is never destroyed
    }
    reap_cv_.notify_one();
    return;
  }
  free_.emplace(b.size, b.p);
  cached_ += b.size;
}

void PinnedPool::reaper_main() {
  for (;;) {
    Block b;
    {
      std::unique_lock<std::mutex> lk(mu_);
      reap_cv_.wait(lk, [&] { return !reap_.empty(); });
      b = reap_.front();
      reap_.pop_front();
      ++reaping_;
    }
    pinned_host_free(b.p);
    std::lock_guard<std::mutex> g(mu_);
    --reaping_;
    reap_cv_.notify_all();
  }
}

void PinnedPool::drain_reaper() {
  for (;;) {
    Block b;
    {
      std::unique_lock<std::mutex> lk(mu_);
      if (reap_.empty()) {
        reap_cv_.wait(lk, [&] { return reaping_ == 0 || !reap_.empty(); });
        if (reap_.empty()) return;
      }
      b = reap_.front();
      reap_.pop_front();
    }
    pinned_host_free(b.p);
  }
}

void PinnedPool::set_cache_cap(size_t bytes) {
  std::lock_guard<std::mutex> g(mu_);
  cap_ = bytes;
}

namespace {
size_t host_memory_limit() {
  size_t lim = (size_t)sysconf(_SC_PHYS_PAGES) * (size_t)sysconf(_SC_PAGESIZE);
  if (FILE* f = std::fopen("/sys/fs/cgroup/memory.max", "r")) {  // cgroup v2 ("max" = none)
    unsigned long long v = 0;
    if (std::fscanf(f, "%llu", &v) == 1 && v > 0) lim = std::min<size_t>(lim, (size_t)v);
    std::fclose(f);
  }
  return lim;
}
}  // namespace

void PinnedPool::raise_cache_cap(size_t bytes) {
  static const size_t ceiling = host_memory_limit() / 4;
  std::lock_guard<std::mutex> g(mu_);
  cap_ = std::max(cap_, std::min(bytes, ceiling));
}

size_t PinnedPool::cached_bytes() {
  std::lock_guard<std::mutex> g(mu_);
  return cached_;
}

uint8_t* PinnedArena::alloc(size_t bytes) {
  bytes = (bytes + 255) & ~(size_t)255;
  bytes_ += bytes;
  if (bytes > kBlock / 4) {  // large request: a dedicated block, kept behind the shared one
    PinnedPool::Block b = PinnedPool::instance().acquire(std::max<size_t>(bytes, 256));
    if (last_shared_ && !blocks_.empty()) {
      blocks_.insert(blocks_.end() - 1, b);
    } else {
      blocks_.push_back(b);
      last_shared_ = false;
    }
    return b.p;
  }
  if (!last_shared_ || used_ + bytes > blocks_.back().size) {
    blocks_.push_back(PinnedPool::instance().acquire(kBlock));
    used_ = 0;
    last_shared_ = true;
  }
  uint8_t* p = blocks_.back().p + used_;
  used_ += bytes;
  return p;
}

void PinnedArena::release_all() {
  for (auto& b : blocks_) PinnedPool::instance().release(b);
  blocks_.clear();
  used_ = 0;
  last_shared_ = false;
  bytes_ = 0;
}

void PinnedBuffer::alloc(size_t bytes) {
  pinned_host_free(ptr_);
  ptr_ = nullptr;
  size_ = 0;
  if (bytes == 0) return;
  const int64_t tt = trace::host_enabled() ? trace::now_ns() : 0;
  ptr_ = pinned_host_alloc(bytes);
  if (tt) trace::host_event("pinned_buf_alloc", (int64_t)bytes, -1, tt, trace::now_ns());
  size_ = bytes;
}

void PinnedBuffer::alloc_on_node(size_t bytes, int node) {
  pinned_host_free(ptr_);
  ptr_ = nullptr;
  size_ = 0;
  if (bytes == 0) return;
  const int64_t tt = trace::host_enabled() ? trace::now_ns() : 0;
  ptr_ = pinned_host_alloc(bytes, node);  // preferred-node pages, registered (sdma.h)
  if (tt) trace::host_event("pinned_buf_alloc", (int64_t)bytes, node, tt, trace::now_ns());
  size_ = bytes;
}

std::string nccl_unique_id() {
  ncclUniqueId id;
  ncclResult_t r = ncclGetUniqueId(&id);
  if (r != ncclSuccess) throw std::runtime_error(std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
  return std::string(reinterpret_cast<const char*>(&id), sizeof(id));
}

int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

namespace {
struct StreamPool {
  std::mutex mu;
  std::map<std::pair<int, int>, std::vector<hipStream_t>> idle;  // (device, priority) -> streams
  std::map<hipStream_t, std::pair<int, int>> owner;               // every pooled stream's key
  static StreamPool& get() {
    static StreamPool* p = new StreamPool;  // never destroyed: streams outlive static teardown order
    return *p;
  }
};
}  // namespace

hipStream_t pooled_stream(int priority) {
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  StreamPool& p = StreamPool::get();
  {
    std::lock_guard<std::mutex> g(p.mu);
    auto& v = p.idle[{dev, priority}];
    if (!v.empty()) {
      hipStream_t s = v.back();
      v.pop_back();
      return s;
    }
  }
  hipStream_t s = nullptr;
  HIP_CHECK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority));
  std::lock_guard<std::mutex> g(p.mu);
  p.owner[s] = {dev, priority};
  return s;
}

void return_stream(hipStream_t s) {
  if (!s) return;
  StreamPool& p = StreamPool::get();
  std::lock_guard<std::mutex> g(p.mu);
  auto it = p.owner.find(s);
  if (it == p.owner.end()) {
    (void)hipStreamDestroy(s);  // not one of ours
    return;
  }
  p.idle[it->second].push_back(s);
}

void prewarm_streams(int device, int n) {
  HIP_CHECK(hipSetDevice(device));
  std::vector<hipStream_t> v;
  for (int i = 0; i < n; ++i) v.push_back(pooled_stream(0));
  for (hipStream_t s : v) return_stream(s);
}

}  // namespace gpu
}  // namespace uda
