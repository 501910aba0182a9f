// GPU prewarm: what a reduce task (at INIT) or a node daemon (at its start) builds ahead of the merges:
// the HIP context and code objects, the SDMA queues, pooled workspaces with their pinned D2H rings.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../gpu/device_ptr.h"
#include "../gpu/device_reduce.h"
#include "../gpu/device_engine.h"
#include "../gpu/fixed_delivery.h"
#include "../gpu/sdma.h"
#include "gpu_workspace.h"
#include "reduce_task.h"
#include "uda/log.h"

namespace uda {

namespace {
// once per process: the context and the library's code objects (loaded at the first kernel launch);
// later prewarms must not hipFree (it synchronizes the device under running tasks)
void warm_code(int device) {
  static std::once_flag code_once;
  std::call_once(code_once, [device] {
    uint8_t* tmp = nullptr;  // raw hipMalloc: the prewarm is not the merge (fault injection hits the merge)
    HIP_CHECK(hipMalloc(&tmp, 4096));
    HIP_CHECK(hipMemsetAsync(tmp, 0, 64, nullptr));
    gpu::launch_max_i32(reinterpret_cast<int32_t*>(tmp), 1, reinterpret_cast<unsigned int*>(tmp + 32), nullptr);
    HIP_CHECK(hipStreamSynchronize(nullptr));
    try {  // the SDMA engines' queues (staging H2D, delivery D2H)
      gpu::SdmaEngine::for_device(device).warm(tmp);
    } catch (const std::exception& e) {
      UDA_LOG(kWarn, "GPU prewarm: SDMA warm-up: %s", e.what());
    }
    HIP_CHECK(hipFree(tmp));
  });
}

// `n` pooled merge workspaces with their pinned D2H rings (NUMA-local), held at once so the pool keeps n
void warm_workspaces(int device, int n) {
  std::vector<std::unique_ptr<PoolLease<DeviceWorkspace>>> held;
  for (int i = 0; i < std::max(1, n); ++i) {
    held.emplace_back(new PoolLease<DeviceWorkspace>{
        device, DevicePool<DeviceWorkspace>::get().acquire(device, [] { return std::make_unique<DeviceWorkspace>(); })});
    auto& wl = *held.back();
    if (wl.obj->ring.size() < (size_t)(2 * kPieceBytes))
      wl.obj->ring.alloc_on_node((size_t)(2 * kPieceBytes), gpu::device_numa_node(device));
    wl.clean = true;
  }
}
}  // namespace

void prewarm_node_merges(int device, int tasks, int64_t round_bytes, int maps, int64_t kv_buf) {
  HIP_CHECK(hipSetDevice(device));
  (void)gpu::SdmaEngine::for_device(device);
  warm_code(device);
  warm_workspaces(device, tasks);
  gpu::prewarm_streams(device, tasks);
  gpu::DeviceReduceConfig cfg;
  cfg.device = device;
  cfg.kv_buf_bytes = kv_buf;
  cfg.round_bytes = round_bytes;
  // the hosted tasks' defaults (mapred.uda.gpu.delivery.pack): their ring blocks carry the unpack staging
  cfg.pack_version = std::max(0, gpu::delivery_pack_version("auto"));
  gpu::prewarm_device_reduce(cfg, std::max(1, maps), tasks);
}

// Every reduce task of a Hadoop job usually runs in a fresh JVM (YarnChild), so what a warm process
// keeps in its pools (HIP context, code objects, pinned rings and arenas, workspaces) a task would build
// on its critical path: a 2 GB task went 27 -> 3.9 GB/s cold (profiles/r3_netmerger2.json). INIT comes
// while most maps still run (reduce slow-start), so the task builds them then. Best effort: any failure
// leaves the merge to build what it needs as before.
void ReduceTask::prewarm_gpu(PrewarmConf pc) {
  const auto t0 = std::chrono::steady_clock::now();
  auto tp = t0;
  std::string phases;
  auto lap = [&](const char* name) {
    const auto t = std::chrono::steady_clock::now();
    char b[48];
    std::snprintf(b, sizeof(b), "%s%s=%.1f", phases.empty() ? "" : " ", name,
                  std::chrono::duration<double, std::milli>(t - tp).count());
    phases += b;
    tp = t;
  };
  try {
    std::call_once(placed_, [this] { place_on_gpu(); });
    if (gpu::device_count() <= 0) return;
    const int device = device_;
    if (hipSetDevice(device) != hipSuccess) return;
    lap("hip");
    try {
      (void)gpu::SdmaEngine::for_device(device);
    } catch (const std::exception&) {
    }
    lap("sdma");
    warm_code(device);
    lap("code");
    // a workspace with its pinned D2H ring (NUMA-local), and an early stager, into the device pools
    warm_workspaces(device, 1);
    if (pc.early_h2d) {
      PoolLease<EarlyStager> sl{device, DevicePool<EarlyStager>::get().acquire(
                                            device, [device] { return std::make_unique<EarlyStager>(device); })};
      sl.clean = true;
    }
    lap("ws");
    // TeraSort-shaped tasks merge through device_reduce_fixed: its pooled workspace, merger and SDMA
    // delivery ring
    {
      gpu::DeviceReduceConfig cfg;
      cfg.device = device;
      cfg.kv_buf_bytes = kv_buf_size_;
      cfg.round_bytes = pc.round_bytes;
      cfg.pack_version = pc.delivery_pack;
      cfg.piece_bytes = pc.delivery_piece_bytes;
      gpu::prewarm_device_reduce(cfg, std::max(1, pc.maps));
    }
    lap("fixed10");
    // pinned blocks for the fetch arena, kept in the pool's cache for this task's partitions (not for
    // tasks that only fetch device descriptors)
    const int64_t pin = pc.pinned_bytes;
    std::vector<gpu::PinnedPool::Block> blocks;
    for (int64_t b = 0; b < pin && !stop_; b += (int64_t)gpu::PinnedArena::kBlock)
      blocks.push_back(gpu::PinnedPool::instance().acquire(gpu::PinnedArena::kBlock));
    for (auto& b : blocks) gpu::PinnedPool::instance().release(b);
    lap("pinned");
  } catch (const std::exception& e) {
    UDA_LOG(kWarn, "GPU prewarm: %s", e.what());
  }
  std::lock_guard<std::mutex> g(st_mu_);
  st_.gpu_prewarm_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  st_.gpu_prewarm_phases = phases;
}

void ReduceTask::join_prewarm() {
  // placed by the prewarm; without one (or if it failed there) here, where a failure fails the task
  if (!prewarm_thr_.joinable()) {
    std::call_once(placed_, [this] { place_on_gpu(); });
    return;
  }
  const auto t0 = std::chrono::steady_clock::now();
  prewarm_thr_.join();
  std::call_once(placed_, [this] { place_on_gpu(); });
  std::lock_guard<std::mutex> g(st_mu_);
  st_.gpu_prewarm_wait_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace uda
