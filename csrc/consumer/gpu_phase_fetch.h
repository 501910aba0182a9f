// The fetch threads of the two progressive merges of the staged GPU path (gpu_merge_staged.cc): every
// partition is fetched in P byte phases, all partitions' phase p before any phase p + 1, so the merge can
// start on the key range that has fully arrived while later phases still come in.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <exception>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../gpu/device_ptr.h"
#include "gpu_workspace.h"
#include "reduce_task.h"
#include "rpq_plan.h"

namespace uda {

constexpr int64_t kSampleSpacing = 256 << 10;  // LPQ sparse-index granularity

// Progressive merge (mapred.uda.gpu.progressive.phases = P > 1, online tasks whose whole input fits
// the device budget): every partition is fetched in P byte phases, all partitions' phase p before
// any phase p + 1, each phase staged to HBM as it lands. After phase p the key range below the least
// last-landed key has fully arrived in every run (plan_progressive_split), so it is merged and its
// output streamed back while phase p + 1 still comes in: the D2H of the output overlaps the H2D of
// the input on the duplex link instead of following it.
struct ProgFetch {
  ReduceTask* task = nullptr;
  const std::atomic<bool>* stop = nullptr;
  EarlyStager* st = nullptr;
  int depth = 1;
  int P = 0, K = 0;
  std::vector<std::shared_ptr<MofFetcher>> f;
  std::vector<uint8_t*> dst, dev;
  std::vector<int64_t> cap;
  std::vector<int64_t> body;  // cap less the partition's IFile checksum trailer (uda/ifile.h), if it has one
  std::vector<int> id;        // the merge's name for the partition's map output
  std::vector<std::vector<int64_t>> landed;  // [phase][run]: end of the bytes that phase fetched
  std::vector<int> done;                     // per phase: partitions whose phase is fetched and queued to HBM
  std::mutex mu;
  std::condition_variable cv;
  std::exception_ptr err;
  std::atomic<int64_t> next{0};
  std::vector<std::thread> threads;
  std::chrono::steady_clock::time_point t_end;
  ~ProgFetch() {
    for (auto& t : threads)
      if (t.joinable()) t.join();
  }
  void start(int nthreads) {
    for (int w = 0; w < nthreads; ++w) threads.emplace_back([this] { work(); });
  }
  void work();
};

// Progressive direct RPQ (mapred.uda.gpu.hybrid.progressive, default on): a task whose input outgrows
// the device budget on the DRAM tier fetches every partition in P byte phases into pinned DRAM, and the
// fetch threads index each run as its phases land (in order per run). After phase p the key range below
// the least last-complete key of the unfinished runs has fully arrived in every run: it is merged in
// RPQ rounds (slices H2D, merge, D2H, as the direct RPQ) while later phases still come in. Without it
// the RPQ rounds start after the last byte landed (the reference's fetcher-ahead-of-LPQ pipeline,
// MergeManager.cc:202-288, is what this recovers).
struct DirectProg {
  ReduceTask* task = nullptr;
  const std::atomic<bool>* stop = nullptr;
  int depth = 1;
  int P = 0, K = 0;
  int64_t spacing = kSampleSpacing;        // index sample spacing of the runs
  std::vector<std::shared_ptr<MofFetcher>> f;
  std::vector<uint8_t*> dst;
  std::vector<int64_t> cap;
  std::vector<int64_t> body;  // cap less the partition's IFile checksum trailer: the bytes that are indexed
  std::vector<std::vector<char>> fetched;  // [k][p]
  std::vector<int> indexed;                // [k]: phases of run k indexed
  std::vector<char> indexing;              // [k]: a thread is indexing run k
  std::vector<RunCursor> cur;              // [k]: touched by the thread indexing run k only
  std::vector<std::vector<int64_t>> cut;   // [k]: samples so far (appended under mu)
  std::vector<std::vector<std::string>> key;
  std::vector<int64_t> complete;           // [k]: end of the last complete record indexed
  std::vector<std::string> last_key;       // [k]: key of that record ("" none yet)
  std::vector<char> eof;                   // [k]: the partition is indexed to its EOF marker
  std::vector<int> phase_runs;             // [p]: runs indexed through phase p
  std::vector<gpu::PinnedPool::Block> blocks;  // [k]: the pinned span of partition k (back to the pool at the end)
  std::mutex mu;
  std::condition_variable cv;
  std::exception_ptr err;
  std::atomic<int64_t> next{0};
  std::vector<std::thread> threads;
  std::chrono::steady_clock::time_point t_end;
  ~DirectProg() {
    for (auto& t : threads)
      if (t.joinable()) t.join();
    for (auto& b : blocks) gpu::PinnedPool::instance().release(b);
  }
  void start(int nthreads) {
    for (int w = 0; w < nthreads; ++w) threads.emplace_back([this] { work(); });
  }
  void work();
  void index_landed(int k, std::unique_lock<std::mutex>& lk);
};

}  // namespace uda
