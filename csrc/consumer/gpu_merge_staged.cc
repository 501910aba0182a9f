// NetMerger GPU backend (mapred.uda.merge.backend=gpu), staged path: ReduceTask::merge_gpu().
//
// Online (the reduce input fits the device budget): every fetched MOF partition is staged in HBM
// (compressed partitions cross PCIe compressed and are decoded there by the F6 kernels), the whole
// input is merged by the generic HIP merge tree (csrc/gpu/generic.hip) and streamed back to the
// host reducer through dataFromUda in whole-record buffers.
//
// Hybrid (input larger than the budget, mapred.uda.gpu.merge.bytes): the reference's two-level
// merge (merge_hybrid, src/Merger/MergeManager.cc:195-290) re-planned for a device:
//   LPQ  (disk tier, or mapred.uda.gpu.hybrid.direct=0) MOFs are grouped as they arrive; each group
//        is merged on the GPU and spilled to the local dirs through AsyncIO (io_uring) or to DRAM,
//        with a sparse index: the key at every record boundary the merge placed <= 256 KiB apart.
//        DRAM tier by default: no LPQ level; the fetched partitions are the runs, indexed the same
//        way by the drain threads (direct RPQ, see StagedMerge::overflow).
//   RPQ  instead of a streaming heap over the runs, the key space is cut into rounds from the
//        sparse indices (splitters every ~budget/2 bytes, rpq_plan.h); for each round the matching
//        byte range of every run is copied to HBM and merged on the GPU in one go. Records equal to a
//        splitter all fall in the later round, in every run, so ties keep run order.
// Reference counterpart of the online path: merge_online (MergeManager.cc:184-193).
#include <fcntl.h>
#include <sys/stat.h>
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <optional>
#include <random>
#include <thread>

#include "../gpu/device_ptr.h"
#include "../gpu/generic_rounds.h"
#include "../gpu/hbm_ledger.h"
#include "../gpu/sdma.h"
#include "gpu_phase_fetch.h"
#include "gpu_workspace.h"
#include "reduce_task.h"
#include "rpq_plan.h"
#include "uda/aio.h"
#include "uda/fault.h"
#include "uda/ifile.h"
#include "uda/log.h"
#include "uda/safe_file.h"
#include "uda/trace.h"

namespace uda {

namespace {

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// index_host_run of a whole fetched partition, with its "index" trace event
SpillRun index_partition(uint8_t* p, int64_t len) {
  const int64_t tt = trace::host_enabled() ? trace::now_ns() : 0;
  SpillRun run = index_host_run(p, len, kSampleSpacing);
  if (tt) trace::host_event("index", len, (int64_t)run.cut.size(), tt, trace::now_ns());
  return run;
}

// Three workspaces and streams of the pipelined RPQ rounds: round q + 2's slices cross PCIe (SDMA H2D)
// while round q + 1 merges and round q is delivered (D2H), so the rounds cost max(H2D, merge, D2H) each
// instead of H2D + merge. At most three rounds are in flight: workspace q % 3 is free again once round
// q - 3 has been delivered.
struct RpqPipeline {
  StreamGuard sg2, sg3;
  DeviceWorkspace* ws[3] = {nullptr, nullptr, nullptr};
  hipStream_t s[3] = {nullptr, nullptr, nullptr};
};

// merge-owned state of the progressive direct RPQ's planner (StagedMerge::plan_more)
struct DirectPlan {
  std::vector<SpillRun> runs;   // views of the runs: the landed, indexed prefix of every partition
                                // (.mem set once the fetch threads have pinned the spans)
  std::vector<int64_t> at;      // merged so far (a record boundary)
  std::vector<size_t> taken;    // samples copied into runs[k]
  // every round is a list of per-run [b, e) slices of the pinned partitions; rounds queue up as the
  // phases land and the pipeline takes them in order
  std::vector<RoundSlices> rounds;
  bool planned_all = false;
  int64_t target = 0;
  int epoch = 0;
  std::vector<char> eof;        // runs[k].bytes is final: the run is indexed to its EOF marker
};

// mapred.uda.ifile.checksum.over.budget=verify over direct RPQ rounds: the partitions never lie whole in HBM,
// but a run's slices are contiguous over the rounds (slice_rounds: b[k][q] to b[k][q + 1]), so every body
// byte passes through HBM once, in order. Each round's device_merge leaves one raw CRC state per slice
// (ChecksumPolicy::slice_states); the delivering thread folds a run's states in round order and compares
// with the stored value once the run's body is complete. Runs without a trailer are not folded.
class SliceChecksums {
 public:
  void add_run(bool trailer, int64_t body, const std::string& map_id) {
    runs_.push_back(Run{trailer, !trailer, body, map_id, Crc32Running()});
    any_ = any_ || trailer;
  }
  bool any() const { return any_; }
  size_t size() const { return runs_.size(); }
  bool open(size_t k) const { return !runs_[k].closed; }
  int64_t folded(size_t k) const { return runs_[k].crc.bytes(); }
  // slice [b, e) of run k went through HBM with state `st`; bytes between the last slice and this one (none,
  // as the rounds are planned) are folded on the host from the pinned partition at mem
  void fold(size_t k, const uint8_t* mem, int64_t b, int64_t e, uint32_t st) {
    Run& r = runs_[k];
    if (b < r.crc.bytes() || e < b || e > r.body)
      throw UdaError("RPQ slice [" + std::to_string(b) + ", " + std::to_string(e) + ") of map output " + r.map_id +
                     " does not follow the " + std::to_string(r.crc.bytes()) + " bytes checksummed so far");
    if (b > r.crc.bytes()) r.crc.append_bytes(mem + r.crc.bytes(), (size_t)(b - r.crc.bytes()));
    r.crc.append_state(st, e - b);
  }
  // The run's last slice is in: the body bytes no slice carries (the EOF marker, which the run's index leaves
  // out) from the host copy, then the comparison with the trailer behind the body. Returns the body's length.
  int64_t close(size_t k, const uint8_t* mem) {
    Run& r = runs_[k];
    r.crc.append_bytes(mem + r.crc.bytes(), (size_t)(r.body - r.crc.bytes()));
    r.closed = true;
    const uint32_t stored = ifile_stored_checksum(mem + r.body), got = r.crc.value();
    if (stored != got) throw UdaError(ifile_checksum_mismatch(r.map_id, stored, got, r.body));
    return r.body;
  }

 private:
  struct Run {
    bool trailer, closed;
    int64_t body;
    std::string map_id;
    Crc32Running crc;
  };
  std::vector<Run> runs_;
  bool any_ = false;
};

}  // namespace

// ReduceTask::merge_gpu() as an object: what were the function's locals are members, its steps methods.
class StagedMerge {
 public:
  explicit StagedMerge(ReduceTask& t) : t_(t), maps_(t.init_.num_maps), device_(t.device_) {
    map_ids_.reserve((size_t)std::max(maps_, 0));  // (read by the LPQ thread while the fetch appends: never regrown)
  }
  void run();

 private:
  // setup
  void acquire_gate();
  void read_conf();
  void acquire_resources();
  void restore_checkpoint();
  // fetch
  void fetch();
  bool decide_progressive(const std::vector<std::shared_ptr<MofFetcher>>& ready);
  void start_direct_prog(const std::vector<std::shared_ptr<MofFetcher>>& ready, int64_t tot);
  void start_prog_fetch(const std::vector<std::shared_ptr<MofFetcher>>& ready);
  void drain_ready(const std::vector<std::shared_ptr<MofFetcher>>& ready);
  void drain_batch(const std::vector<std::shared_ptr<MofFetcher>>& ready, const std::vector<size_t>& sub);
  void overflow();
  void spill_group();
  void lpq_wait();
  void merge_spill(std::vector<Span> jg, std::vector<std::string> ids, EarlyStager* st);
  void index_spans(const std::vector<Span>& spans, size_t first, std::vector<SpillRun>* out) const;
  void count_decoded(const DeviceMergeOut& m);
  void count_checksums(const DeviceMergeOut& m);
  int span_id(const std::string& map_id);
  // delivery
  void deliver(const DeviceMergeOut& m, bool last, hipStream_t ds, DeviceWorkspace& w);
  gpu::GenericMerger::RoundFn round_sink(bool last_phase);
  // modes
  void run_progressive_direct();
  bool plan_more(DirectPlan& pl, bool wait);
  void run_progressive();
  void run_online();
  void run_hybrid();
  void read_run(const SpillRun& run, int64_t off, int64_t len, uint8_t* dst);
  std::vector<std::vector<int64_t>> run_bounds(const std::vector<std::string>& split);
  void open_pipeline(RpqPipeline* pipe);
  void fold_slices(const RoundSlices& rr, const DeviceMergeOut& m, const std::vector<uint8_t*>& mems,
                   const std::vector<int64_t>& fin, bool last, const std::function<void(size_t)>& landed);
  // end
  void cleanup(bool ok);
  void finish();

  ReduceTask& t_;
  const int maps_;
  const int device_;
  std::chrono::steady_clock::time_point t0_;
  // configuration (read_conf)
  bool device_decode_ = false;
  Codec fetch_codec_ = Codec::kNone, stage_codec_ = Codec::kNone;
  int64_t budget_ = 0;  // device budget per merge: in + out + elements + side tables ~ 3x the input
  std::string tier_;
  bool early_h2d_ = false;
  int depth_ = 4;
  int64_t stage_step_ = 0, drains_ = 8;
  int prog_phases_ = 0, pdirect_phases_ = 1;
  bool prog_auto_ = false, prog_ok_ = false, direct_ok_ = false, pdirect_ok_ = false;
  bool ckpt_ = false;
  std::string manifest_;
  std::vector<std::string> dirs_;
  int64_t kv_ = 0;
  // state of the run
  bool prog_decided_ = false, progressive_ = false, direct_ = false;
  int drained_ = 0;
  int64_t group_raw_ = 0;
  size_t checkpointed_ = 0;
  double fetch_ms_ = 0, prog_fetch_ms_ = -1;
  std::atomic<int64_t> combine_in_{0};  // (the LPQ thread counts its merges' input too)
  bool combine_skipped_ = false;
  // IFile checksum trailers (uda/ifile.h, mapred.uda.ifile.checksum): partitions whose trailer was stripped,
  // and of those verified on the device. The online and progressive merges verify every one; over budget
  // (LPQ spills, RPQ rounds over partitions that never lie whole in HBM) they are stripped unverified unless
  // mapred.uda.ifile.checksum.over.budget=verify.
  std::atomic<int64_t> trailers_{0}, verified_{0};
  std::vector<std::string> map_ids_;  // Span::id -> map output, for the mismatch message
  ChecksumPolicy verify_ck_, strip_ck_;
  // mapred.uda.ifile.checksum.over.budget=verify (under auto): the LPQ merges verify their groups (lpq_ck_ is
  // verify_ck_, else strip_ck_), the direct RPQ rounds ask for slice states (slice_ck_) and slice_sums_ folds them
  bool verify_over_ = false;
  ChecksumPolicy lpq_ck_, slice_ck_;
  SliceChecksums slice_sums_;
  double slice_ms_ = 0;  // device CRC time of rounds not yet booked with a closed run
  // over budget under mapred.uda.merge.combine.over.budget=combine: the op of the RPQ rounds, and of the
  // LPQ merges (kNone under an LPQ checkpoint: its spills stay as a resumed attempt expects them)
  CombineOp hybrid_combine_ = CombineOp::kNone, lpq_combine_ = CombineOp::kNone;
  // The budget counts ~3x the input per merge; a combining merge holds 17 B per record more (group index,
  // sums: 0.27 of the input at 64 B records, as the device path's admission counts them), so its input
  // shrinks by 3 / 3.27: an RPQ round's target of half the budget, and an LPQ group's whole budget. A numeric
  // key kind (mapred.uda.key.order=hadoop) holds its normalized keys, 8 B per record (0.125 of the input), as well.
  int64_t less_combine(int64_t b, CombineOp op) const {
    const double extra = (op != CombineOp::kNone ? 0.27 : 0.0) + (key_kind_numeric(t_.kind_) ? 0.125 : 0.0);
    return extra > 0 ? (int64_t)((double)b * (3.0 / (3.0 + extra))) : b;
  }
  int64_t round_target() const { return less_combine(budget_ / 2, hybrid_combine_); }
  // (with direct RPQ there is no LPQ merge: the budget only decides when the task stops being an online one)
  int64_t group_budget() const { return direct_ok_ ? budget_ : less_combine(budget_, lpq_combine_); }
  // Sparse-index granularity of an LPQ spill. A combined spill can be far smaller than the budget, so it is
  // sampled as finely as DirectProg samples partitions: the RPQ planner can then still cut it into rounds.
  int64_t lpq_spacing() const {
    if (lpq_combine_ == CombineOp::kNone) return kSampleSpacing;
    return std::clamp<int64_t>(budget_ / 64, 4 << 10, kSampleSpacing);
  }
  bool eof_sent_ = false;
  std::vector<uint8_t> tail_;
  hipStream_t s_ = nullptr;
  DeviceWorkspace* ws_ = nullptr;
  DeviceWorkspace* ws2_ = nullptr;
  DeviceWorkspace* ws3_ = nullptr;
  EarlyStager* stager_ = nullptr;
  EarlyStager* job_stager_ = nullptr;
  gpu::PinnedArena* fill_mem_ = &group_mem_;
  gpu::PinnedArena* job_mem_ = &group_mem2_;

  // Owners, in the declaration order of the function this was (destroyed in reverse). The members that own
  // threads come last, so they are joined before anything their threads use goes away: prog_ / dprog_
  // (fetch threads: the arenas, stager and workspace leases above them), lpq_join_ (the LPQ thread: all of
  // the above) and direct_head_ (a std::async future whose destructor blocks: group_, index_spans).
  GateLease gate_;
  StreamGuard sg_;
  PoolLease<DeviceWorkspace> ws_lease_{device_, nullptr};
  PoolLease<DeviceWorkspace> ws2_lease_{device_, nullptr}, ws3_lease_{device_, nullptr};  // pipelined RPQ rounds
  // uncompressed partitions go to HBM as soon as each one is complete (overlapping the fetch)
  // Two stagers: the group being fetched is staged by `stager_` while the LPQ thread merges the
  // previous group out of `job_stager_`'s arena; spill_group swaps them.
  PoolLease<EarlyStager> stager_lease_{device_, nullptr}, stager_lease2_{device_, nullptr};
  std::vector<SpillRun> spills_;
  std::vector<Span> group_;          // fetched partitions of the current group (pinned, group_mem_)
  gpu::PinnedArena group_mem_, spill_mem_;
  std::unique_ptr<AsyncIO> aio_;
  std::optional<StagedCount> staged_count_;
  std::vector<std::string> group_ids_;  // MOFs of the current group (for the manifest)
  // The group being fetched lives in fill_mem_ (and is staged to HBM by `stager_`); the one being merged
  // in job_mem_ (its HBM copies in job_stager_'s arena), so the next group's H2D overlaps an LPQ merge.
  gpu::PinnedArena group_mem2_;
  std::vector<SpillRun> direct_runs_;  // one per partition drained after the switch, in `group_` order
  std::unique_ptr<ProgFetch> prog_;
  std::unique_ptr<DirectProg> dprog_;
  std::thread lpq_thr_;
  std::exception_ptr lpq_err_;
  struct LpqJoin {
    std::thread& t;
    ~LpqJoin() {
      if (t.joinable()) t.join();
    }
  } lpq_join_{lpq_thr_};
  std::future<std::vector<SpillRun>> direct_head_;  // partitions drained before the switch, indexed meanwhile
};

void ReduceTask::merge_gpu() {
  join_prewarm();
  StagedMerge(*this).run();
}

void StagedMerge::run() {
  if (gpu::device_count() <= 0) throw UdaError("mapred.uda.merge.backend=gpu but no HIP device is visible");
  {
    std::lock_guard<std::mutex> g(t_.st_mu_);
    t_.st_.merge_path = "staged";
  }
  t0_ = std::chrono::steady_clock::now();
  if (hipSetDevice(device_) != hipSuccess) throw UdaError("hipSetDevice failed");
  acquire_gate();
  read_conf();
  acquire_resources();
  restore_checkpoint();
  try {
    fetch();
    // ---- delivery of merged rounds; EOF rides in the very last buffer
    tail_.resize((size_t)t_.kv_buf_size_ + kEofBytes);
    kv_ = t_.kv_buf_size_ - kEofBytes;
    lpq_wait();  // an LPQ of the fetch phase may still be merging
    // mapred.uda.merge.combine: the online and progressive merges combine; the over-budget hybrid (LPQ /
    // RPQ rounds, progressive direct) delivers the uncombined stream, which a combiner allows, unless
    // mapred.uda.merge.combine.over.budget=combine: then every RPQ round (and LPQ merge) combines, the host
    // planner never splitting equal keys between rounds (rpq_plan.h)
    if (dprog_) {
      run_progressive_direct();
    } else if (progressive_) {
      run_progressive();
    } else if (spills_.empty() && !direct_) {
      run_online();
    } else {
      run_hybrid();
    }
    if (!eof_sent_) {  // empty final round (or empty input): EOF alone
      const uint8_t eof[2] = {0xFF, 0xFF};
      if (t_.host_->data_from_uda(eof, kEofBytes) != 0) throw UdaError("dataFromUda callback failed");
      std::lock_guard<std::mutex> g(t_.st_mu_);
      t_.st_.buffers++;
      t_.st_.bytes_delivered += kEofBytes;
    }
    finish();
  } catch (...) {
    if (lpq_thr_.joinable()) lpq_thr_.join();  // the LPQ thread uses this object's state
    cleanup(false);
    throw;
  }
}

// ---------------------------------------------------------------------------------------- setup
void StagedMerge::acquire_gate() {
  // Off by default: a gated task fetches nothing until all its FETCHes are in, which under reduce
  // slow-start gives up the fetch / map-phase overlap. With every map output already there, 16
  // concurrent host-MOF TeraSort tasks reach 20.8 GB/s unlimited and 31.2 / 34.3 / 32.6 with 4 / 6 / 8
  // slots (profiles/r2_api_host_mofs_gate_sweep.md): set it for jobs whose reduces start after the maps.
  if (const int cap = (int)t_.host_->conf_i64("mapred.uda.gpu.max.concurrent.merges", 0); cap > 0) {
    const auto w0 = std::chrono::steady_clock::now();
    // A task asks for a slot only once every map has been announced (all FETCH commands in): a task
    // still waiting for map outputs (reduce slow-start) must not hold a slot, and a host that feeds the
    // tasks' FETCHes one task after another cannot deadlock against the gate.
    {
      std::unique_lock<std::mutex> lk(t_.mu_);
      while (!t_.stop_ && !t_.final_ && t_.fetch_cmds_ < maps_) t_.cv_.wait_for(lk, std::chrono::milliseconds(50));
    }
    if (!DeviceGate::get().acquire(device_, cap, [&] { return t_.stop_.load(); }))
      throw UdaError("reduce task stopped while waiting for a GPU merge slot");
    gate_.device = device_;
    std::lock_guard<std::mutex> g(t_.st_mu_);
    t_.st_.gpu_gate_wait_ms = ms_since(w0);
  }
}

// every configuration read of the merge, once, on the merge thread
void StagedMerge::read_conf() {
  Host* host = t_.host_;
  device_decode_ = t_.codec_ != Codec::kNone && host->conf_i64("mapred.uda.gpu.decompress", 1) != 0;
  fetch_codec_ = device_decode_ ? Codec::kNone : t_.codec_;
  stage_codec_ = device_decode_ ? t_.codec_ : Codec::kNone;
  budget_ = host->conf_i64("mapred.uda.gpu.merge.bytes", 0);
  if (budget_ <= 0) {
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    budget_ = (int64_t)(free_b / 4);
  }
  // and within the device's HBM budget (mapred.uda.gpu.hbm.budget, hbm_ledger.h): three pipelined RPQ
  // rounds of budget/2 input, each workspace ~3x its input, come to ~4.5x the input budget (the stager's
  // blocks are released at the switch to direct rounds)
  {
    const int64_t hr = gpu::HbmLedger::get().headroom(device_);
    if (hr > 0 && budget_ > hr / 5) {
      budget_ = std::max<int64_t>(hr / 5, 64ll << 20);
      std::lock_guard<std::mutex> g(t_.st_mu_);
      t_.st_.merge_budget_from_ledger = 1;
    }
  }
  tier_ = host->get_conf("mapred.uda.gpu.spill", t_.init_.local_dirs.empty() ? "host" : "disk");
  early_h2d_ = fetch_codec_ == Codec::kNone && stage_codec_ == Codec::kNone &&
               host->conf_i64("mapred.uda.gpu.early.h2d", 1) != 0;
  depth_ = (int)std::max<int64_t>(1, host->conf_i64("mapred.uda.gpu.fetch.depth", 4));
  // early staging granularity: <= 0 (default) copies each partition once it is complete; > 0 copies
  // every `step` bytes of its landed prefix. Measured on the 2 GB secondary sort, 8 MiB pieces made the
  // fetch 70-200 ms instead of 21-25 ms (either copy path, SDMA or blit), while a standalone probe
  // (tools/host_dma_contention.py) shows CPU copies into pinned memory unaffected by a concurrent H2D;
  // the cause is not understood, so piecewise staging stays opt-in.
  stage_step_ = host->conf_i64("mapred.uda.gpu.early.h2d.step", 0);
  // MOFs drained at once (0: all that have arrived). 8 keeps partitions completing one after another,
  // so each one's H2D overlaps the remaining fetch: 2 GB secondary sort 23.3 GB/s vs 12.7-21 with all 64.
  drains_ = host->conf_i64("mapred.uda.gpu.fetch.drains", 8);
  dirs_ = t_.init_.local_dirs;
  if (dirs_.empty()) dirs_.push_back("/tmp");
  // LPQ checkpoint (disk tier): spills_[0, checkpointed_) are fsynced, indexed in <path>.idx and
  // listed in the manifest; a failed attempt keeps them for the next one
  ckpt_ = t_.checkpoint_ && tier_ == "disk";
  verify_ck_ = ChecksumPolicy{t_.checksum_ == ChecksumMode::kAuto, &map_ids_};
  strip_ck_ = ChecksumPolicy{false, &map_ids_};
  verify_over_ = verify_ck_.verify && t_.checksum_over_budget_;
  lpq_ck_ = verify_over_ ? verify_ck_ : strip_ck_;
  slice_ck_ = ChecksumPolicy{false, &map_ids_, true};
  hybrid_combine_ = t_.combine_over_budget_ ? t_.combine_ : CombineOp::kNone;
  lpq_combine_ = ckpt_ ? CombineOp::kNone : hybrid_combine_;
  // Progressive phases (ProgFetch). Default (-1): 4 phases when the task is the only staged GPU merge on
  // its device when it decides (a lone task: 22 -> 26.3-26.8 GB/s on the 2 GB secondary sort); concurrent
  // tasks already overlap each other's H2D and D2H and gain nothing
  // (profiles/r3_api_host_mofs_progressive_ab.txt).
  const int64_t prog_conf = host->conf_i64("mapred.uda.gpu.progressive.phases", -1);
  prog_phases_ = (int)std::min<int64_t>(EarlyStager::kGroups, prog_conf < 0 ? 4 : prog_conf);
  prog_auto_ = prog_conf < 0;
  // over budget, DRAM tier: phases into pinned DRAM, RPQ rounds of every fully arrived key range (DirectProg)
  pdirect_phases_ = (int)std::max<int64_t>(1, host->conf_i64("mapred.uda.gpu.hybrid.progressive.phases", 16));
  manifest_ = ckpt_ ? t_.checkpoint_path() : std::string();
  // Direct RPQ (mapred.uda.gpu.hybrid.direct, default on, DRAM tier, uncompressed partitions, at most
  // mapred.uda.gpu.hybrid.direct.max.runs maps): once the input outgrows the device budget, the
  // fetched partitions stay where the fetch put them (pinned DRAM, already sorted runs) and are indexed
  // by the drain threads; the RPQ key-range rounds then merge slices of all of them. The reference's
  // LPQ level (MergeManager.cc:202-288) bounds a CPU heap's fan-in and spills to disk; on this tier it
  // would only re-sort bytes already in DRAM, at two extra PCIe crossings (LPQ H2D + spill D2H), while
  // the device K-way merge takes hundreds of runs per round. The disk tier keeps the LPQ level.
  direct_ok_ = tier_ == "host" && t_.codec_ == Codec::kNone && t_.restored_files_.empty() && !ckpt_ &&
               host->conf_i64("mapred.uda.gpu.hybrid.direct", 1) != 0 &&
               maps_ <= host->conf_i64("mapred.uda.gpu.hybrid.direct.max.runs", 1024);
  pdirect_ok_ = direct_ok_ && pdirect_phases_ > 1 && host->conf_i64("mapred.uda.gpu.hybrid.progressive", 1) != 0;
}

void StagedMerge::acquire_resources() {
  sg_.s = gpu::pooled_stream();
  s_ = sg_.s;
  ws_lease_.obj = pooled_workspace(device_);
  ws_ = ws_lease_.obj.get();
  ws_->reset_stats();
  if (early_h2d_) {
    stager_lease_.obj = pooled_stager(device_);
    stager_ = stager_lease_.obj.get();
    stager_->reset();
  }
  staged_count_.emplace(device_);
  prog_ok_ = prog_phases_ > 1 && stager_ && stager_->sdma() && t_.restored_files_.empty() && !ckpt_;
}

// resume: restored LPQ spills (data + sparse index) of a failed attempt
void StagedMerge::restore_checkpoint() {
  if (ckpt_ && t_.restored_files_.empty()) ::unlink(manifest_.c_str());
  for (const std::string& path : t_.restored_files_) {
    SpillRun run;
    run.path = path;
    run.fd = ::open(path.c_str(), O_RDWR | O_CLOEXEC);
    struct stat sb;
    if (run.fd < 0 || ::fstat(run.fd, &sb) != 0) throw UdaError("cannot reopen checkpointed LPQ " + path);
    run.bytes = (int64_t)sb.st_size;
    read_lpq_index(path + ".idx", &run.cut, &run.key);
    spills_.push_back(std::move(run));
  }
  checkpointed_ = spills_.size();
  if (!spills_.empty()) {
    if (!aio_) aio_ = AsyncIO::create(AsyncIO::Options{});
    std::lock_guard<std::mutex> g(t_.st_mu_);
    t_.st_.restored_lpqs = (int64_t)spills_.size();
    t_.st_.restored_maps = (int64_t)t_.restored_maps_.size();
    t_.st_.maps_fetched += (int64_t)t_.restored_maps_.size();
  }
}

// ---------------------------------------------------------------------------------------- fetch
// start every MOF (bounded by the buffer pool), drain each fully into host memory
void StagedMerge::fetch() {
  std::mt19937_64 rng((uint64_t)std::chrono::steady_clock::now().time_since_epoch().count());
  int started = (int)t_.restored_maps_.size();
  drained_ = started;
  t_.total_count_ += started;
  if (started > 0 && t_.total_count_ == maps_) t_.host_->fetch_over();
  std::vector<FetchParams> pending;
  std::vector<std::shared_ptr<MofFetcher>> ready;
  while (drained_ < maps_) {
    std::vector<std::shared_ptr<MofFetcher>> to_start;
    {
      std::unique_lock<std::mutex> lk(t_.mu_);
      t_.cv_.wait(lk, [&] {
        return t_.stop_ || !t_.fetched_.empty() ||
               ((!t_.fetch_list_.empty() || !pending.empty()) && t_.free_pairs_ > 0 && started < maps_);
      });
      if (t_.stop_) throw UdaError("reduce task stopped during fetch");
      while (!t_.fetch_list_.empty()) {
        pending.push_back(t_.fetch_list_.front());
        t_.fetch_list_.pop_front();
      }
      std::shuffle(pending.begin(), pending.end(), rng);
      while (!pending.empty() && t_.free_pairs_ > 0 && started < maps_) {
        to_start.push_back(std::make_shared<MofFetcher>(&t_, pending.back(), t_.buffer_size_, fetch_codec_));
        pending.pop_back();
        t_.free_pairs_--;
        started++;
      }
      while (!t_.fetched_.empty()) {
        ready.push_back(t_.fetched_.front());
        t_.fetched_.pop_front();
      }
    }
    for (auto& f : to_start) f->start();
    if ((prog_ok_ || pdirect_ok_) && !prog_decided_) {
      if (drained_ + (int)ready.size() < maps_) continue;  // every partition's length before deciding
      if (decide_progressive(ready)) {
        drained_ = maps_;  // the phases run on the fetch threads; the merge consumes them
        ready.clear();
        continue;
      }
    }
    drain_ready(ready);
    ready.clear();
  }
  fetch_ms_ = ms_since(t0_);
  if (stager_ && std::getenv("UDA_STAGE_TRACE"))
    std::fprintf(stderr, "[stage] fetch %.1f ms, early H2D (%s) %lld copies of %.1f MB issued in %.1f ms, step %lld\n",
                 fetch_ms_, stager_->engine(), (long long)stager_->copies(), stager_->bytes() / 1e6, stager_->issue_ms(),
                 (long long)stage_step_);

  if (trace::host_enabled()) trace::host_event("fetch_phase", stage_step_, drains_, trace::now_ns() - (int64_t)(fetch_ms_ * 1e6), trace::now_ns());
}

// every partition's first chunk is in: progressive (fits the budget), progressive direct RPQ (does not), or
// neither (false: the partitions are drained whole)
bool StagedMerge::decide_progressive(const std::vector<std::shared_ptr<MofFetcher>>& ready) {
  prog_decided_ = true;
  int64_t tot = 0;
  for (auto& f : ready) tot += std::max<int64_t>(f->part_len(), 0);
  progressive_ = prog_ok_ && drained_ == 0 && tot <= budget_ && (!prog_auto_ || staged_merges(device_).load() == 1);
  if (!progressive_ && pdirect_ok_ && drained_ == 0 && tot > budget_) {
    start_direct_prog(ready, tot);
    return true;
  }
  if (progressive_) start_prog_fetch(ready);
  return progressive_;
}

void StagedMerge::start_direct_prog(const std::vector<std::shared_ptr<MofFetcher>>& ready, int64_t tot) {
  {
    std::lock_guard<std::mutex> g(t_.st_mu_);
    t_.st_.merge_path = "staged-progressive-direct";
    t_.st_.hybrid_direct = 1;
  }
  if (stager_) {  // the partitions never go to HBM whole: RPQ rounds copy their slices
    stager_->release_blocks();
    stager_ = nullptr;
  }
  // the partitions' pinned spans come back to the pool when the task ends: keep them cached for the
  // next task of this size instead of re-pinning them
  gpu::PinnedPool::instance().raise_cache_cap((size_t)(tot + tot / 8));
  dprog_ = std::make_unique<DirectProg>();
  DirectProg& dp = *dprog_;
  dp.task = &t_;
  dp.stop = &t_.stop_;
  dp.depth = depth_;
  dp.P = pdirect_phases_;
  dp.K = (int)ready.size();
  // samples fine enough that a round of budget/2 can be cut from K runs (a few per run and round):
  // 256 KiB for GB partitions, finer for small tasks under a small budget
  dp.spacing = std::clamp<int64_t>(budget_ / 2 / (4 * std::max(1, dp.K)), 4 << 10, kSampleSpacing);
  dp.f = ready;
  for (auto& f : ready) {
    const int64_t cap = std::max<int64_t>(f->part_len(), 0);
    const int tail = ifile_trailer_bytes(f->raw_len(), cap);  // (uncompressed partitions only get here)
    dp.cap.push_back(cap);
    dp.body.push_back(cap - tail);
    if (tail) ++trailers_;
    if (verify_over_) slice_sums_.add_run(tail != 0, cap - tail, f->params().map_id);
  }
  const size_t K = (size_t)dp.K;
  // each partition's pinned span is taken by the thread that fetches its first phase (in parallel,
  // beside the first fetches: pinning GBs serially here held up the whole fetch)
  dp.dst.assign(K, nullptr);
  dp.blocks.assign(K, gpu::PinnedPool::Block{});
  dp.fetched.assign(K, std::vector<char>((size_t)dp.P, 0));
  dp.indexed.assign(K, 0);
  dp.indexing.assign(K, 0);
  dp.cur.assign(K, RunCursor());
  dp.cut.assign(K, {});
  dp.key.assign(K, {});
  dp.complete.assign(K, 0);
  dp.last_key.assign(K, std::string());
  dp.eof.assign(K, 0);
  dp.phase_runs.assign((size_t)dp.P, 0);
  // fetch threads: enough to stay ahead of the merge, few enough not to slow the consumer they overlap
  const int64_t pt = t_.host_->conf_i64("mapred.uda.gpu.hybrid.progressive.threads", drains_ > 0 ? drains_ : 8);
  dp.start((int)std::max<int64_t>(1, std::min<int64_t>(pt, dp.K)));
}

void StagedMerge::start_prog_fetch(const std::vector<std::shared_ptr<MofFetcher>>& ready) {
  {
    std::lock_guard<std::mutex> g(t_.st_mu_);
    t_.st_.merge_path = "staged-progressive";
  }
  prog_ = std::make_unique<ProgFetch>();
  ProgFetch& pf = *prog_;
  pf.task = &t_;
  pf.stop = &t_.stop_;
  pf.st = stager_;
  pf.depth = depth_;
  pf.P = prog_phases_;
  pf.K = (int)ready.size();
  pf.f = ready;
  for (auto& f : ready) {
    const int64_t cap = std::max<int64_t>(f->part_len(), 0);
    const int tail = ifile_trailer_bytes(f->raw_len(), cap);  // (uncompressed: the stager needs them so)
    pf.cap.push_back(cap);
    pf.body.push_back(cap - tail);
    pf.id.push_back(span_id(f->params().map_id));
    if (tail) ++trailers_;
    pf.dst.push_back(fill_mem_->alloc((size_t)std::max<int64_t>(cap, 1)));
    pf.dev.push_back(stager_->reserve(cap));
  }
  pf.landed.assign((size_t)pf.P, std::vector<int64_t>((size_t)pf.K, 0));
  pf.done.assign((size_t)pf.P, 0);
  pf.start((int)std::max<int64_t>(1, std::min<int64_t>(drains_ > 0 ? drains_ : 8, pf.K)));
}

// Drain arrived MOFs in parallel (each drain keeps one request in flight ahead) straight into
// pinned spans of the group arena. Group boundaries are decided before a MOF is drained (on
// its partition length), so a group is complete in host memory when it is merged and spilled.
void StagedMerge::drain_ready(const std::vector<std::shared_ptr<MofFetcher>>& ready) {
  size_t next = 0;
  while (next < ready.size()) {
    std::vector<size_t> sub;
    while (next < ready.size()) {
      const int64_t pl = std::max<int64_t>(ready[next]->part_len(), 0);
      const int64_t est = pl * (t_.codec_ != Codec::kNone ? 3 : 1);  // decoded size estimate
      if (!direct_ && (!group_.empty() || !sub.empty()) && group_raw_ + est > group_budget()) break;
      sub.push_back(next++);
      group_raw_ += est;
    }
    if (sub.empty()) {  // the group is full: merge and spill it (or go direct), then admit the MOF
      overflow();
      continue;
    }
    drain_batch(ready, sub);
    if (next < ready.size()) overflow();  // the next MOF did not fit this group
  }
}

void StagedMerge::drain_batch(const std::vector<std::shared_ptr<MofFetcher>>& ready, const std::vector<size_t>& sub) {
  const bool index_now = direct_;  // direct RPQ: each drain thread indexes its partition
  EarlyStager* const stager = stager_;
  const int64_t stage_step = stage_step_;
  std::vector<SpillRun> sub_idx(index_now ? sub.size() : 0);
  std::vector<Span> got(sub.size());
  std::vector<std::vector<uint8_t>> host_decoded(sub.size());
  std::vector<uint8_t*> dst(sub.size(), nullptr);
  std::vector<std::exception_ptr> errs(sub.size());
  for (size_t k = 0; k < sub.size(); ++k)
    if (fetch_codec_ == Codec::kNone)
      dst[k] = fill_mem_->alloc((size_t)std::max<int64_t>(ready[sub[k]]->part_len(), 1));
  // drains > 0: that many drain threads take the MOFs in turn, so partitions complete one after
  // another and their H2D overlaps the rest of the fetch (all at once, they complete together)
  std::atomic<size_t> next_k{0};
  auto drain = [&](size_t k) {
    const int64_t td = trace::host_enabled() ? trace::now_ns() : 0;
    try {
      MofFetcher& f = *ready[sub[k]];
      if (dst[k]) {
        // first chunk from the fetcher, the rest straight into the pinned span
        // With early staging the partition is copied to HBM once complete, or (stage_step > 0)
        // every stage_step bytes of its landed prefix while the rest is still in flight.
        const int64_t cap = f.part_len();
        uint8_t* dev = stager ? stager->reserve(cap) : nullptr;
        int64_t off = f.take_first(dst[k], cap);
        if (dev && stage_step > 0) stager->copy(dst[k], dev, off);
        if (off < cap) {
          std::function<void(int64_t, int64_t)> on_prefix;
          if (dev && stage_step > 0)
            on_prefix = [&, k, dev](int64_t a, int64_t b) { stager->copy(dst[k] + a, dev + a, b - a); };
          off = t_.fetch_direct(f.params(), dst[k], off, cap, depth_, on_prefix, stage_step);
        }
        if (dev && stage_step <= 0) stager->copy(dst[k], dev, off);
        // an uncompressed partition's IFile checksum trailer stays behind its span (in pinned memory and in
        // the staged copy); a compressed one's is found by the framing walk of the merge that decodes it
        const int tail = stage_codec_ == Codec::kNone ? ifile_trailer_bytes(f.raw_len(), off) : 0;
        if (tail) ++trailers_;
        got[k] = Span{dst[k], off - tail, dev, tail, f.raw_len()};
        if (index_now) sub_idx[k] = index_partition(dst[k], off - tail);
      } else {  // host decode: decoded length unknown up front
        std::vector<uint8_t> buf((size_t)t_.buffer_size_);
        for (int64_t n; (n = f.pull(buf.data(), (int64_t)buf.size())) > 0;)
          host_decoded[k].insert(host_decoded[k].end(), buf.begin(), buf.begin() + n);
      }
    } catch (...) {
      errs[k] = std::current_exception();
    }
    if (td) trace::host_event("drain", (int64_t)k, got[k].len, td, trace::now_ns());
  };
  std::vector<std::thread> ts;
  const size_t nthreads = drains_ > 0 ? std::min<size_t>((size_t)drains_, sub.size()) : sub.size();
  for (size_t w = 0; w < nthreads; ++w)
    ts.emplace_back([&] {
      for (size_t k; (k = next_k++) < sub.size();) drain(k);
    });
  for (auto& t : ts) t.join();
  for (auto& e : errs)
    if (e) std::rethrow_exception(e);
  for (size_t k = 0; k < sub.size(); ++k) {
    if (!dst[k]) {
      uint8_t* p = fill_mem_->alloc(std::max<size_t>(host_decoded[k].size(), 1));
      std::memcpy(p, host_decoded[k].data(), host_decoded[k].size());
      got[k] = Span{p, (int64_t)host_decoded[k].size()};
    }
    got[k].id = span_id(ready[sub[k]]->params().map_id);
    group_.push_back(got[k]);
    if (index_now) direct_runs_.push_back(std::move(sub_idx[k]));
    if (ckpt_) group_ids_.push_back(ready[sub[k]]->params().map_id);
    drained_++;
    t_.note_map_fetched();
  }
}

void StagedMerge::index_spans(const std::vector<Span>& spans, size_t first, std::vector<SpillRun>* out) const {
  const size_t n = spans.size() - first;
  out->resize(n);
  std::atomic<size_t> nk{0};
  std::vector<std::exception_ptr> errs(n);
  std::vector<std::thread> ts;
  // half the drain threads: this runs beside them (and the provider's) under the task's CPU share
  const size_t nt = std::min<size_t>(n, (size_t)std::max<int64_t>(1, (drains_ > 0 ? drains_ : 8) / 2));
  for (size_t w = 0; w < nt; ++w)
    ts.emplace_back([&] {
      for (size_t k; (k = nk++) < n;) try {
          (*out)[k] = index_partition(const_cast<uint8_t*>(spans[first + k].p), spans[first + k].len);
        } catch (...) {
          errs[k] = std::current_exception();
        }
    });
  for (auto& t : ts) t.join();
  for (auto& e : errs)
    if (e) std::rethrow_exception(e);
}

// The group overflowed the budget: an LPQ merge, or the switch to direct RPQ (partitions drained so
// far are indexed here, later ones by their drain threads; early staging to HBM stops).
void StagedMerge::overflow() {
  if (!direct_ok_) {
    spill_group();
    return;
  }
  if (direct_) return;
  direct_ = true;
  if (stager_) {
    stager_->release_blocks();  // the partitions' HBM copies are not used: RPQ rounds copy their slices
    stager_ = nullptr;
  }
  // indexed beside the fetch (which goes on filling `group_`; the spans indexed here are a copy)
  direct_head_ = std::async(std::launch::async, [this, head = group_] {
    std::vector<SpillRun> idx;
    index_spans(head, 0, &idx);
    return idx;
  });
  std::lock_guard<std::mutex> g(t_.st_mu_);
  t_.st_.hybrid_direct = 1;
}

void StagedMerge::lpq_wait() {
  if (lpq_thr_.joinable()) lpq_thr_.join();
  if (lpq_err_) {
    std::exception_ptr e = lpq_err_;
    lpq_err_ = nullptr;
    std::rethrow_exception(e);
  }
}

void StagedMerge::spill_group() {
  if (group_.empty()) return;
  lpq_wait();               // one LPQ merge at a time (device workspace, stream s_)
  job_mem_->release_all();  // the previous LPQ's inputs are merged
  std::swap(fill_mem_, job_mem_);
  if (stager_ && !job_stager_) {  // first LPQ: the second stager (online merges never need one)
    stager_lease2_.obj = pooled_stager(device_);
    job_stager_ = stager_lease2_.obj.get();
    job_stager_->reset();
  }
  std::swap(stager_, job_stager_);  // the group's staged copies go with it; the next group stages into the other
  std::vector<Span> jg;
  jg.swap(group_);
  std::vector<std::string> ids;
  ids.swap(group_ids_);
  group_raw_ = 0;
  EarlyStager* st = job_stager_;
  lpq_thr_ = std::thread([this, st, jg = std::move(jg), ids = std::move(ids)]() mutable {
    try {
      if (hipSetDevice(device_) != hipSuccess) throw UdaError("hipSetDevice failed");
      merge_spill(std::move(jg), std::move(ids), st);
    } catch (...) {
      lpq_err_ = std::current_exception();
    }
  });
}

void StagedMerge::count_decoded(const DeviceMergeOut& m) {
  std::lock_guard<std::mutex> g(t_.st_mu_);
  t_.st_.device_decoded_blocks += m.decoded_blocks;
  t_.st_.device_decoded_streams += m.decoded_streams;
}

// trailers a device merge stripped from its runs (compressed runs: found by its framing walk; uncompressed
// ones were counted when their spans were made) and those it verified
void StagedMerge::count_checksums(const DeviceMergeOut& m) {
  if (stage_codec_ != Codec::kNone) trailers_ += m.trailers;
  if (m.checksum_parts > 0) {
    verified_ += m.checksum_parts;
    t_.note_checksum(m.checksum_parts, m.checksum_bytes, m.checksum_ms);
  }
}

int StagedMerge::span_id(const std::string& map_id) {
  map_ids_.push_back(map_id);
  return (int)map_ids_.size() - 1;
}

// LPQ: merge one group on the device and spill it with its sparse index. Runs on the LPQ thread,
// one group at a time, while the fetch fills the next group (the reference's fetcher running ahead
// of the LPQ merges, MergeManager.cc:202-288).
void StagedMerge::merge_spill(std::vector<Span> jg, std::vector<std::string> ids, EarlyStager* st) {
  DeviceWorkspace& ws = *ws_;
  hipStream_t s = s_;
  const int64_t tl = trace::host_enabled() ? trace::now_ns() : 0;
  if (st) st->flush();
  const int64_t tm = tl ? trace::now_ns() : 0;
  // under lpq_combine_ the spill holds one record per key of its group (the RPQ rounds combine again:
  // wrapping sums are associative, so the delivered bits do not depend on the grouping)
  DeviceMergeOut m;
  try {
    m = device_merge(ws, jg, stage_codec_, t_.kind_, lpq_spacing(), s, nullptr, false, lpq_combine_, 256ll << 20,
                     &lpq_ck_);
  } catch (const std::runtime_error& e) {
    // the merge's cuts are the index samples, and a cut spacing bounds the record size: a record longer than
    // the finer spacing of a combined spill takes the usual one
    if (lpq_spacing() == kSampleSpacing || !std::strstr(e.what(), "record larger than the delivery buffer")) throw;
    m = device_merge(ws, jg, stage_codec_, t_.kind_, kSampleSpacing, s, nullptr, false, lpq_combine_, 256ll << 20,
                     &lpq_ck_);
  }
  count_checksums(m);
  if (lpq_combine_ != CombineOp::kNone) combine_in_ += m.records_in;
  if (tl) {
    trace::host_event("lpq_flush", (int64_t)jg.size(), 0, tl, tm);
    trace::host_event("lpq_merge", m.bytes, (int64_t)jg.size(), tm, trace::now_ns());
  }
  count_decoded(m);
  if (st) st->reset();  // the merge read the staged copies; recycle their HBM
  SpillRun run;
  run.bytes = m.bytes;
  const bool disk = tier_ == "disk";
  if (disk) {
    if (!aio_) aio_ = AsyncIO::create(AsyncIO::Options{});
    char name[64];
    snprintf(name, sizeof(name), ".gpu-lpq-%03d", (int)spills_.size());
    run.path = dirs_[spills_.size() % dirs_.size()] + "/uda." + t_.init_.reduce_task_id + name;
    run.fd = create_private_file(run.path, O_RDWR);
    if (run.fd < 0) throw UdaError("cannot create spill file " + run.path + ": " + strerror(errno));
  } else {
    run.mem = spill_mem_.alloc((size_t)std::max<int64_t>(run.bytes, 1));
  }
  // stream the LPQ output out of HBM: sparse index from every cut, bytes to DRAM or to the file.
  // The DRAM tier is pinned, so the LPQ lands there by one DMA (no bounce through the ring).
  std::atomic<int64_t> err{0};
  if (!disk) {
    const auto td = std::chrono::steady_clock::now();
    const int64_t tt = trace::host_enabled() ? trace::now_ns() : 0;
    // on the SDMA delivery engine (idle until the RPQ rounds deliver), not a blit kernel on the CUs
    // the next LPQ merge needs; device_merge returned with `s` drained
    gpu::SdmaEngine* eng = nullptr;
    if (m.bytes > 0) {
      try {
        eng = &gpu::SdmaEngine::for_device(device_);
      } catch (const std::exception&) {
        eng = nullptr;
      }
    }
    if (eng) {
      if (!ws.h2d_sig.handle) ws.h2d_sig = eng->make_signal();
      gpu::SdmaEngine::arm(ws.h2d_sig, eng->parts((size_t)m.bytes, 1));
      eng->copy_d2h(run.mem, ws.out.as<uint8_t>(), (size_t)m.bytes, ws.h2d_sig, 1);
      gpu::SdmaEngine::wait(ws.h2d_sig);
    } else if (m.bytes > 0) {
      HIP_CHECK(hipMemcpyAsync(run.mem, ws.out.as<uint8_t>(), (size_t)m.bytes, hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
    if (tt) trace::host_event("lpq_d2h", m.bytes, 0, tt, trace::now_ns());
    ws.d2h_ms += ms_since(td);
    for (size_t j = 0; j + 1 < m.cuts.size(); ++j) {
      run.cut.push_back(m.cuts[j]);
      run.key.push_back(key_at(run.mem + m.cuts[j], m.cuts[j + 1] - m.cuts[j]));
    }
  } else
  stream_out(ws, m, s, [&](const uint8_t* p, size_t c0, size_t c1) {
    const int64_t base = m.cuts[c0], len = m.cuts[c1] - base;
    for (size_t j = c0; j < c1; ++j) {
      run.cut.push_back(m.cuts[j]);
      run.key.push_back(key_at(p + (m.cuts[j] - base), m.cuts[c1] - m.cuts[j]));
    }
    if (disk) {
      constexpr int64_t kIo = 8 << 20;
      for (int64_t o = 0; o < len; o += kIo)
        aio_->write(run.fd, base + o, std::min(kIo, len - o), p + o, [&err](int64_t r) {
          if (r < 0) err = r;
        });
      aio_->drain();  // the pinned piece is reused after this returns
    } else {
      std::memcpy(run.mem + base, p, (size_t)len);
    }
  });
  if (err.load() < 0) throw UdaError("spill write failed: " + std::string(strerror((int)-err.load())));
  {
    std::lock_guard<std::mutex> g(t_.st_mu_);
    t_.st_.lpqs++;
    t_.st_.spill_bytes += run.bytes;
  }
  const std::string run_path = run.path;
  const int run_fd = run.fd;
  std::vector<int64_t> idx_cut = ckpt_ ? run.cut : std::vector<int64_t>();
  std::vector<std::string> idx_key = ckpt_ ? run.key : std::vector<std::string>();
  const int64_t run_bytes = run.bytes;
  spills_.push_back(std::move(run));
  if (ckpt_ && disk) {
    // durable before listed: data, then the sparse index, then the manifest line
    if (::fsync(run_fd) != 0) throw UdaError("spill fsync failed");
    write_lpq_index(run_path + ".idx", idx_cut, idx_key);
    std::string line = "glpq " + std::to_string(spills_.size() - 1) + " " + std::to_string(run_bytes) + " " + run_path + " ";
    for (size_t j = 0; j < ids.size(); ++j) line += (j ? "," : "") + ids[j];
    if (!append_owned_line(manifest_, line)) throw UdaError("cannot append to LPQ manifest " + manifest_);
    checkpointed_ = spills_.size();
    if (fault_hit("LPQ_DONE")) throw UdaError("injected failure after an LPQ spill");
  }
}

// ------------------------------------------------------------------------------------- delivery
void StagedMerge::deliver(const DeviceMergeOut& m, bool last, hipStream_t ds, DeviceWorkspace& w) {
  const size_t nb = m.cuts.size() < 2 ? 0 : m.cuts.size() - 1;
  stream_out(w, m, ds, [&](const uint8_t* piece, size_t c0, size_t c1) {
    for (size_t j = c0; j < c1; ++j) {
      if (t_.stop_) throw UdaError("reduce task stopped during merge");
      const int64_t b = m.cuts[j], e = m.cuts[j + 1];
      const bool final_buf = last && j + 1 == nb;
      const uint8_t* p = piece + (b - m.cuts[c0]);
      int64_t len = e - b;
      if (final_buf) {  // copy so the EOF marker can follow the records
        std::memcpy(tail_.data(), p, (size_t)len);
        tail_[(size_t)len] = 0xFF;
        tail_[(size_t)len + 1] = 0xFF;
        p = tail_.data();
        len += kEofBytes;
        eof_sent_ = true;
      }
      if (t_.host_->data_from_uda(p, (int32_t)len) != 0) throw UdaError("dataFromUda callback failed");
      std::lock_guard<std::mutex> g(t_.st_mu_);
      t_.st_.buffers++;
      t_.st_.bytes_delivered += len;
    }
  });
  std::lock_guard<std::mutex> g(t_.st_mu_);
  t_.st_.records += m.records;
}

// rounds of a device merge's output go out on the copy stream while the next round merges
gpu::GenericMerger::RoundFn StagedMerge::round_sink(bool last_phase) {
  return [this, last_phase](const std::vector<int64_t>& cuts, int64_t records, bool last) {
    DeviceMergeOut r;
    r.cuts = cuts;
    r.records = records;
    {
      std::lock_guard<std::mutex> g(t_.st_mu_);
      t_.st_.merge_rounds++;
    }
    deliver(r, last && last_phase, ws_->copy_stream(), *ws_);
  };
}

// ---------------------------------------------------------------------------------------- modes
void StagedMerge::open_pipeline(RpqPipeline* pipe) {
  ws2_lease_.obj = pooled_workspace(device_);
  ws2_ = ws2_lease_.obj.get();
  ws2_->reset_stats();
  ws3_lease_.obj = pooled_workspace(device_);
  ws3_ = ws3_lease_.obj.get();
  ws3_->reset_stats();
  pipe->sg2.s = gpu::pooled_stream();
  pipe->sg3.s = gpu::pooled_stream();
  pipe->ws[0] = ws_;
  pipe->ws[1] = ws2_;
  pipe->ws[2] = ws3_;
  pipe->s[0] = s_;
  pipe->s[1] = pipe->sg2.s;
  pipe->s[2] = pipe->sg3.s;
}

// Round `rr` has merged (m: its slice states), and is not delivered yet: fold every open run's slice and
// close the runs whose records are all in (fin[k]: the run's final length in records' bytes, -1 while it is
// not known; last: no round follows). A mismatch throws here, so the round it is found in is not delivered;
// earlier key ranges are. landed(k): called before run k's trailer is read.
void StagedMerge::fold_slices(const RoundSlices& rr, const DeviceMergeOut& m, const std::vector<uint8_t*>& mems,
                              const std::vector<int64_t>& fin, bool last, const std::function<void(size_t)>& landed) {
  const size_t K = slice_sums_.size();
  if (rr.size() != K || m.slice_crc.size() != K || mems.size() != K || fin.size() != K)
    throw UdaError("RPQ round of " + std::to_string(rr.size()) + " slices with " + std::to_string(m.slice_crc.size()) +
                   " checksum states for " + std::to_string(K) + " runs");
  slice_ms_ += m.checksum_ms;
  int64_t parts = 0, bytes = 0;
  for (size_t k = 0; k < K; ++k) {
    if (!slice_sums_.open(k)) continue;
    slice_sums_.fold(k, mems[k], rr[k].first, rr[k].second, m.slice_crc[k]);
    if (!last && (fin[k] < 0 || slice_sums_.folded(k) < fin[k])) continue;
    if (landed) landed(k);
    bytes += slice_sums_.close(k, mems[k]);
    ++parts;
  }
  if (parts > 0) {
    verified_ += parts;
    t_.note_checksum(parts, bytes, slice_ms_);
    slice_ms_ = 0;
  }
}

// plan the rounds of every key range that has fully arrived; false while nothing new can be planned
bool StagedMerge::plan_more(DirectPlan& pl, bool wait) {
  DirectProg& dp = *dprog_;
  const int K = dp.K;
  std::unique_lock<std::mutex> lk(dp.mu);
  auto ready_epoch = [&] { return pl.epoch < dp.P && dp.phase_runs[(size_t)pl.epoch] == K; };
  if (wait)
    while (!dp.cv.wait_for(lk, std::chrono::milliseconds(50), [&] { return ready_epoch() || dp.err || t_.stop_; })) {
    }
  if (dp.err) std::rethrow_exception(dp.err);
  if (t_.stop_) throw UdaError("reduce task stopped during fetch");
  if (!ready_epoch()) return false;
  while (ready_epoch()) ++pl.epoch;  // take every phase indexed by now
  bool all_eof = true, blocked = false;
  std::string bound;
  bool have_bound = false;
  for (int k = 0; k < K; ++k) {
    SpillRun& r = pl.runs[(size_t)k];
    r.mem = dp.dst[(size_t)k];  // indexed through a phase: its span exists
    auto& vc = dp.cut[(size_t)k];
    auto& vk = dp.key[(size_t)k];
    for (size_t j = pl.taken[(size_t)k]; j < vc.size(); ++j) {
      r.cut.push_back(vc[j]);
      r.key.push_back(vk[j]);
    }
    pl.taken[(size_t)k] = vc.size();
    r.bytes = dp.complete[(size_t)k];
    if (dp.eof[(size_t)k]) {
      pl.eof[(size_t)k] = 1;
      continue;
    }
    all_eof = false;
    if (dp.last_key[(size_t)k].empty()) {
      blocked = true;  // no complete record of this run yet: nothing below any bound is known
      continue;
    }
    if (!have_bound || cmp_key(t_.kind_, dp.last_key[(size_t)k], bound) < 0) {
      bound = dp.last_key[(size_t)k];
      have_bound = true;
    }
  }
  lk.unlock();
  if (!all_eof && (blocked || !have_bound)) return true;  // wait for more phases
  std::vector<int64_t> end((size_t)K);
  for (int k = 0; k < K; ++k)
    end[(size_t)k] = all_eof ? pl.runs[(size_t)k].bytes
                             : std::max(pl.at[(size_t)k], boundary(pl.runs[(size_t)k], bound, t_.kind_));
  // splitters every ~budget/2 bytes of the range (samples inside it, by key)
  const std::vector<std::string> split = plan_splitters(pl.runs, pl.at, end, pl.target, t_.kind_);
  std::vector<std::vector<int64_t>> bnd((size_t)K);
  for (int k = 0; k < K; ++k)
    for (const auto& kk : split) bnd[(size_t)k].push_back(boundary(pl.runs[(size_t)k], kk, t_.kind_));
  for (auto& rr : slice_rounds(bnd, pl.at, end, true, all_eof)) pl.rounds.push_back(std::move(rr));
  pl.at = end;
  if (all_eof) pl.planned_all = true;
  return true;
}

void StagedMerge::run_progressive_direct() {
  combine_skipped_ = t_.combine_ != CombineOp::kNone && hybrid_combine_ == CombineOp::kNone;
  DirectProg& dp = *dprog_;
  const int K = dp.K;
  DirectPlan pl;
  pl.runs.resize((size_t)K);
  pl.at.assign((size_t)K, 0);
  pl.taken.assign((size_t)K, 0);
  pl.eof.assign((size_t)K, 0);
  pl.target = std::max<int64_t>(round_target(), dp.spacing);
  // three workspaces, two rounds prepared ahead (as the direct RPQ of run_hybrid)
  RpqPipeline pipe;
  open_pipeline(&pipe);
  const ChecksumPolicy* const slice_ck = slice_sums_.any() ? &slice_ck_ : nullptr;
  // a round's slices by value: `rounds` grows (and reallocates) on this thread while earlier rounds merge
  auto prep = [&](size_t q, RoundSlices rr, std::vector<uint8_t*> mems) {
    if (hipSetDevice(device_) != hipSuccess) throw UdaError("hipSetDevice failed");
    std::vector<Span> views((size_t)K);
    for (int k = 0; k < K; ++k)
      views[(size_t)k] = Span{mems[(size_t)k] + rr[(size_t)k].first, rr[(size_t)k].second - rr[(size_t)k].first};
    return device_merge(*pipe.ws[q % 3], views, Codec::kNone, t_.kind_, kv_, pipe.s[q % 3], nullptr, true,
                        hybrid_combine_, 256ll << 20, slice_ck);
  };
  // a run's trailer may lie in a later phase than its EOF marker: it is compared once every phase is in
  auto landed = [&](size_t k) {
    std::unique_lock<std::mutex> lk(dp.mu);
    while (!dp.cv.wait_for(lk, std::chrono::milliseconds(50),
                           [&] { return dp.indexed[k] == dp.P || dp.err || t_.stop_; })) {
    }
    if (dp.err) std::rethrow_exception(dp.err);
    if (t_.stop_) throw UdaError("reduce task stopped during fetch");
  };
  std::vector<int64_t> fin((size_t)K);
  std::vector<std::future<DeviceMergeOut>> next;
  // at most three rounds in flight (one delivering, two preparing): workspace q % 3 is free again
  // once round q - 3 has been delivered
  auto issue = [&](size_t q) {
    while (next.size() < pl.rounds.size() && next.size() < q + 3) {
      std::vector<uint8_t*> mems((size_t)K);
      for (int k = 0; k < K; ++k) mems[(size_t)k] = pl.runs[(size_t)k].mem;
      next.push_back(std::async(std::launch::async, prep, next.size(), pl.rounds[next.size()], std::move(mems)));
    }
  };
  size_t q = 0;
  while (!pl.planned_all || q < pl.rounds.size()) {
    // plan what has arrived (wait only when nothing is queued)
    while (!pl.planned_all && (q + 2 >= pl.rounds.size())) {
      const size_t before = pl.rounds.size();
      if (!plan_more(pl, q >= pl.rounds.size())) break;
      if (pl.rounds.size() == before && q < pl.rounds.size()) break;
    }
    issue(q);
    if (q >= pl.rounds.size()) continue;
    DeviceMergeOut m = next[q].get();
    if (hybrid_combine_ != CombineOp::kNone) combine_in_ += m.records_in;
    issue(q);
    const bool last = pl.planned_all && q + 1 == pl.rounds.size();
    if (slice_ck) {
      std::vector<uint8_t*> mems((size_t)K);
      for (int k = 0; k < K; ++k) {
        mems[(size_t)k] = pl.runs[(size_t)k].mem;
        fin[(size_t)k] = pl.eof[(size_t)k] ? pl.runs[(size_t)k].bytes : -1;
      }
      fold_slices(pl.rounds[q], m, mems, fin, last, landed);
    }
    deliver(m, last, pipe.s[q % 3], *pipe.ws[q % 3]);
    ++q;
  }
  for (auto& t : dp.threads) t.join();
  prog_fetch_ms_ = std::chrono::duration<double, std::milli>(dp.t_end - t0_).count();
  {
    std::lock_guard<std::mutex> g(t_.st_mu_);
    t_.st_.rpq_rounds = (int64_t)pl.rounds.size();
  }
  for (int k = 0; k < K; ++k) t_.note_map_fetched();
}

void StagedMerge::run_progressive() {
  ProgFetch& pf = *prog_;
  DeviceWorkspace& ws = *ws_;
  const int K = pf.K;
  std::vector<int64_t> start((size_t)K, 0), land((size_t)K, 0);
  for (int p = 0; p < pf.P; ++p) {
    const auto tw = std::chrono::steady_clock::now();
    {
      std::unique_lock<std::mutex> lk(pf.mu);
      // exit() sets stop_ without notifying pf.cv: wake up to look
      while (!pf.cv.wait_for(lk, std::chrono::milliseconds(50),
                             [&] { return pf.done[(size_t)p] == K || pf.err || t_.stop_; })) {
      }
      if (pf.err) std::rethrow_exception(pf.err);
      if (t_.stop_) throw UdaError("reduce task stopped during fetch");
      for (int k = 0; k < K; ++k) land[(size_t)k] = std::max(land[(size_t)k], pf.landed[(size_t)p][(size_t)k]);
    }
    stager_->flush_group(p);
    ws.h2d_ms += ms_since(tw);
    const bool last_phase = p + 1 == pf.P;
    std::vector<Span> spans((size_t)K);
    if (!last_phase) {
      std::vector<const uint8_t*> win((size_t)K);
      std::vector<int64_t> avail((size_t)K);
      std::vector<char> fin((size_t)K);
      for (int k = 0; k < K; ++k) {
        win[(size_t)k] = pf.dev[(size_t)k] + start[(size_t)k];
        avail[(size_t)k] = std::min(land[(size_t)k], pf.body[(size_t)k]) - start[(size_t)k];  // (never the trailer)
        fin[(size_t)k] = land[(size_t)k] >= pf.cap[(size_t)k];
      }
      const auto tp = std::chrono::steady_clock::now();
      const gpu::ProgressiveSplit sp = gpu::plan_progressive_split(win, avail, fin, (int)t_.kind_, ws.rounds, s_);
      ws.device_ms += ms_since(tp);
      int64_t take = 0;
      for (int k = 0; k < K; ++k) take += sp.split[(size_t)k];
      if (take == 0) continue;  // nothing complete below the bound yet: wait for the next phase
      for (int k = 0; k < K; ++k) {
        spans[(size_t)k] = Span{pf.dst[(size_t)k] + start[(size_t)k], sp.split[(size_t)k],
                                pf.dev[(size_t)k] + start[(size_t)k]};
        start[(size_t)k] += sp.split[(size_t)k];
      }
      {
        std::lock_guard<std::mutex> g(t_.st_mu_);
        t_.st_.rpq_rounds++;  // progressive phases merged
      }
    } else {
      prog_fetch_ms_ = std::chrono::duration<double, std::milli>(pf.t_end - t0_).count();
      for (int k = 0; k < K; ++k)
        spans[(size_t)k] = Span{pf.dst[(size_t)k] + start[(size_t)k], pf.body[(size_t)k] - start[(size_t)k],
                                pf.dev[(size_t)k] + start[(size_t)k]};
      // every partition lies whole in HBM now: their IFile checksums, before the last key range is merged
      // (earlier ranges are delivered already, as with any failure this late)
      std::vector<gpu::DeviceChecksum::Item> items;
      for (int k = 0; k < K && verify_ck_.verify; ++k)
        if (pf.body[(size_t)k] < pf.cap[(size_t)k])
          items.push_back(gpu::DeviceChecksum::Item{pf.dev[(size_t)k], pf.body[(size_t)k], map_ids_[(size_t)pf.id[(size_t)k]],
                                                    false, 0});
      if (!items.empty()) {
        ws.checksum.reset();
        ws.checksum.launch(std::move(items), s_);
        ws.checksum.finish(s_, false);
        verified_ += ws.checksum.partitions();
        t_.note_checksum(ws.checksum.partitions(), ws.checksum.bytes(), ws.checksum.ms());
        ws.checksum.reset();
      }
    }
    const DeviceMergeOut pm =
        device_merge(ws, spans, Codec::kNone, t_.kind_, kv_, s_, round_sink(last_phase), false, t_.combine_,
                     t_.merge_round_bytes_);
    combine_in_ += pm.records_in;
  }
  for (auto& t : pf.threads) t.join();
  for (int k = 0; k < K; ++k) t_.note_map_fetched();
}

// online: the whole reduce input in one device merge
void StagedMerge::run_online() {
  if (stager_) {
    const auto tf = std::chrono::steady_clock::now();
    stager_->flush();
    ws_->h2d_ms += ms_since(tf);
  }
  DeviceMergeOut m = device_merge(*ws_, group_, stage_codec_, t_.kind_, kv_, s_, round_sink(true), false, t_.combine_,
                                  t_.merge_round_bytes_, &verify_ck_);
  count_checksums(m);
  combine_in_ += m.records_in;
  count_decoded(m);
}

// read [off, off+len) of a spilled run into dst
void StagedMerge::read_run(const SpillRun& run, int64_t off, int64_t len, uint8_t* dst) {
  if (len <= 0) return;
  if (run.fd < 0) {
    std::memcpy(dst, run.mem + off, (size_t)len);
    return;
  }
  std::atomic<int64_t> err{0};
  constexpr int64_t kPiece = 8 << 20;
  for (int64_t o = 0; o < len; o += kPiece)
    aio_->read(run.fd, off + o, std::min(kPiece, len - o), dst + o, [&err](int64_t r) {
      if (r < 0) err = r;
    });
  aio_->drain();
  if (err.load() < 0) throw UdaError("spill read failed");
}

// bnd[r][i]: boundary of run r for splitter i (first record whose key >= the splitter)
std::vector<std::vector<int64_t>> StagedMerge::run_bounds(const std::vector<std::string>& split) {
  const int R = (int)spills_.size();
  std::vector<std::vector<int64_t>> bnd((size_t)R);
  const ReadWindow window = [this](const SpillRun& run, int64_t off, int64_t len, uint8_t* dst) {
    read_run(run, off, len, dst);
  };
  auto bounds_of = [&](int r) {
    for (auto& k : split) bnd[(size_t)r].push_back(boundary(spills_[(size_t)r], k, t_.kind_, window));
  };
  bool all_mem = true;
  for (const SpillRun& run : spills_) all_mem = all_mem && run.fd < 0;
  if (all_mem && R > 1) {  // in-place scans of DRAM runs, spread over threads (files share one AsyncIO)
    std::atomic<int> nr{0};
    std::vector<std::exception_ptr> errs((size_t)R);
    std::vector<std::thread> ts;
    for (int w = 0; w < std::min(R, 8); ++w)
      ts.emplace_back([&] {
        for (int r; (r = nr++) < R;) try {
            bounds_of(r);
          } catch (...) {
            errs[(size_t)r] = std::current_exception();
          }
      });
    for (auto& t : ts) t.join();
    for (auto& e : errs)
      if (e) std::rethrow_exception(e);
  } else {
    for (int r = 0; r < R; ++r) bounds_of(r);
  }
  return bnd;
}

// hybrid: last LPQ, then RPQ rounds over the spilled runs (direct: over the partitions)
void StagedMerge::run_hybrid() {
  combine_skipped_ = t_.combine_ != CombineOp::kNone && hybrid_combine_ == CombineOp::kNone;
  if (direct_) {
    spills_ = direct_head_.get();
    for (auto& r : direct_runs_) spills_.push_back(std::move(r));
  } else {
    spill_group();
    lpq_wait();
  }
  const int R = (int)spills_.size();
  if (direct_ && verify_over_) {  // spills_[r] is the index of group_[r]
    if (group_.size() != (size_t)R) throw UdaError("direct RPQ: " + std::to_string(R) + " runs indexed of " +
                                                   std::to_string(group_.size()) + " partitions");
    for (const Span& sp : group_)
      slice_sums_.add_run(sp.tail != 0, sp.len, sp.id >= 0 ? map_ids_[(size_t)sp.id] : std::string("?"));
  }
  const ChecksumPolicy* const slice_ck = slice_sums_.any() ? &slice_ck_ : nullptr;
  // splitters every ~budget/2 bytes of input (a sample stands for the bytes up to its run's next cut)
  std::vector<int64_t> at((size_t)R, 0), end((size_t)R);
  for (int r = 0; r < R; ++r) end[(size_t)r] = spills_[(size_t)r].bytes;
  int64_t target = std::max<int64_t>(round_target(), kSampleSpacing);
  if (!direct_ && lpq_combine_ != CombineOp::kNone) {
    // Combined spills can all fit one round of the budget. They are still planned in at least two key-range
    // rounds, so an over-budget task runs the RPQ the way uncombined spills (always larger than the budget)
    // make it run: several combining rounds through the pipeline. Measured (docs/BENCHMARKS.md), the extra
    // round does not pay for itself up to 100 MB of spills: it costs the launches and synchronizes of one
    // more device merge, so the minimum is two and not the pipeline's three workspaces.
    int64_t tot = 0;
    for (int r = 0; r < R; ++r) tot += end[(size_t)r];
    const char* mr = std::getenv("UDA_RPQ_MIN_ROUNDS");  // A/B: 1 plans them by the budget alone
    const int64_t min_rounds = mr && *mr ? std::max<int64_t>(1, std::atoll(mr)) : 2;
    target = std::min(target, std::max<int64_t>(lpq_spacing(), (tot + min_rounds - 1) / min_rounds));
  }
  const std::vector<std::string> split = plan_splitters(spills_, at, end, target, t_.kind_);
  const std::vector<RoundSlices> slices = slice_rounds(run_bounds(split), at, end, false, false);
  const int rounds = (int)split.size() + 1;
  {
    std::lock_guard<std::mutex> g(t_.st_mu_);
    t_.st_.rpq_rounds = rounds;
  }
  // RPQ rounds: each round's slices are read, copied to HBM and merged on a helper thread (its own
  // workspace and stream) while earlier rounds are delivered.
  RpqPipeline pipe;
  open_pipeline(&pipe);
  gpu::PinnedArena slice_mem[3];
  auto prep = [&](int q) {
    if (hipSetDevice(device_) != hipSuccess) throw UdaError("hipSetDevice failed");
    std::vector<Span> views;
    gpu::PinnedArena& sm = slice_mem[q % 3];
    sm.release_all();  // round q - 3's slices: copied to HBM before its merge returned
    for (int r = 0; r < R; ++r) {
      const SpillRun& run = spills_[(size_t)r];
      const int64_t b = slices[(size_t)q][(size_t)r].first, e = slices[(size_t)q][(size_t)r].second;
      if (run.fd < 0) {
        views.push_back(Span{run.mem + b, e - b});
      } else {
        uint8_t* p = sm.alloc((size_t)std::max<int64_t>(e - b, 1));
        read_run(run, b, e - b, p);
        views.push_back(Span{p, e - b});
      }
    }
    // views: pinned host spans (spill arena or slice arena): SDMA H2D, not a blit kernel
    return device_merge(*pipe.ws[q % 3], views, Codec::kNone, t_.kind_, kv_, pipe.s[q % 3], nullptr, true,
                        hybrid_combine_, 256ll << 20, slice_ck);
  };
  std::vector<uint8_t*> mems;
  for (int r = 0; r < R && slice_ck; ++r) mems.push_back(spills_[(size_t)r].mem);
  std::vector<std::future<DeviceMergeOut>> next((size_t)rounds);
  for (int q = 0; q < std::min(rounds, 2); ++q) next[(size_t)q] = std::async(std::launch::async, prep, q);
  for (int q = 0; q < rounds; ++q) {
    DeviceMergeOut m = next[(size_t)q].get();
    // records enter a combining merge once: at the LPQ level when it combines, else here
    if (hybrid_combine_ != CombineOp::kNone && (direct_ || lpq_combine_ == CombineOp::kNone))
      combine_in_ += m.records_in;
    // workspace (q + 2) % 3 delivered round q - 1 before this iteration
    if (q + 2 < rounds) next[(size_t)q + 2] = std::async(std::launch::async, prep, q + 2);
    if (slice_ck) fold_slices(slices[(size_t)q], m, mems, end, q + 1 == rounds, nullptr);
    const int64_t td = trace::host_enabled() ? trace::now_ns() : 0;
    deliver(m, q + 1 == rounds, pipe.s[q % 3], *pipe.ws[q % 3]);
    if (td) trace::host_event("rpq_deliver", m.bytes, q, td, trace::now_ns());
  }
}

// ------------------------------------------------------------------------------------------ end
void StagedMerge::cleanup(bool ok) {
  for (size_t i = 0; i < spills_.size(); ++i) {
    SpillRun& r = spills_[i];
    if (r.fd >= 0) ::close(r.fd);
    const bool keep = !ok && ckpt_ && i < checkpointed_;
    if (!r.path.empty() && !keep) {
      ::unlink(r.path.c_str());
      if (ckpt_) ::unlink((r.path + ".idx").c_str());
    }
    r.fd = -1;
    r.path.clear();
  }
  if (ok && ckpt_) ::unlink(manifest_.c_str());
}

void StagedMerge::finish() {
  DeviceWorkspace& ws = *ws_;
  DeviceWorkspace* ws2 = ws2_;
  DeviceWorkspace* ws3 = ws3_;
  ReduceStats& st_ = t_.st_;
  cleanup(true);
  HIP_CHECK(hipStreamSynchronize(s_));
  ws_lease_.clean = true;
  ws2_lease_.clean = true;
  ws3_lease_.clean = true;
  stager_lease_.clean = true;
  stager_lease2_.clean = true;
  if (trailers_ > 0 && !verify_ck_.verify) t_.note_checksum(0, 0);  // stripped, mapred.uda.ifile.checksum=off
  std::lock_guard<std::mutex> g(t_.st_mu_);
  if (trailers_ > verified_ && verify_ck_.verify && st_.ifile_checksum != "verified")
    st_.ifile_checksum = "skipped-over-budget";  // (host-decoded partitions are verified as they are pulled)
  st_.gpu_checksum_ms += slice_ms_;  // (rounds after the last run closed)
  if (combine_skipped_) {
    st_.combine = "skipped-over-budget";
  } else if (t_.combine_ != CombineOp::kNone) {
    st_.combine_in_records = combine_in_;
    st_.combine_groups = st_.records;
  }
  st_.gpu_h2d_ms = ws.h2d_ms + (ws2 ? ws2->h2d_ms : 0) + (ws3 ? ws3->h2d_ms : 0);
  st_.gpu_device_ms = ws.device_ms + (ws2 ? ws2->device_ms : 0) + (ws3 ? ws3->device_ms : 0);
  st_.gpu_d2h_wait_ms = ws.d2h_ms + (ws2 ? ws2->d2h_ms : 0) + (ws3 ? ws3->d2h_ms : 0);
  st_.gpu_sink_ms = ws.sink_ms + (ws2 ? ws2->sink_ms : 0) + (ws3 ? ws3->sink_ms : 0);
  st_.fetch_ms = prog_fetch_ms_ >= 0 ? prog_fetch_ms_ : fetch_ms_;
  st_.merge_ms = ms_since(t0_) - st_.fetch_ms;
  if (trace::host_enabled()) {
    trace::host_event("task", stage_step_, drains_,
                      trace::now_ns() - (int64_t)((st_.merge_ms + fetch_ms_) * 1e6), trace::now_ns());
    trace::host_dump();
  }
}

}  // namespace uda
