// ShuffleJob: construction, the partition store and its generation, sampling, and plan() with the
// delivery threads' start. The plan's device work is in shuffle_job_plan.cc, the step in shuffle_step.cc,
// the delivery threads in shuffle_delivery.cc.
#include "device_engine.h"
#include "engine_util.h"
#include "sdma.h"
#include "uda/log.h"
#include "uda/thread_name.h"
#include "uda/topology.h"
#include "uda/vint.h"

#include <unistd.h>

#include <algorithm>
#include <stdexcept>

namespace uda {
namespace gpu {

// -------------------------------------------------------------------------------- ShuffleJob
ShuffleJob::ShuffleJob(const ShuffleConfig& cfg) : cfg_(cfg) {
  if (cfg_.world < 1 || cfg_.rank < 0 || cfg_.rank >= cfg_.world)
    throw std::runtime_error("ShuffleJob: bad rank/world");
  if (cfg_.maps_per_rank < 1) throw std::runtime_error("ShuffleJob: maps_per_rank < 1");
  if (cfg_.rounds < 1) cfg_.rounds = 1;
  if (cfg_.reducers < 1) cfg_.reducers = 1;
  if (cfg_.pinned_slots < 2) cfg_.pinned_slots = 2;
  if (cfg_.d2h != "sdma" && cfg_.d2h != "hip") throw std::runtime_error("ShuffleJob: d2h must be sdma or hip");
  if (cfg_.store != "hbm" && cfg_.store != "host" && cfg_.store != "disk")
    throw std::runtime_error("unknown store tier " + cfg_.store);
  const int version = delivery_pack_version(cfg_.delivery_pack);
  if (version < 0) throw std::runtime_error("ShuffleJob: delivery_pack must be auto, v1 or off");
  check_delivery_order(cfg_.delivery_order);
  pack_ = cfg_.deliver_host && version != 0;
  lay_ = fixed_layout(cfg_.kv_buf_bytes, cfg_.d2h_piece_bytes, cfg_.pinned_slots, pack_ ? version : 0);
  R_ = cfg_.reducers;
  Q_ = cfg_.rounds;
  C_ = R_ * Q_;
  geo_ = ShuffleGeometry{cfg_.world, R_, Q_, cfg_.maps_per_rank, cfg_.rank, kTeraRecordBytes};
  if ((int64_t)R_ * cfg_.world * cfg_.maps_per_rank > 65536)
    throw std::runtime_error("ShuffleJob: reducers * world * maps_per_rank must be <= 65536 (merge run index)");
  HIP_CHECK(hipSetDevice(cfg_.device));
  int lo_prio = 0, hi_prio = 0;
  HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio));
  // HBM store: the comm stream carries RCCL and gets the high priority. Spill tiers: it carries the
  // round's H2D staging (a copy kernel reading host memory), which must not hold back the merge of
  // the previous round: the merge stream gets the high priority instead.
  const bool spill = cfg_.store != "hbm";
  HIP_CHECK(hipStreamCreateWithPriority(&s_comm_, hipStreamNonBlocking, spill ? lo_prio : hi_prio));
  HIP_CHECK(hipStreamCreateWithPriority(&s_compute_, hipStreamNonBlocking, spill ? hi_prio : lo_prio));
  HIP_CHECK(hipStreamCreateWithFlags(&s_copy_, hipStreamNonBlocking));
  HIP_CHECK(hipStreamCreateWithFlags(&s_plan_, hipStreamNonBlocking));
  merged_ev_.resize(kSlots);
  comm_ev_.resize(kSlots);
  sent_ev_.resize(2);
  early_ev_.resize(kSlots);
  for (auto& e : early_ev_) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (auto& e : merged_ev_) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (auto& e : comm_ev_) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (auto& e : sent_ev_) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
}

ShuffleJob::~ShuffleJob() {
  {
    std::lock_guard<std::mutex> g(mu_);
    stop_ = true;
  }
  cv_.notify_all();
  if (copy_thr_.joinable()) copy_thr_.join();
  for (auto& t : consumers_)
    if (t.joinable()) t.join();
  (void)hipDeviceSynchronize();
  for (auto e : merged_ev_) (void)hipEventDestroy(e);
  for (auto e : early_ev_) (void)hipEventDestroy(e);
  if (s_stage_) (void)hipStreamDestroy(s_stage_);
  for (auto e : comm_ev_) (void)hipEventDestroy(e);
  for (auto e : sent_ev_) (void)hipEventDestroy(e);
  for (auto e : piece_ev_) (void)hipEventDestroy(e);
  if (!sdma_ && ring_) pinned_host_free(ring_);
  if (sdma_) {
    for (auto sg : piece_sig_) sdma_->destroy_signal(sg);
    sdma_->free_host(ring_);
    ring_ = nullptr;
    sdma_.reset();
  }
  exchange_.reset();
  if (s_copy_) (void)hipStreamDestroy(s_copy_);
  if (s_plan_) (void)hipStreamDestroy(s_plan_);
  if (s_comm_) (void)hipStreamDestroy(s_comm_);
  if (s_compute_) (void)hipStreamDestroy(s_compute_);
}

void ShuffleJob::init_comm(const std::string& uid) {
  if (cfg_.world == 1) return;
  HIP_CHECK(hipSetDevice(cfg_.device));
  exchange_ = make_rccl_exchange(cfg_.rank, cfg_.world, uid);
}

void ShuffleJob::init_local() {
  if (cfg_.world == 1) return;
  if (cfg_.local_group.empty()) throw std::runtime_error("init_local: config.local_group is empty");
  HIP_CHECK(hipSetDevice(cfg_.device));
  exchange_ = make_local_exchange(cfg_.local_group, cfg_.rank, cfg_.world);
}

void ShuffleJob::init_ipc(const std::string& name) {
  if (cfg_.world == 1) return;
  HIP_CHECK(hipSetDevice(cfg_.device));
  exchange_ = make_ipc_exchange(name, cfg_.rank, cfg_.world, cfg_.device);
}

// The store's layout (every run 16-byte aligned behind its predecessor's EOF marker, every MOF 256-byte
// aligned) and its memory or files.
void ShuffleJob::alloc_store() {
  const int M = cfg_.maps_per_rank, W = cfg_.world;
  const int nruns = M * W;
  run_off_.assign(nruns, 0);
  run_nrec_.assign(nruns, 0);
  mof_off_.assign(M + 1, 0);
  int64_t off = 0;
  for (int m = 0; m < M; ++m) {
    mof_off_[m] = off;
    for (int d = 0; d < W; ++d) {
      const int64_t n = cfg_.records_per_map / W + (d < cfg_.records_per_map % W ? 1 : 0);
      run_nrec_[m * W + d] = n;
      run_off_[m * W + d] = off;
      off = align_up(off + n * kTeraRecordBytes + kEofBytes, 16);
    }
    off = align_up(off, 256);
  }
  mof_off_[M] = off;
  store_bytes_ = off;
  if (disk_store()) {
    std::vector<std::string> dirs;
    for (size_t b = 0; b <= cfg_.local_dirs.size();) {
      const size_t e = cfg_.local_dirs.find(',', b);
      const std::string d = cfg_.local_dirs.substr(b, e == std::string::npos ? std::string::npos : e - b);
      if (!d.empty()) dirs.push_back(d);
      if (e == std::string::npos) break;
      b = e + 1;
    }
    disk_.reset(new DiskStore(cfg_.device, dirs, std::to_string(getpid()) + "." + std::to_string(cfg_.rank), M));
    store_base_ = store_dev_base_ = nullptr;
  } else if (host_store()) {
    hstore_.alloc((size_t)store_bytes_);
    store_base_ = hstore_.as<uint8_t>();
    void* dp = nullptr;
    HIP_CHECK(hipHostGetDevicePointer(&dp, store_base_, 0));
    store_dev_base_ = reinterpret_cast<uint8_t*>(dp);
  } else {
    store_.alloc((size_t)store_bytes_, /*resident=*/true);  // padded for hipIpc export by DeviceBuffer::alloc
    store_base_ = store_dev_base_ = store_.as<uint8_t>();
  }
}

void ShuffleJob::generate() {
  HIP_CHECK(hipSetDevice(cfg_.device));
  const int M = cfg_.maps_per_rank, W = cfg_.world;
  const int nruns = M * W;
  alloc_store();

  std::vector<uint8_t*> bases(nruns), gen_bases(nruns);
  std::vector<uint64_t> key_lo(nruns), key_span(nruns), seeds(nruns);
  const uint64_t step = (W == 1) ? ~0ull : (~0ull / (uint64_t)W);
  int64_t max_n = 0, max_mof = 0;
  DeviceBuffer tmp;  // host/disk tier: one MOF at a time is generated in HBM, then copied out
  if (spilled()) {
    for (int m = 0; m < M; ++m) max_mof = std::max(max_mof, mof_off_[m + 1] - mof_off_[m]);
    tmp.alloc((size_t)max_mof);
  }
  for (int m = 0; m < M; ++m)
    for (int d = 0; d < W; ++d) {
      const int r = m * W + d;
      bases[r] = disk_store() ? nullptr : store_dev_base_ + run_off_[r];
      gen_bases[r] = spilled() ? tmp.as<uint8_t>() + (run_off_[r] - mof_off_[m]) : bases[r];
      key_lo[r] = step * (uint64_t)d;
      key_span[r] = step;
      const uint64_t gmap = (uint64_t)cfg_.rank * M + m;
      seeds[r] = cfg_.seed ^ (0x9E3779B97F4A7C15ull * (gmap + 1)) ^ (0xC2B2AE3D27D4EB4Full * (d + 1));
      max_n = std::max(max_n, run_nrec_[r]);
    }
  // sorted generation strides each run's keys over its span (kernels.h: key_span >= nrec); unsorted
  // generation draws them and the map-side sort orders them
  if (!cfg_.map_sort) require_teragen_spans(run_nrec_.data(), key_span.data(), nruns);
  DeviceBuffer d_b(nruns * sizeof(uint8_t*)), d_n(nruns * 8), d_lo(nruns * 8), d_sp(nruns * 8), d_sd(nruns * 8),
      d_ck(nruns * 8);
  HIP_CHECK(hipMemcpy(d_b.as(), gen_bases.data(), nruns * sizeof(uint8_t*), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(d_n.as(), run_nrec_.data(), nruns * 8, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(d_lo.as(), key_lo.data(), nruns * 8, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(d_sp.as(), key_span.data(), nruns * 8, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(d_sd.as(), seeds.data(), nruns * 8, hipMemcpyHostToDevice));
  // on the stream the generation kernels accumulate on: a hipMemset goes to the null stream, which a
  // non-blocking stream does not wait for, and it returns before the device ran it -- the kernels then
  // added onto stale bytes or were zeroed midway, and the job's expected checksums came out wrong
  // (the r5 multi-rank "checksum mismatch" with records, order and every slice correct)
  static const bool old_memset = [] {  // tools/multirank_stress.py --old-memset: the r5 code, to show the race
    const char* e = std::getenv("UDA_GEN_NULL_STREAM_MEMSET");
    return e && std::atoi(e) != 0;
  }();
  if (old_memset)
    HIP_CHECK(hipMemset(d_ck.as(), 0, nruns * 8));
  else
    HIP_CHECK(hipMemsetAsync(d_ck.as(), 0, nruns * 8, s_compute_));
  // cfg.map_sort: the map side's own work — each partition is generated unsorted into the sort
  // workspace and the device radix sort (F8) gathers it, sorted, into the store. The checksums are
  // order-independent.
  DeviceBuffer sort_ws, d_stage;
  hipEvent_t sort_t0 = nullptr, sort_t1 = nullptr;
  struct EvGuard {
    hipEvent_t* a;
    hipEvent_t* b;
    ~EvGuard() {
      if (*a) (void)hipEventDestroy(*a);
      if (*b) (void)hipEventDestroy(*b);
    }
  } ev_guard{&sort_t0, &sort_t1};
  if (cfg_.map_sort) {
    if (max_n >= (int64_t)UINT32_MAX) throw std::runtime_error("map_sort: a run has 2^32 or more records");
    sort_ws.alloc((size_t)sort_fixed_ws_bytes(max_n));
    uint8_t* recs = sort_fixed_ws_records(sort_ws.as(), max_n);
    d_stage.alloc(sizeof(uint8_t*));
    HIP_CHECK(hipMemcpy(d_stage.as(), &recs, sizeof(uint8_t*), hipMemcpyHostToDevice));
    HIP_CHECK(hipEventCreate(&sort_t0));
    HIP_CHECK(hipEventCreate(&sort_t1));
  }
  map_sort_ms_ = 0;
  auto gen_runs = [&](int r0, int r1) {  // generate runs [r0, r1) at gen_bases
    if (!cfg_.map_sort) {
      launch_teragen(d_b.as<uint8_t*>() + r0, d_n.as<int64_t>() + r0, d_lo.as<uint64_t>() + r0,
                     d_sp.as<uint64_t>() + r0, d_sd.as<uint64_t>() + r0, r1 - r0, max_n,
                     d_ck.as<unsigned long long>() + r0, s_compute_);
      HIP_CHECK(hipGetLastError());
      return;
    }
    for (int r = r0; r < r1; ++r) {
      if (run_nrec_[r] <= 0) continue;
      launch_teragen(d_stage.as<uint8_t*>(), d_n.as<int64_t>() + r, d_lo.as<uint64_t>() + r, d_sp.as<uint64_t>() + r,
                     d_sd.as<uint64_t>() + r, 1, run_nrec_[r], d_ck.as<unsigned long long>() + r, s_compute_,
                     /*unsorted=*/1);
      HIP_CHECK(hipEventRecord(sort_t0, s_compute_));
      launch_sort_fixed_run(gen_bases[r], run_nrec_[r], sort_ws.as(), s_compute_, /*staged=*/true);
      HIP_CHECK(hipEventRecord(sort_t1, s_compute_));
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipEventSynchronize(sort_t1));  // the next run reuses the workspace's record area
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, sort_t0, sort_t1));
      map_sort_ms_ += ms;
    }
  };
  if (!spilled()) {
    gen_runs(0, nruns);
    HIP_CHECK(hipStreamSynchronize(s_compute_));
  } else {
    for (int m = 0; m < M; ++m) {
      gen_runs(m * W, (m + 1) * W);
      if (disk_store())  // map output written to its MOF file (O_DIRECT through io_uring)
        disk_->write_file(m, tmp.as<uint8_t>(), mof_off_[m + 1] - mof_off_[m], s_compute_);
      else
        HIP_CHECK(hipMemcpyAsync(store_base_ + mof_off_[m], tmp.as(), (size_t)(mof_off_[m + 1] - mof_off_[m]),
                                 hipMemcpyDeviceToHost, s_compute_));
    }
    HIP_CHECK(hipStreamSynchronize(s_compute_));
  }
  std::vector<uint64_t> ck(nruns);
  HIP_CHECK(hipMemcpy(ck.data(), d_ck.as(), nruns * 8, hipMemcpyDeviceToHost));
  dest_checksum_.assign(W, 0);
  dest_records_.assign(W, 0);
  run_gen_ck_ = ck;
  for (int m = 0; m < M; ++m)
    for (int d = 0; d < W; ++d) {
      dest_checksum_[d] += ck[m * W + d];
      dest_records_[d] += run_nrec_[m * W + d];
    }
  // persistent per-run device tables for splitting
  d_run_bases_.alloc(nruns * sizeof(uint8_t*));
  d_run_nrec_.alloc(nruns * 8);
  d_bound_set_.alloc(nruns * sizeof(int));
  std::vector<int> bset(nruns);
  for (int r = 0; r < nruns; ++r) bset[r] = r % W;
  HIP_CHECK(hipMemcpy(d_run_bases_.as(), bases.data(), nruns * sizeof(uint8_t*), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(d_run_nrec_.as(), run_nrec_.data(), nruns * 8, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(d_bound_set_.as(), bset.data(), nruns * sizeof(int), hipMemcpyHostToDevice));
  UDA_LOG(kInfo, "rank %d generated %d MOFs, %ld bytes in %s%s", cfg_.rank, M, (long)store_bytes_,
          store_name().c_str(), cfg_.map_sort ? " (map-side device sort)" : "");
}

std::string ShuffleJob::store_name() const {
  if (disk_) return disk_->describe();
  return host_store() ? "pinned host DRAM" : "HBM";
}

void ShuffleJob::for_run_batches(
    const std::function<void(int, int, uint8_t* const*, const int64_t*, const int*)>& fn) {
  const int M = cfg_.maps_per_rank, W = cfg_.world;
  if (!disk_store()) {
    fn(0, M * W, d_run_bases_.as<uint8_t*>(), d_run_nrec_.as<int64_t>(), d_bound_set_.as<int>());
    return;
  }
  int64_t max_mof = 0;
  for (int m = 0; m < M; ++m) max_mof = std::max(max_mof, mof_off_[m + 1] - mof_off_[m]);
  DeviceBuffer tmp((size_t)max_mof), d_b((size_t)W * sizeof(uint8_t*));
  std::vector<uint8_t*> b(W);
  for (int m = 0; m < M; ++m) {
    disk_->stage({DiskStore::Piece{m, 0, mof_off_[m + 1] - mof_off_[m], tmp.as<uint8_t>()}}, s_compute_);
    for (int d = 0; d < W; ++d) b[d] = tmp.as<uint8_t>() + (run_off_[m * W + d] - mof_off_[m]);
    HIP_CHECK(hipMemcpyAsync(d_b.as(), b.data(), (size_t)W * sizeof(uint8_t*), hipMemcpyHostToDevice, s_compute_));
    fn(m * W, W, d_b.as<uint8_t*>(), d_run_nrec_.as<int64_t>() + m * W, d_bound_set_.as<int>() + m * W);
    HIP_CHECK(hipStreamSynchronize(s_compute_));  // tmp is reused by the next MOF
  }
}

std::vector<int64_t> ShuffleJob::index_record(int m, int d) const {
  const int W = cfg_.world;
  if (m < 0 || m >= cfg_.maps_per_rank || d < 0 || d >= W) throw std::out_of_range("index_record");
  const int r = m * W + d;
  const int64_t part = run_nrec_[r] * kTeraRecordBytes + kEofBytes;
  return {run_off_[r] - mof_off_[m], part, part};
}

std::vector<uint8_t> ShuffleJob::read_partition(int m, int d) const {
  auto ir = index_record(m, d);
  if (disk_) return disk_->read_host(m, ir[0], ir[2]);
  std::vector<uint8_t> out((size_t)ir[2]);
  HIP_CHECK(hipMemcpy(out.data(), store_base_ + mof_off_[m] + ir[0], out.size(),
                      host_store() ? hipMemcpyHostToHost : hipMemcpyDeviceToHost));
  return out;
}

std::vector<std::vector<uint64_t>> ShuffleJob::sample_keys(int64_t every) {
  const int M = cfg_.maps_per_rank, W = cfg_.world;
  const int nruns = M * W;
  every = std::max<int64_t>(1, every);
  std::vector<int64_t> soff(nruns + 1, 0);
  for (int r = 0; r < nruns; ++r) {
    const int64_t n = run_nrec_[r];
    const int64_t c = n > every / 2 ? (n - every / 2 + every - 1) / every : 0;
    soff[r + 1] = soff[r] + c;
  }
  const int64_t total = soff[nruns];
  std::vector<std::vector<uint64_t>> out(W);
  if (total == 0) return out;
  DeviceBuffer d_off((nruns + 1) * 8), d_out(total * sizeof(Elem));
  for_run_batches([&](int r0, int nr, uint8_t* const* bases, const int64_t* nrec, const int*) {
    std::vector<int64_t> rel(nr + 1);  // this batch's sample offsets, relative to its first sample
    for (int k = 0; k <= nr; ++k) rel[k] = soff[r0 + k] - soff[r0];
    if (rel[nr] == 0) return;
    HIP_CHECK(hipMemcpyAsync(d_off.as<int64_t>() + r0, rel.data(), (nr + 1) * 8, hipMemcpyHostToDevice, s_compute_));
    launch_sample_fixed(bases, nrec, nr, every, d_off.as<int64_t>() + r0, rel[nr], d_out.as<Elem>() + soff[r0],
                        s_compute_);
    HIP_CHECK(hipStreamSynchronize(s_compute_));  // rel is reused
  });
  HIP_CHECK(hipStreamSynchronize(s_compute_));
  std::vector<Elem> h(total);
  HIP_CHECK(hipMemcpy(h.data(), d_out.as(), total * sizeof(Elem), hipMemcpyDeviceToHost));
  for (int r = 0; r < nruns; ++r) {
    auto& v = out[r % W];
    for (int64_t i = soff[r]; i < soff[r + 1]; ++i) {
      v.push_back(h[i].hi);
      v.push_back(h[i].lo);
    }
  }
  return out;
}

void ShuffleJob::set_bounds(const std::vector<uint64_t>& bounds) {
  const int W = cfg_.world;
  if ((int64_t)bounds.size() != (int64_t)W * (C_ - 1) * 2)
    throw std::runtime_error("set_bounds: expected world*(reducers*rounds-1)*2 values");
  bounds_ = bounds;
  if (C_ > 1) {
    d_bounds_.alloc(bounds.size() * 8);
    HIP_CHECK(hipMemcpy(d_bounds_.as(), bounds.data(), bounds.size() * 8, hipMemcpyHostToDevice));
  }
}

void ShuffleJob::plan() {
  HIP_CHECK(hipSetDevice(cfg_.device));
  compute_plans();
  if (cfg_.deliver_host && !copy_thr_.joinable()) {
    const size_t ring_bytes = (size_t)lay_.slot_bytes * lay_.slots;
    if (cfg_.d2h == "sdma") {
      sdma_.reset(new SdmaEngine(cfg_.device));
      ring_ = static_cast<uint8_t*>(sdma_->alloc_host(ring_bytes));
      piece_sig_.resize(cfg_.pinned_slots);
      for (auto& sg : piece_sig_) sg = sdma_->make_signal();
    } else {
      ring_ = static_cast<uint8_t*>(hip_host_alloc_on_node(ring_bytes, device_numa_node(cfg_.device)));
      piece_ev_.resize(cfg_.pinned_slots);
      for (auto& e : piece_ev_) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // first touch from this thread: the pages land where the allocation policy put them
    for (size_t o = 0; o < ring_bytes; o += 4096) ring_[o] = 0;
    ring_numa_ = numa_residency(ring_);
    pinned_free_.assign(cfg_.pinned_slots, true);
    slot_flying_.assign(cfg_.pinned_slots, false);
    flying_ = 0;
    items_.assign(R_, {});
    eof_bufs_.clear();
    for (int i = 0; i < R_; ++i) eof_bufs_.emplace_back(new uint8_t[(size_t)cfg_.kv_buf_bytes + 16]);
    unpack_bufs_.clear();
    if (pack_) {
      const size_t one = (size_t)std::max(cfg_.kv_buf_bytes, lay_.buf_bytes) + 16;
      for (int i = 0; i < R_; ++i) unpack_bufs_.emplace_back(new uint8_t[2 * one]);
    }
    copy_thr_ = std::thread([this] { name_thread("uda-copy"); copy_loop(); });
    for (int i = 0; i < R_; ++i) consumers_.emplace_back([this, i] { name_thread("uda-consume"); consume_loop(i); });
  }
  UDA_LOG(kInfo, "rank %d planned %d reducers x %d rounds, max round %ld records, delivery %s", cfg_.rank, R_, Q_,
          (long)plan_.max_round_records, delivery_name().c_str());
}

void ShuffleJob::wait_exchange_ok() {
  if (exchange_) exchange_->check();
}

}  // namespace gpu
}  // namespace uda
