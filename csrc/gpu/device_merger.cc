// DeviceMerger: merges K sorted FIXED10 runs on one stream. See device_engine.h.
#include "device_engine.h"
#include "engine_util.h"
#include "merge_plan.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>

namespace uda {
namespace gpu {

namespace {
int64_t total_records(const std::vector<RunDesc>& runs) {
  int64_t t = 0;
  for (const auto& r : runs) t += r.nrec;
  return t;
}
}  // namespace

// ------------------------------------------------------------------------------ DeviceMerger
// Per-round plan blob layout (all int64 unless noted), uploaded with one H2D copy:
//   RunDesc runs[K] | int64 elem_off[K+1] | uint8_t* bases[K] | per pass: pairs[3P], tile_prefix[P+1]
DeviceMerger::DeviceMerger(int64_t max_records, int max_runs)
    : max_records_(max_records), max_runs_(max_runs) {
  // the merge-tree buffers (2 x 16 B per record) are allocated on the tree path's first use: the
  // single-pass K-way merge, which takes every group of <= kKwMaxRuns runs, never touches them
  static const bool old_null = [] {  // tools/multirank_stress.py --old-memset 2: the r5 code here too
    const char* e = std::getenv("UDA_GEN_NULL_STREAM_MEMSET");
    return e && std::atoi(e) >= 2;
  }();
  flag_.alloc(sizeof(int));
  if (old_null) HIP_CHECK(hipMemset(flag_.as(), 0, sizeof(int)));
  else HIP_CHECK(hipMemsetAsync(flag_.as(), 0, sizeof(int), nullptr));
  int passes = 1;
  while ((1 << passes) < max_runs) ++passes;
  ++passes;  // groups that are not a power of two may need one extra copy-through level
  slot_bytes_ = (size_t)max_runs * (sizeof(RunDesc) + 2 * sizeof(int64_t) + sizeof(uint8_t*)) +
                (size_t)passes * (4 * (size_t)max_runs + 4) * sizeof(int64_t) + 64 * (size_t)(passes + 4);
  // single-pass K-way tables: runs, bases, counts, sample offsets, bound sets, group / cell tables
  slot_bytes_ += (size_t)max_runs * (sizeof(RunDesc) + 4 * sizeof(int64_t) + 2 * sizeof(int)) + 64 * 16;
  if (const char* e = std::getenv("UDA_KWAY")) kway_ = std::atoi(e) != 0;
  if (const char* e = std::getenv("UDA_KWAY_CAP")) kw_cap_ = std::atoi(e);
  if (const char* e = std::getenv("UDA_KWAY_STAGED")) kw_staged_ = std::atoi(e) != 0;
  if (kw_staged_ && kw_cap_ > 1024) kw_cap_ = 1024;  // a staged cell's records must fit LDS
  if (!kway_cap_supported(kw_cap_)) throw std::runtime_error("UDA_KWAY_CAP must be 512, 1024, 1536, 1792 or 2048");
  kw_overflow_.alloc(sizeof(int));
  if (old_null) {
    HIP_CHECK(hipMemset(kw_overflow_.as(), 0, sizeof(int)));
  } else {
    HIP_CHECK(hipMemsetAsync(kw_overflow_.as(), 0, sizeof(int), nullptr));
    // the merges run on non-blocking streams, which do not wait for the null stream
    HIP_CHECK(hipStreamSynchronize(nullptr));
  }
  slots_.resize(4);
  for (auto& s : slots_) {
    s.host.alloc(slot_bytes_);
    s.dev.alloc(slot_bytes_);
    HIP_CHECK(hipEventCreateWithFlags(&s.uploaded, hipEventDisableTiming));
  }
}

int64_t DeviceMerger::device_bytes() const {
  int64_t n = (int64_t)(elems_a_.held() + elems_b_.held() + splits_.held() + flag_.held() + kw_prof_.held() +
                        kw_overflow_.held());
  for (const auto& p : pbufs_)
    n += (int64_t)(p.samp_runs.held() + p.samp_a.held() + p.samp_b.held() + p.bounds.held() + p.split.held() +
                   p.splits.held());
  for (const auto& s : slots_) n += (int64_t)s.dev.held();
  return n;
}

DeviceMerger::~DeviceMerger() {
  for (auto& s : slots_)
    if (s.uploaded) (void)hipEventDestroy(s.uploaded);
  for (auto& p : pbufs_) {
    if (p.planned) (void)hipEventDestroy(p.planned);
    if (p.used) (void)hipEventDestroy(p.used);
  }
}

int DeviceMerger::kway_overflow_cells() {
  int v = 0;
  HIP_CHECK(hipMemcpy(&v, kw_overflow_.as(), sizeof(int), hipMemcpyDeviceToHost));
  return v;
}

bool DeviceMerger::bad_layout() {
  int v = 0;
  HIP_CHECK(hipMemcpy(&v, flag_.as(), sizeof(int), hipMemcpyDeviceToHost));
  return v != 0;
}

int64_t DeviceMerger::merge_fixed(const std::vector<RunDesc>& runs, const std::vector<int>& group_first,
                                  uint8_t* out, hipStream_t s) {
  const int K = (int)runs.size();
  if (K > max_runs_) throw std::runtime_error("DeviceMerger: too many runs");
  if (K > 65536) throw std::runtime_error("DeviceMerger: FIXED10 mode supports <= 65536 runs");
  if (group_first.empty() || group_first.front() != 0 || group_first.back() != K)
    throw std::runtime_error("DeviceMerger: bad run groups");
  int64_t total = 0;
  for (const auto& r : runs) total += r.nrec;
  if (total > max_records_) throw std::runtime_error("DeviceMerger: round exceeds capacity");
  last_passes_ = 0;
  if (total == 0) return 0;
  if (kway_) {
    int kmax = 0;
    for (size_t g = 0; g + 1 < group_first.size(); ++g) kmax = std::max(kmax, group_first[g + 1] - group_first[g]);
    if (kmax <= kKwMaxRuns) return merge_kway(runs, group_first, out, s);
  }

  if (!elems_a_.size()) {
    elems_a_.alloc_local((size_t)std::max<int64_t>(max_records_, 1) * sizeof(Elem));
    elems_b_.alloc_local((size_t)std::max<int64_t>(max_records_, 1) * sizeof(Elem));
    // tiles per pass <= records/2048 + pairs; splits buffer sized for one pass
    const int64_t max_tiles = max_records_ / kMergeTile + max_runs_ + 2;
    splits_.alloc_local((size_t)max_tiles * sizeof(int64_t));
  }
  Slot& slot = slots_[next_slot_];
  next_slot_ = (next_slot_ + 1) % (int)slots_.size();
  if (slot.used) HIP_CHECK(hipEventSynchronize(slot.uploaded));
  slot.used = true;

  // ---- build the plan blob on the host
  uint8_t* h = slot.host.as();
  uint8_t* d = slot.dev.as();
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    size_t o = off;
    off = (size_t)align_up((int64_t)(off + bytes), 16);
    if (off > slot_bytes_) throw std::runtime_error("DeviceMerger: plan blob overflow");
    return o;
  };
  const size_t o_runs = carve(sizeof(RunDesc) * K);
  const size_t o_eoff = carve(sizeof(int64_t) * (K + 1));
  const size_t o_bases = carve(sizeof(uint8_t*) * K);
  std::memcpy(h + o_runs, runs.data(), sizeof(RunDesc) * K);
  int64_t* eoff = reinterpret_cast<int64_t*>(h + o_eoff);
  uint8_t** bases = reinterpret_cast<uint8_t**>(h + o_bases);
  eoff[0] = 0;
  for (int k = 0; k < K; ++k) {
    eoff[k + 1] = eoff[k] + runs[k].nrec;
    bases[k] = const_cast<uint8_t*>(runs[k].base);
  }
  const std::vector<MergePassPlan> plan = plan_merge_passes(std::vector<int64_t>(eoff, eoff + K + 1), group_first);
  std::vector<PassDesc> pds;
  for (const auto& mp : plan) {
    const size_t o_pairs = carve(sizeof(int64_t) * mp.pairs.size());
    const size_t o_tp = carve(sizeof(int64_t) * mp.tile_prefix.size());
    std::memcpy(h + o_pairs, mp.pairs.data(), sizeof(int64_t) * mp.pairs.size());
    std::memcpy(h + o_tp, mp.tile_prefix.data(), sizeof(int64_t) * mp.tile_prefix.size());
    PassDesc pd;
    pd.pairs = reinterpret_cast<const int64_t*>(d + o_pairs);
    pd.tile_prefix = reinterpret_cast<const int64_t*>(d + o_tp);
    pd.npairs = mp.npairs;
    pd.ntiles = mp.ntiles;
    pds.push_back(pd);
  }
  HIP_CHECK(hipMemcpyAsync(d, h, off, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipEventRecord(slot.uploaded, s));

  // ---- F2: keys
  Elem* cur = elems_a_.as<Elem>();
  Elem* nxt = elems_b_.as<Elem>();
  launch_extract_fixed(reinterpret_cast<const RunDesc*>(d + o_runs), reinterpret_cast<const int64_t*>(d + o_eoff), K,
                       total, cur, flag_.as<int>(), s);
  // ---- F3: merge tree (pairs never cross groups)
  for (const auto& pd : pds) {
    launch_merge_partition(cur, pd, splits_.as<int64_t>(), s);
    launch_merge_pass(cur, nxt, pd, splits_.as<int64_t>(), s);
    std::swap(cur, nxt);
  }
  last_passes_ = (int)pds.size();
  // ---- F4: gather records into merged order
  launch_gather_fixed(cur, total, reinterpret_cast<uint8_t* const*>(d + o_bases), out, s);
  return total;
}

// Tools: mean per-cell time of the k-way kernel phases (slices, F2 keys, F3 LDS merge, F4 gather)
// and the kernel span, from the per-workgroup wall-clock stamps. Synchronizes `s`.
static void report_kway_phases(const unsigned long long* dprof, int64_t ncells, hipStream_t s) {
  std::vector<unsigned long long> h((size_t)ncells * 5);
  HIP_CHECK(hipMemcpyAsync(h.data(), dprof, h.size() * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  int dev = 0, khz = 100000;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev);
  double sum[4] = {0, 0, 0, 0};
  unsigned long long t_min = ~0ull, t_max = 0;
  int64_t n = 0;
  for (int64_t c = 0; c < ncells; ++c) {
    const unsigned long long* p = &h[(size_t)c * 5];
    if (!p[4]) continue;  // overflow cells (PQ path) end early
    for (int k = 0; k < 4; ++k) sum[k] += (double)(p[k + 1] - p[k]);
    t_min = std::min(t_min, p[0]);
    t_max = std::max(t_max, p[4]);
    ++n;
  }
  if (!n) return;
  const double us = 1000.0 / khz;
  std::fprintf(stderr, "kway phases (mean us/cell over %lld cells): slices %.2f f2 %.2f f3 %.2f f4 %.2f | span %.1f us\n",
               (long long)n, sum[0] / n * us, sum[1] / n * us, sum[2] / n * us, sum[3] / n * us,
               (double)(t_max - t_min) * us);
}

// Single-pass K-way merge (kway.hip): sample -> merge the samples per group -> splitters ->
// per-run cell splits -> one workgroup per cell doing F2 + F3 + F4 in LDS.
int64_t DeviceMerger::merge_kway(const std::vector<RunDesc>& runs, const std::vector<int>& group_first, uint8_t* out,
                                 hipStream_t s) {
  const KwayPlan p = plan_kway(runs, group_first, s);
  return run_kway(p, out, s);
}

bool DeviceMerger::kway_applicable(const std::vector<RunDesc>& runs, const std::vector<int>& group_first) const {
  if (!kway_ || group_first.empty() || group_first.back() != (int)runs.size() || (int)runs.size() > max_runs_)
    return false;
  int64_t total = 0;
  for (const auto& r : runs) total += r.nrec;
  if (total > max_records_) return false;
  for (size_t g = 0; g + 1 < group_first.size(); ++g)
    if (group_first[g + 1] - group_first[g] > kKwMaxRuns) return false;
  return true;
}

// Cell planning of one K-way merge (sample -> merge the samples per group -> splitters -> per-run
// cell splits), enqueued on `s` into one of two plan slots. The slot's previous tiles must be done
// reading it first (device-side wait), so planning round q+1 on a side stream overlaps the tiles of
// round q on the compute stream.
DeviceMerger::KwayPlan DeviceMerger::plan_kway(const std::vector<RunDesc>& runs, const std::vector<int>& group_first,
                                               hipStream_t s) {
  const int K = (int)runs.size();
  const int G = (int)group_first.size() - 1;
  KwayPlan kp;
  kp.pslot = next_pslot_;
  next_pslot_ ^= 1;
  PlanBufs& pb = pbufs_[kp.pslot];
  if (!pb.planned) {
    HIP_CHECK(hipEventCreateWithFlags(&pb.planned, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&pb.used, hipEventDisableTiming));
  }
  if (pb.used_valid) HIP_CHECK(hipStreamWaitEvent(s, pb.used, 0));
  int kmax = 1;
  for (int g = 0; g < G; ++g) kmax = std::max(kmax, group_first[g + 1] - group_first[g]);
  const int64_t cap = kw_cap_;
  // target records per cell: cap * fill %; the rest of the capacity is the sampling slack (K * step)
  const char* fe = std::getenv("UDA_KWAY_FILL");  // read per plan: tests flip it within one process
  const int fill = fe ? std::min(90, std::max(10, std::atoi(fe))) : 65;  // profiles/r3_kway_occupancy.md
  int64_t T = cap * fill / 100;
  if (const char* e = std::getenv("UDA_KWAY_TARGET")) T = std::max<int64_t>(1, std::atoll(e));  // tests: force the PQ path
  const int64_t step = std::max<int64_t>(1, (cap - std::min<int64_t>(T, cap)) / (kmax + 2));  // cell <= T + K*step
  std::vector<int64_t> soff(K + 1, 0), nrec(K);
  std::vector<uint8_t*> bases(K);
  std::vector<int> bset(K);
  for (int g = 0; g < G; ++g)
    for (int r = group_first[g]; r < group_first[g + 1]; ++r) bset[r] = g;
  for (int r = 0; r < K; ++r) {
    nrec[r] = runs[r].nrec;
    bases[r] = const_cast<uint8_t*>(runs[r].base);
    const int64_t c = nrec[r] > step / 2 ? (nrec[r] - step / 2 + step - 1) / step : 0;
    soff[r + 1] = soff[r] + c;
  }
  const int64_t ns = soff[K];
  std::vector<int64_t> gcells(G), cell_first(G + 1, 0), gsamp(G + 1, 0), gout(G, 0);
  int64_t nbmax = 0, acc = 0;
  for (int g = 0; g < G; ++g) {
    int64_t ng = 0;
    for (int r = group_first[g]; r < group_first[g + 1]; ++r) ng += nrec[r];
    gcells[g] = std::max<int64_t>(1, (ng + T - 1) / T);
    cell_first[g + 1] = cell_first[g] + gcells[g];
    gsamp[g] = soff[group_first[g]];
    gout[g] = acc;
    acc += ng;
    nbmax = std::max(nbmax, gcells[g] - 1);
  }
  gsamp[G] = soff[K];
  const int64_t per = nbmax + 2;
  auto ensure = [](DeviceBuffer& b, size_t bytes) {
    if (b.size() < bytes) b.alloc_local(bytes + bytes / 8);
  };
  ensure(pb.samp_a, (size_t)std::max<int64_t>(ns, 1) * sizeof(Elem));
  ensure(pb.samp_b, (size_t)std::max<int64_t>(ns, 1) * sizeof(Elem));
  ensure(pb.samp_runs, (size_t)std::max<int64_t>(ns, 1) * sizeof(Elem));
  ensure(pb.bounds, (size_t)std::max<int64_t>((int64_t)G * nbmax, 1) * sizeof(Elem));
  ensure(pb.split, (size_t)K * per * sizeof(int64_t));
  ensure(pb.splits, (size_t)(ns / kMergeTile + K + 2) * sizeof(int64_t));

  Slot& slot = slots_[next_slot_];
  next_slot_ = (next_slot_ + 1) % (int)slots_.size();
  if (slot.used) HIP_CHECK(hipEventSynchronize(slot.uploaded));
  slot.used = true;
  uint8_t* h = slot.host.as();
  uint8_t* d = slot.dev.as();
  size_t off = 0;
  auto carve = [&](const void* src, size_t bytes) {
    const size_t o = off;
    off = (size_t)align_up((int64_t)(off + bytes), 16);
    if (off > slot_bytes_) throw std::runtime_error("DeviceMerger: plan blob overflow (k-way)");
    std::memcpy(h + o, src, bytes);
    return o;
  };
  const size_t o_runs = carve(runs.data(), sizeof(RunDesc) * K);
  const size_t o_bases = carve(bases.data(), sizeof(uint8_t*) * K);
  const size_t o_nrec = carve(nrec.data(), 8 * K);
  const size_t o_soff = carve(soff.data(), 8 * (K + 1));
  const size_t o_bset = carve(bset.data(), sizeof(int) * K);
  const size_t o_gf = carve(group_first.data(), sizeof(int) * (G + 1));
  const size_t o_cf = carve(cell_first.data(), 8 * (G + 1));
  const size_t o_gs = carve(gsamp.data(), 8 * (G + 1));
  const size_t o_gc = carve(gcells.data(), 8 * G);
  const size_t o_go = carve(gout.data(), 8 * G);
  std::vector<PassDesc> pds;
  for (const auto& mp : plan_merge_passes(soff, group_first)) {
    const size_t o_pairs = carve(mp.pairs.data(), 8 * mp.pairs.size());
    const size_t o_tp = carve(mp.tile_prefix.data(), 8 * mp.tile_prefix.size());
    PassDesc pd;
    pd.pairs = reinterpret_cast<const int64_t*>(d + o_pairs);
    pd.tile_prefix = reinterpret_cast<const int64_t*>(d + o_tp);
    pd.npairs = mp.npairs;
    pd.ntiles = mp.ntiles;
    pds.push_back(pd);
  }
  HIP_CHECK(hipMemcpyAsync(d, h, off, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipEventRecord(slot.uploaded, s));

  // splitters: a regular sample of every run, merged per group, every (ns_g / C_g)-th kept; the
  // per-run sample stays intact (first merge pass reads it) and brackets the split searches
  Elem* sr = pb.samp_runs.as<Elem>();
  Elem* sbuf[2] = {pb.samp_a.as<Elem>(), pb.samp_b.as<Elem>()};
  if (ns > 0)
    launch_sample_fixed(reinterpret_cast<uint8_t* const*>(d + o_bases), reinterpret_cast<const int64_t*>(d + o_nrec), K,
                        step, reinterpret_cast<const int64_t*>(d + o_soff), ns, sr, s);
  const Elem* merged = sr;
  int w = 0;
  for (const auto& pd : pds) {
    launch_merge_partition(merged, pd, pb.splits.as<int64_t>(), s);
    launch_merge_pass(merged, sbuf[w], pd, pb.splits.as<int64_t>(), s);
    merged = sbuf[w];
    w ^= 1;
  }
  launch_pick_splitters(merged, reinterpret_cast<const int64_t*>(d + o_gs), reinterpret_cast<const int64_t*>(d + o_gc),
                        G, (int)nbmax, pb.bounds.as<Elem>(), s);
  launch_split_sampled(reinterpret_cast<uint8_t* const*>(d + o_bases), reinterpret_cast<const int64_t*>(d + o_nrec), sr,
                       reinterpret_cast<const int64_t*>(d + o_soff), step,
                       nbmax > 0 ? pb.bounds.as<Elem>() : nullptr, reinterpret_cast<const int*>(d + o_bset), K,
                       (int)nbmax, pb.split.as<int64_t>(), s);
  HIP_CHECK(hipEventRecord(pb.planned, s));
  KwayDesc& kd = kp.kd;
  kd.runs = reinterpret_cast<const RunDesc*>(d + o_runs);
  kd.group_first = reinterpret_cast<const int*>(d + o_gf);
  kd.cell_first = reinterpret_cast<const int64_t*>(d + o_cf);
  kd.split = pb.split.as<int64_t>();
  kd.nbmax = (int)nbmax;
  kd.group_out = reinterpret_cast<const int64_t*>(d + o_go);
  kd.G = G;
  kd.overflow = kw_overflow_.as<int>();
  kd.bad_layout = flag_.as<int>();
  kd.cap = (int)cap;
  kd.kmax = kmax;
  // the staged kernel reads each record's words from LDS at the run's own alignment mod 16: 8-byte
  // aligned runs only (partitions of Hadoop MOF files start 2 bytes after the previous one's EOF marker)
  bool aligned8 = true;
  for (const auto& r : runs) aligned8 = aligned8 && ((uintptr_t)r.base & 7) == 0;
  kd.staged = kw_staged_ && aligned8 ? 1 : 0;
  kp.ncells = cell_first[G];
  kp.total = total_records(runs);
  return kp;
}

int64_t DeviceMerger::run_kway(const KwayPlan& kp, uint8_t* out, hipStream_t s) {
  PlanBufs& pb = pbufs_[kp.pslot];
  HIP_CHECK(hipStreamWaitEvent(s, pb.planned, 0));
  KwayDesc kd = kp.kd;
  static const bool prof = std::getenv("UDA_KWAY_PROF") != nullptr;
  if (prof) {
    auto ensure = [](DeviceBuffer& b, size_t bytes) {
      if (b.size() < bytes) b.alloc_local(bytes + bytes / 8);
    };
    ensure(kw_prof_, (size_t)kp.ncells * 5 * 8);
    HIP_CHECK(hipMemsetAsync(kw_prof_.as(), 0, (size_t)kp.ncells * 5 * 8, s));
    kd.prof = kw_prof_.as<unsigned long long>();
  }
  HIP_CHECK(hipGetLastError());  // nothing pending from the plan's launches
  launch_kway_tiles(kd, kp.ncells, out, s);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(pb.used, s));
  pb.used_valid = true;
  if (prof) report_kway_phases(kd.prof, kp.ncells, s);
  last_passes_ = 1;
  return kp.total;
}

}  // namespace gpu
}  // namespace uda
