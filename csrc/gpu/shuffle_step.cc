// ShuffleJob::run_step(): one shuffle + merge + deliver pass, as a step object holding the step's locals
// with one method per thing the round loop does. See device_engine.h for the pipeline.
#include "device_engine.h"
#include "engine_util.h"
#include "sdma.h"
#include "uda/fault.h"
#include "uda/trace.h"

#include <algorithm>
#include <stdexcept>

namespace uda {
namespace gpu {

// Validate steps: where a wrong total checksum came from. Per (round q, reducer i): the received
// slices and own cells against their plan-time checksums right before and right after the merge, the
// merged output against the sum of its inputs, and (check_delivery) the output slot right before its
// D2H and the bytes the consumer received against the merged output.
void ShuffleJob::localize_mismatch(StepStats& st) {
  const int F = diag_stride();
  std::vector<uint64_t> dg((size_t)Q_ * F);
  HIP_CHECK(hipMemcpy(dg.data(), d_diag_.as(), dg.size() * 8, hipMemcpyDeviceToHost));
  std::vector<uint64_t> pre_d2h, deliv;
  bool check;
  {
    std::lock_guard<std::mutex> g(mu_);
    pre_d2h = pre_d2h_ck_;
    deliv = delivered_ck_;
    check = step_.check_delivery;
  }
  st.pre_merge_errors = st.own_errors = st.merge_errors = 0;
  st.pre_d2h_errors = st.delivery_errors = check ? 0 : -1;
  std::string first[5];
  auto note = [](std::string& f, const char* what, int q, int i, uint64_t a, uint64_t b) {
    if (!f.empty()) return;
    char buf[160];
    std::snprintf(buf, sizeof(buf), "%s: round %d reducer %d (%016llx vs %016llx)", what, q, i, (unsigned long long)a,
                  (unsigned long long)b);
    f = buf;
  };
  for (int q = 0; q < Q_; ++q) {
    const uint64_t* d = &dg[(size_t)q * F];
    st.pre_merge_errors += (int64_t)d[0];
    st.own_errors += (int64_t)(d[2] + d[3]);
    if (d[0]) note(first[0], "received slices wrong before the merge", q, -1, d[0], d[1]);
    if (d[2] || d[3]) note(first[1], "own cells wrong (before, after the merge)", q, -1, d[2], d[3]);
    for (int i = 0; i < R_; ++i) {
      const uint64_t merged = d[4 + i], expect = plan_.expect_group_ck[(size_t)q * R_ + i];
      if (merged != expect) {
        ++st.merge_errors;
        note(first[2], "merged output differs from its inputs", q, i, merged, expect);
      }
      if (!check) continue;
      if (pre_d2h[(size_t)q * R_ + i] != merged) {
        ++st.pre_d2h_errors;
        note(first[3], "output slot changed between the merge and its D2H", q, i, pre_d2h[(size_t)q * R_ + i], merged);
      }
      if (deliv[(size_t)q * R_ + i] != merged) {
        ++st.delivery_errors;
        note(first[4], "consumer received other bytes than the merge wrote", q, i, deliv[(size_t)q * R_ + i], merged);
      }
    }
  }
  st.diag.clear();
  for (const auto& f : first)
    if (!f.empty()) st.diag += (st.diag.empty() ? "" : "; ") + f;
}

class ShuffleJob::Step {
 public:
  Step(ShuffleJob& job, bool validate)
      : j_(job),
        validate_(validate),
        W_(job.cfg_.world),
        M_(job.cfg_.maps_per_rank),
        deliver_(job.cfg_.deliver_host),
        staged_send_(W_ > 1 && job.spilled()),
        sdma_stage_(job.spilled() && (job.disk_store() || (job.host_store() && job.sdma_h2d_))),
        ev_(4 * (size_t)job.Q_, nullptr),
        vstats_(job.d_validate_.as<unsigned long long>()),
        vprev_(reinterpret_cast<Elem*>(job.d_validate_.as<uint8_t>() + 64)),
        vlast_(vprev_ + job.R_),
        has_prev_(job.R_, false),
        staged_round_(job.Q_, 0),
        merge_recorded_(job.Q_, 0),
        xchg_recorded_(job.Q_, 0) {}
  // Joins the stager (released first when the round loop failed) and destroys the step's events.
  ~Step();
  StepStats run();

 private:
  void reset_step_state();
  void wait_until(const std::function<bool()>& ready);
  void stage_rounds();
  void stage_round(int q, SdmaEngine* eng, hsa_signal_t sig);
  void build_runs(int q, std::vector<RunDesc>& runs, std::vector<int>& group_first);
  void plan_first_round();
  void run_round(int q);
  void enqueue_exchange(int q);
  void check_inputs(int q, int at);
  int64_t merge_round(int q, std::vector<RunDesc>& runs, std::vector<int>& group_first, uint8_t* out);
  void inject_faults(int q, uint8_t* out);
  void validate_outputs(int q, uint8_t* out);
  void pack_round(int q);
  void drain();
  void read_stats();
  unsigned long long* diag(int q) const {
    return j_.d_diag_.as<unsigned long long>() + (size_t)q * j_.diag_stride();
  }

  ShuffleJob& j_;
  const bool validate_;
  const int W_, M_;
  const bool deliver_;
  // Spill tiers (pinned DRAM, disk): a staging thread fills each round's HBM buffers ahead of the
  // round loop: the own cells into the receive slot and, at world > 1, the outgoing slices into the
  // round's send staging (peers only ever read device memory). Pinned DRAM is copied on an SDMA
  // engine of its own: a copy kernel (or hipMemcpyAsync, which runs as one) reading host memory
  // stalls the merge kernels beside it in the CU memory pipeline, while on the copy engines staging
  // overlaps delivery (the link's other direction) and the merge. The disk tier reads through
  // io_uring into the pinned chunk ring and copies to HBM on a stream of its own. Before reusing a
  // receive slot the thread waits for the merge that read it; before reusing a send staging parity,
  // for the exchange that sent it and for the peers' copies (Exchange::wait_sent). The round loop
  // waits for staged_round_[q] instead of a stream dependency, then enqueues the exchange.
  const bool staged_send_, sdma_stage_;
  StepStats st_;
  double t0_ = 0;
  std::vector<hipEvent_t> ev_;  // per round: exchange start / end, merge start / end
  unsigned long long* vstats_;
  Elem *vprev_, *vlast_;
  std::vector<bool> has_prev_;
  int64_t xbase_ = 0;  // sequence number of this step's first exchange
  std::vector<char> staged_round_, merge_recorded_, xchg_recorded_;  // under mu_
  double stage_ms_ = 0;                                              // under mu_
  std::thread stage_thr_;
  // Runs read in place (HBM store, one rank): round q+1's cell planning is enqueued on the plan stream
  // right after round q's tiles, so it runs beside them instead of between them (+1.7 % device-only,
  // profiles/r3_kway_lookahead_ab.md).
  bool lookahead_ = false;
  DeviceMerger::KwayPlan next_plan_;
  DeviceBuffer fault_scratch_;  // MERGE_SWAP's third record; allocated when the fault fires
};

StepStats ShuffleJob::run_step(bool validate) {
  trace::Range tr_step("uda.step");
  HIP_CHECK(hipSetDevice(cfg_.device));
  if (!merger_) throw std::runtime_error("run_step before plan()");
  Step step(*this, validate);
  return step.run();
}

ShuffleJob::Step::~Step() {
  if (stage_thr_.joinable()) {
    if (std::uncaught_exceptions() > 0) {  // the round loop failed: release the stager
      std::lock_guard<std::mutex> g(j_.mu_);
      j_.stop_ = true;
      j_.cv_.notify_all();
    }
    stage_thr_.join();
  }
  for (hipEvent_t e : ev_)
    if (e) (void)hipEventDestroy(e);
}

StepStats ShuffleJob::Step::run() {
  st_.validated = validate_;
  t0_ = now_ms();
  reset_step_state();
  for (auto& e : ev_) HIP_CHECK(hipEventCreate(&e));
  if (validate_) {
    HIP_CHECK(hipMemsetAsync(j_.d_validate_.as(), 0, 64, j_.s_compute_));
    HIP_CHECK(hipMemsetAsync(j_.d_diag_.as(), 0, (size_t)j_.Q_ * j_.diag_stride() * 8, j_.s_compute_));
  }
  if (j_.cfg_.replan) {
    const double tp = now_ms();
    j_.refresh_plan();
    st_.plan_ms = now_ms() - tp;
  }
  if (sdma_stage_ && j_.disk_store() && !j_.s_stage_)
    HIP_CHECK(hipStreamCreateWithFlags(&j_.s_stage_, hipStreamNonBlocking));
  xbase_ = j_.xseq_;
  if (sdma_stage_) stage_thr_ = std::thread([this] { stage_rounds(); });
  plan_first_round();
  for (int q = 0; q < j_.Q_; ++q) run_round(q);
  drain();
  read_stats();
  if (j_.step_.error) throw std::runtime_error("delivery sink reported error " + std::to_string(j_.step_.error));
  return st_;
}

void ShuffleJob::Step::reset_step_state() {
  std::lock_guard<std::mutex> g(j_.mu_);
  if (j_.stop_) throw std::runtime_error("delivery pipeline stopped: " + j_.step_error_msg_);
  j_.out_free_.assign(j_.Q_, 0);
  j_.step_ = StepCounters{};
  j_.step_.t0_ms = t0_;
  j_.step_.check_delivery = validate_ && j_.cfg_.check_delivery && deliver_;
  j_.pre_d2h_ck_.assign((size_t)j_.Q_ * j_.R_, 0);
  j_.delivered_ck_.assign((size_t)j_.Q_ * j_.R_, 0);
}

void ShuffleJob::Step::wait_until(const std::function<bool()>& ready) {
  std::unique_lock<std::mutex> lk(j_.mu_);
  while (!j_.cv_.wait_for(lk, std::chrono::milliseconds(100), [&] { return ready() || j_.stop_; })) {
    if (j_.exchange_) {  // a lost peer must fail the step, not hang it
      lk.unlock();
      j_.wait_exchange_ok();
      lk.lock();
    }
  }
  if (j_.stop_) throw std::runtime_error("delivery pipeline failed: " + j_.step_error_msg_);
}

// The staging thread's body: round by round, once the buffers the round stages into are free again.
void ShuffleJob::Step::stage_rounds() {
  try {
    HIP_CHECK(hipSetDevice(j_.cfg_.device));
    SdmaEngine* eng = j_.host_store() ? &SdmaEngine::for_device(j_.cfg_.device) : nullptr;
    hsa_signal_t sig{};
    if (eng) sig = eng->make_signal();
    struct SigGuard {
      SdmaEngine* e;
      hsa_signal_t s;
      ~SigGuard() {
        if (e) e->destroy_signal(s);
      }
    } sig_guard{eng, sig};
    for (int q = 0; q < j_.Q_; ++q) {
      const int slot = q % kSlots;
      if (q >= kSlots) {
        {
          std::unique_lock<std::mutex> lk(j_.mu_);
          j_.cv_.wait(lk, [&] { return merge_recorded_[q - kSlots] != 0 || j_.stop_; });
          if (j_.stop_) break;
        }
        HIP_CHECK(hipEventSynchronize(j_.merged_ev_[slot]));  // the slot's previous round is merged
      }
      if (staged_send_ && q >= 2) {  // send staging parity q & 1 was sent by exchange q-2
        {
          std::unique_lock<std::mutex> lk(j_.mu_);
          j_.cv_.wait(lk, [&] { return xchg_recorded_[q - 2] != 0 || j_.stop_; });
          if (j_.stop_) break;
        }
        HIP_CHECK(hipEventSynchronize(j_.sent_ev_[q & 1]));
        j_.exchange_->wait_sent(xbase_ + q - 2);
      }
      stage_round(q, eng, sig);
    }
  } catch (const std::exception& e) {
    std::lock_guard<std::mutex> g(j_.mu_);
    if (!j_.stop_) j_.step_error_msg_ = std::string("H2D staging: ") + e.what();
    j_.stop_ = true;
    j_.cv_.notify_all();
  }
}

// One staged round: the plan's H2D list, copied by the SDMA engine (pinned DRAM) or read from the MOF
// files (disk), then marked staged.
void ShuffleJob::Step::stage_round(int q, SdmaEngine* eng, hsa_signal_t sig) {
  const double ts = now_ms();
  uint8_t* rbuf = j_.recv_slots_[q % kSlots].as<uint8_t>();
  uint8_t* sbuf = j_.send_staging_[q & 1].as<uint8_t>();
  std::vector<CopyDesc> pieces;
  std::vector<DiskStore::Piece> dpieces;
  for (const PlanCopy& c : j_.plan_.rounds[q].h2d) {
    uint8_t* dst = (c.to_staging ? sbuf : rbuf) + c.dst_off;
    if (eng)
      pieces.push_back(CopyDesc{j_.store_base_ + c.store_off, dst, c.bytes});
    else
      dpieces.push_back(DiskStore::Piece{c.map, c.store_off - j_.mof_off_[c.map], c.bytes, dst});
  }
  if (eng) {
    SdmaEngine::arm(sig, (int64_t)pieces.size());
    for (const CopyDesc& d : pieces) eng->copy_h2d(d.dst, d.src, (size_t)d.bytes, sig);
    SdmaEngine::wait(sig);
  } else {
    if (!dpieces.empty()) j_.disk_->stage(dpieces, j_.s_stage_);
    HIP_CHECK(hipStreamSynchronize(j_.s_stage_));
  }
  std::lock_guard<std::mutex> g(j_.mu_);
  staged_round_[q] = 1;
  stage_ms_ += now_ms() - ts;
  j_.cv_.notify_all();
}

// runs of round q, grouped by reducer: group i = cell (i, q) from every source map
void ShuffleJob::Step::build_runs(int q, std::vector<RunDesc>& runs, std::vector<int>& group_first) {
  const ShuffleRoundPlan& rp = j_.plan_.rounds[q];
  uint8_t* rbuf = j_.staged() ? j_.recv_slots_[q % kSlots].as<uint8_t>() : nullptr;
  runs.clear();
  group_first.assign(1, 0);
  runs.reserve((size_t)j_.R_ * W_ * M_);
  for (int i = 0; i < j_.R_; ++i) {
    for (int s = 0; s < W_; ++s)
      for (int j = 0; j < M_; ++j) {
        const size_t x = j_.geo_.cell(s, i, j);
        RunDesc d;
        d.nrec = rp.recv_cnt[x];
        d.nbytes = d.nrec * kTeraRecordBytes;
        d.offsets = nullptr;
        if (rp.recv_off[x] >= 0)
          d.base = rbuf + rp.recv_off[x];
        else  // own cell, read in place from the HBM store
          d.base = j_.store_dev_base_ + rp.self_off[(size_t)i * M_ + j];
        runs.push_back(d);
      }
    group_first.push_back((int)runs.size());
  }
}

// K-way lookahead: round 0's cells are planned before the loop, round q+1's beside round q's tiles.
void ShuffleJob::Step::plan_first_round() {
  if (j_.staged() || !j_.merger_->kway_enabled()) return;
  std::vector<RunDesc> r0;
  std::vector<int> g0;
  build_runs(0, r0, g0);
  if (j_.merger_->kway_applicable(r0, g0)) {
    lookahead_ = true;
    next_plan_ = j_.merger_->plan_kway(r0, g0, j_.s_plan_);
  }
}

void ShuffleJob::Step::run_round(int q) {
  trace::Range tr_round("uda.round");
  const int slot = q % kSlots;
  const ShuffleRoundPlan& rp = j_.plan_.rounds[q];
  if (j_.spilled())
    for (const PlanOwn& o : rp.own) st_.bytes_h2d += o.nrec * kTeraRecordBytes;
  if (staged_send_) st_.bytes_h2d += rp.send_bytes;
  if (sdma_stage_) wait_until([&] { return staged_round_[q] != 0; });
  if (j_.staged()) enqueue_exchange(q);
  std::vector<RunDesc> runs;
  std::vector<int> group_first;
  if (!lookahead_) build_runs(q, runs, group_first);
  // output slot reuse: every D2H piece of round q-kSlots must have landed
  if (deliver_ && q >= kSlots) {
    const double tw = now_ms();
    wait_until([&] { return j_.out_free_[q - kSlots] != 0; });
    st_.wait_out_ms += now_ms() - tw;
  }
  if (validate_) check_inputs(q, 0);
  HIP_CHECK(hipEventRecord(ev_[4 * q + 2], j_.s_compute_));
  uint8_t* out = j_.out_slots_[slot].as<uint8_t>();
  const int64_t n = merge_round(q, runs, group_first, out);
  if (validate_) {
    inject_faults(q, out);
    validate_outputs(q, out);
    check_inputs(q, 1);
  }
  HIP_CHECK(hipEventRecord(ev_[4 * q + 3], j_.s_compute_));
  if (j_.pack_ && deliver_ && j_.pack_n_[q] > 0) pack_round(q);
  HIP_CHECK(hipEventRecord(j_.merged_ev_[slot], j_.s_compute_));
  if (sdma_stage_) {
    std::lock_guard<std::mutex> g(j_.mu_);
    merge_recorded_[q] = 1;
    j_.cv_.notify_all();
  }
  st_.records += n;
  if (deliver_) {
    {
      std::lock_guard<std::mutex> g(j_.mu_);
      j_.round_q_.push_back(RoundOut{q, slot, rp.group_recs, j_.pack_early_[q]});
    }
    j_.cv_.notify_all();
  }
}

// The comm stream's part of round q: the receive slot's previous merge, the copy-kernel staging
// (pinned DRAM with UDA_H2D_SDMA=0), the exchange, and the compute stream's wait for all of it.
void ShuffleJob::Step::enqueue_exchange(int q) {
  const int slot = q % kSlots;
  const ShuffleRoundPlan& rp = j_.plan_.rounds[q];
  if (q >= kSlots) HIP_CHECK(hipStreamWaitEvent(j_.s_comm_, j_.merged_ev_[slot], 0));  // slot consumed
  HIP_CHECK(hipEventRecord(ev_[4 * q + 0], j_.s_comm_));
  if (j_.spilled() && !sdma_stage_) {
    if (staged_send_ && q >= 2) j_.exchange_->wait_sent(xbase_ + q - 2);  // peers done with this parity
    launch_batched_copy(j_.h2d_descs_[q].as<CopyDesc>(), (int)rp.h2d.size(), rp.h2d_max, j_.s_comm_, j_.h2d_blocks_);
  }
  if (W_ > 1) {
    j_.exchange_->exchange(j_.xchg_[q].send, j_.xchg_[q].recv, j_.s_comm_);
    ++j_.xseq_;
    HIP_CHECK(hipEventRecord(j_.sent_ev_[q & 1], j_.s_comm_));
    {
      std::lock_guard<std::mutex> g(j_.mu_);
      xchg_recorded_[q] = 1;
    }
    j_.cv_.notify_all();
    st_.bytes_sent += rp.send_bytes;
  }
  HIP_CHECK(hipEventRecord(ev_[4 * q + 1], j_.s_comm_));
  HIP_CHECK(hipEventRecord(j_.comm_ev_[slot], j_.s_comm_));
  HIP_CHECK(hipStreamWaitEvent(j_.s_compute_, j_.comm_ev_[slot], 0));
}

// the merge's inputs as it is about to read them (at = 0) or has read them (at = 1): received slices
// and own cells against their plan-time checksums (the same checks after the merge tell a late write
// from a late read)
void ShuffleJob::Step::check_inputs(int q, int at) {
  const ShuffleRoundPlan& rp = j_.plan_.rounds[q];
  unsigned long long* dg = diag(q);
  unsigned long long* got = j_.d_verify_got_.as<unsigned long long>();
  const int nv = (int)rp.verify.size(), no = (int)rp.own.size();
  if (W_ > 1 && nv > 0) {
    launch_slice_checksums(j_.d_verify_runs_[q].as<RunDesc>(), nv, rp.verify_max_nrec, got, j_.s_compute_);
    launch_count_mismatch(got, j_.d_verify_expect_[q].as<unsigned long long>(), nv, dg + at, j_.s_compute_);
    if (at == 1)
      launch_count_mismatch(got, j_.d_verify_expect_[q].as<unsigned long long>(), nv, vstats_ + 2, j_.s_compute_);
  }
  if (no > 0) {
    launch_slice_checksums(j_.d_own_runs_[q].as<RunDesc>(), no, rp.own_max_nrec, got, j_.s_compute_);
    launch_count_mismatch(got, j_.d_own_expect_[q].as<unsigned long long>(), no, dg + at + 2, j_.s_compute_);
  }
  HIP_CHECK(hipGetLastError());
}

// The merge of round q into `out`. With lookahead this round was planned while the previous one merged,
// and the next one is planned now.
int64_t ShuffleJob::Step::merge_round(int q, std::vector<RunDesc>& runs, std::vector<int>& group_first, uint8_t* out) {
  int64_t n = 0;
  if (lookahead_) {
    n = j_.merger_->run_kway(next_plan_, out, j_.s_compute_);
    if (q + 1 < j_.Q_) {
      build_runs(q + 1, runs, group_first);
      next_plan_ = j_.merger_->plan_kway(runs, group_first, j_.s_plan_);
    }
  } else {
    n = j_.merger_->merge_fixed(runs, group_first, out, j_.s_compute_);
  }
  HIP_CHECK(hipGetLastError());
  st_.merge_passes = std::max(st_.merge_passes, j_.merger_->last_passes());
  return n;
}

// Fault sites (uda/fault.h), polled once per validated round: a wrong merge the checks must report. Both
// act on the first reducer group with two or more records in this round's output slot.
void ShuffleJob::Step::inject_faults(int q, uint8_t* out) {
  const ShuffleRoundPlan& rp = j_.plan_.rounds[q];
  const bool swap_fault = fault_hit("MERGE_SWAP"), flip_fault = fault_hit("MERGE_FLIP");
  if (!swap_fault && !flip_fault) return;
  int64_t at = 0;
  int gi = 0;
  while (gi < j_.R_ && rp.group_recs[gi] < 2) at += rp.group_recs[gi++];
  if (gi >= j_.R_) return;
  uint8_t* r0 = out + at * kTeraRecordBytes;
  uint8_t* r1 = r0 + kTeraRecordBytes;
  hipStream_t s = j_.s_compute_;
  if (swap_fault) {  // records 0 and 1 exchanged: one inverted pair, the same checksum
    if (!fault_scratch_.size()) fault_scratch_.alloc_local(kTeraRecordBytes);
    uint8_t* t = fault_scratch_.as<uint8_t>();
    HIP_CHECK(hipMemcpyAsync(t, r0, kTeraRecordBytes, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(r0, r1, kTeraRecordBytes, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(r1, t, kTeraRecordBytes, hipMemcpyDeviceToDevice, s));
  }
  if (flip_fault) {  // one value bit of record 0: the same order, another checksum
    uint8_t b = 0;
    uint8_t* p = r0 + kTeraKeyOffset + kTeraKeyBytes + 1 + 40;
    HIP_CHECK(hipMemcpyAsync(&b, p, 1, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    b ^= 0x01;
    HIP_CHECK(hipMemcpyAsync(p, &b, 1, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
}

// Per reducer: order within the round's output and against the reducer's last key of the round before,
// and its checksum.
void ShuffleJob::Step::validate_outputs(int q, uint8_t* out) {
  const ShuffleRoundPlan& rp = j_.plan_.rounds[q];
  unsigned long long* dg = diag(q);
  int64_t goff = 0;
  for (int i = 0; i < j_.R_; ++i) {
    const int64_t g = rp.group_recs[i];
    if (g > 0) {
      launch_validate_fixed(out + goff * kTeraRecordBytes, g, vprev_ + i, has_prev_[i] ? 1 : 0, vlast_ + i, vstats_,
                            j_.s_compute_, dg + 4 + i);
      HIP_CHECK(hipMemcpyAsync(vprev_ + i, vlast_ + i, sizeof(Elem), hipMemcpyDeviceToDevice, j_.s_compute_));
      has_prev_[i] = true;
    }
    goff += g;
  }
}

// bit-pack the round's D2H pieces; lengths and flags to the copy thread
void ShuffleJob::Step::pack_round(int q) {
  const int slot = q % kSlots;
  // pieces [a, b) of the round's issue-ordered descriptors: pack them, results to the pinned table
  auto pack_range = [&](int a, int b) {
    launch_colpack(j_.d_pack_pieces_[q].as<ColpackPieceDesc>() + a, b - a, j_.pack_max_nrec_[q], kTeraRecordBytes,
                   j_.lay_.buf_records, j_.d_pack_table_.as<uint32_t>(),
                   j_.d_pack_results_[slot].as<ColpackResult>() + a, j_.s_compute_, j_.lay_.pack_version, kTeraKeyOffset,
                   kTeraKeyBytes);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(j_.h_pack_results_[slot].as<ColpackResult>() + a,
                             j_.d_pack_results_[slot].as<ColpackResult>() + a, (size_t)(b - a) * sizeof(ColpackResult),
                             hipMemcpyDeviceToHost, j_.s_compute_));
  };
  if (j_.pack_early_[q] > 0) {  // the first wave leaves while the rest of the round is packed
    pack_range(0, j_.pack_early_[q]);
    HIP_CHECK(hipEventRecord(j_.early_ev_[slot], j_.s_compute_));
  }
  pack_range(j_.pack_early_[q], j_.pack_n_[q]);
}

// End of the step: every reducer's EOF is out, the streams are idle, the stager is joined.
void ShuffleJob::Step::drain() {
  if (deliver_) wait_until([&] { return j_.step_.eof_count == j_.R_; });
  if (j_.exchange_) j_.exchange_->wait(j_.s_comm_);
  HIP_CHECK(hipStreamSynchronize(j_.s_compute_));
  HIP_CHECK(hipStreamSynchronize(j_.s_comm_));
  HIP_CHECK(hipStreamSynchronize(j_.s_copy_));
  if (stage_thr_.joinable()) stage_thr_.join();
  // every rank's pulls from this rank's memory are done before any rank reuses or frees it
  if (j_.exchange_) j_.exchange_->quiesce();
}

void ShuffleJob::Step::read_stats() {
  StepStats& st = st_;
  const StepCounters& c = j_.step_;
  st.wall_ms = now_ms() - t0_;
  st.stage_ms = stage_ms_;
  for (int q = 0; q < j_.Q_; ++q) {
    float a = 0, b = 0;
    if (j_.staged() && hipEventElapsedTime(&a, ev_[4 * q + 0], ev_[4 * q + 1]) == hipSuccess) st.comm_ms += a;
    if (hipEventElapsedTime(&b, ev_[4 * q + 2], ev_[4 * q + 3]) == hipSuccess) st.merge_ms += b;
    st.round_comm_ms.push_back(a);
    st.round_merge_ms.push_back(b);
  }
  static const bool round_trace = std::getenv("UDA_ROUND_TRACE") != nullptr;  // tools: per-round timeline
  if (round_trace && j_.staged()) {
    std::string line = "[round trace ms: comm start-end | merge start-end]";
    for (int q = 0; q < j_.Q_; ++q) {
      float t[4] = {0, 0, 0, 0};
      for (int k = 0; k < 4; ++k) (void)hipEventElapsedTime(&t[k], ev_[0], ev_[4 * q + k]);
      char b[96];
      snprintf(b, sizeof(b), " q%d %.0f-%.0f|%.0f-%.0f", q, t[0], t[1], t[2], t[3]);
      line += b;
    }
    fprintf(stderr, "%s\n", line.c_str());
  }
  st.d2h_ms = c.d2h_ms;
  st.bytes_in = st.records * kTeraRecordBytes;
  st.buffers = c.buffers;
  {
    std::lock_guard<std::mutex> g(j_.mu_);
    st.d2h_bytes = c.d2h_bytes;
    st.packed_pieces = c.packed;
    st.raw_pieces = c.raw;
    st.pack_delta_pieces = c.delta;
    st.pack_stride_min = std::max<int64_t>(c.stride_min, 0);
    st.pack_stride_max = c.stride_max;
    if (deliver_ && j_.pack_) j_.last_delta_ = c.packed > 0 && c.delta == c.packed ? 1 : 0;
    st.unpack_ms = c.unpack_ms;
    st.slot_wait_ms = c.slot_wait_ms;
    if (c.first_issue_ms >= 0) {  // every piece has landed and every EOF is out by now
      st.lead_in_ms = c.first_issue_ms - c.t0_ms;
      st.link_idle_ms = c.link_idle_ms;
      if (c.eof_done_ms >= c.last_landing_ms) st.tail_ms = c.eof_done_ms - c.last_landing_ms;
    }
  }
  if (deliver_ && st.bytes_in > 0) j_.last_d2h_ratio_ = (double)st.d2h_bytes / (double)st.bytes_in;
  if (validate_) {
    unsigned long long v[3];
    HIP_CHECK(hipMemcpy(v, vstats_, sizeof(v), hipMemcpyDeviceToHost));
    st.order_errors = (int64_t)v[0];
    st.checksum = v[1];
    st.exchange_errors = W_ > 1 ? (int64_t)v[2] : 0;
    j_.localize_mismatch(st);
  }
  st.bad_layout = j_.merger_->bad_layout();
}

}  // namespace gpu
}  // namespace uda
