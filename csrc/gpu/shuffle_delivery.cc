// ShuffleJob's delivery: the copy thread (merged rounds -> D2H pieces in the pinned ring), the per-reducer
// consumer threads and the link-occupancy bookkeeping they share. See device_engine.h.
#include "device_engine.h"
#include "engine_util.h"
#include "sdma.h"
#include "uda/topology.h"

#include <algorithm>
#include <stdexcept>

namespace uda {
namespace gpu {

std::string ShuffleJob::delivery_name() const {
  if (!cfg_.deliver_host) return "none";
  std::string name = sdma_ ? sdma_->describe() : "hip[numa=" + std::to_string(device_numa_node(cfg_.device)) + "]";
  name += " ring=" + ring_numa_ + " order=" + cfg_.delivery_order;
  if (!pack_) return name + " pack=off";
  name += " pack=colbits v" + std::to_string(lay_.pack_version);
  if (last_delta_ >= 0) name += last_delta_ ? " delta" : " plain";  // the last step's pieces
  if (last_d2h_ratio_ >= 0) {  // the last step's d2h_bytes / bytes_in
    char b[32];
    std::snprintf(b, sizeof(b), " d2h/in=%.3f", last_d2h_ratio_);
    name += b;
  }
  return name;
}

std::vector<ShuffleJob::PackPiece> ShuffleJob::round_pieces(const std::vector<int64_t>& group_recs) const {
  std::vector<PackPiece> v;
  int64_t doff = 0;
  for (const DeliveryPiece& dp : delivery_schedule(group_recs, lay_.piece, "reducer", kTeraRecordBytes)) {
    const int64_t nrec = dp.len / kTeraRecordBytes;
    v.push_back(PackPiece{dp.src_off, doff, nrec});
    doff += lay_.piece_bound(nrec);
  }
  return v;
}

void ShuffleJob::note_issue(int k, double now) {
  if (step_.first_issue_ms < 0) step_.first_issue_ms = now;
  if (flying_ == 0 && step_.idle_since_ms >= 0) step_.link_idle_ms += now - step_.idle_since_ms;
  slot_flying_[k] = true;
  ++flying_;
}

void ShuffleJob::note_landing(int k, double now) {
  if (!slot_flying_[k]) return;  // another waiter saw it first
  slot_flying_[k] = false;
  step_.last_landing_ms = now;
  if (--flying_ == 0) step_.idle_since_ms = now;
}

void ShuffleJob::poll_landings() {
  if (flying_ == 0) return;
  for (int k = 0; k < (int)slot_flying_.size(); ++k) {
    if (!slot_flying_[k]) continue;
    // a copy error (negative signal, failed event) is left to the piece's waiter, which throws
    bool done;
    if (sdma_) {
      done = hsa_signal_load_relaxed(piece_sig_[k]) == 0;
    } else {
      const hipError_t e = hipEventQuery(piece_ev_[k]);
      done = e == hipSuccess;
      if (e == hipErrorNotReady) (void)hipGetLastError();  // not an error: not left for a later HIP_PENDING
    }
    if (done) note_landing(k, now_ms());
  }
}

// Copy thread: merged rounds -> D2H pieces in the pinned ring, in round order; within a round in
// delivery_schedule()'s order (cfg.delivery_order).
void ShuffleJob::copy_loop() {
  try {
    bind_thread_to_cpus(device_consumer_cpus(cfg_.device));
    HIP_CHECK(hipSetDevice(cfg_.device));
    for (;;) {
      RoundOut r;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || !round_q_.empty(); });
        if (stop_) return;
        r = std::move(round_q_.front());
        round_q_.pop_front();
      }
      // merged, and packed as far as the first pieces need: the whole round, or its first wave (r.early)
      HIP_CHECK(hipEventSynchronize(r.early > 0 ? early_ev_[r.slot] : merged_ev_[r.slot]));
      const uint8_t* src = out_slots_[r.slot].as<uint8_t>();
      const bool last_round = (r.q == Q_ - 1);
      bool check;
      {
        std::lock_guard<std::mutex> g(mu_);
        check = step_.check_delivery;
      }
      if (check) {  // the output slot as the D2H is about to read it, per reducer
        std::vector<RunDesc> gr(R_);
        int64_t o = 0, mx = 0;
        for (int i = 0; i < R_; ++i) {
          gr[i].base = src + o * kTeraRecordBytes;
          gr[i].nrec = r.group_recs[i];
          gr[i].nbytes = gr[i].nrec * kTeraRecordBytes;
          gr[i].offsets = nullptr;
          o += r.group_recs[i];
          mx = std::max(mx, r.group_recs[i]);
        }
        std::vector<uint64_t> ck(R_, 0);
        HIP_CHECK(hipMemcpyAsync(d_d2h_runs_.as(), gr.data(), (size_t)R_ * sizeof(RunDesc), hipMemcpyHostToDevice, s_copy_));
        launch_slice_checksums(d_d2h_runs_.as<RunDesc>(), R_, std::max<int64_t>(mx, 1),
                               d_d2h_ck_.as<unsigned long long>(), s_copy_);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(ck.data(), d_d2h_ck_.as(), (size_t)R_ * 8, hipMemcpyDeviceToHost, s_copy_));
        HIP_CHECK(hipStreamSynchronize(s_copy_));
        std::lock_guard<std::mutex> g(mu_);
        for (int i = 0; i < R_; ++i) pre_d2h_ck_[(size_t)r.q * R_ + i] = ck[i];
      }
      std::vector<int> used;
      // packed rounds: a piece's region is that of round_pieces()[pack_index]; its length and flag as the plan
      // kernel wrote them are in the results table at its place in the issue order
      const std::vector<PackPiece> ppieces = pack_ ? round_pieces(r.group_recs) : std::vector<PackPiece>();
      const ColpackResult* pres = pack_ ? h_pack_results_[r.slot].as<ColpackResult>() : nullptr;
      if (last_round) {  // a reducer without records in the last round: its EOF travels alone
        bool any = false;
        {
          std::lock_guard<std::mutex> g(mu_);
          for (int i = 0; i < R_; ++i)
            if (r.group_recs[i] == 0) {
              items_[i].push_back(Item{-1, 0, true, now_ms(), r.q});
              any = true;
            }
        }
        if (any) cv_.notify_all();
      }
      // Pieces go out in schedule order and take their ring slots in that order: every held slot belongs
      // to an issued piece whose consumer reaches it without needing another slot, so no order can deadlock.
      int issued = 0;
      for (const DeliveryPiece& dp :
           delivery_schedule(r.group_recs, lay_.piece, cfg_.delivery_order, kTeraRecordBytes)) {
        if (r.early > 0 && issued == r.early) HIP_CHECK(hipEventSynchronize(merged_ev_[r.slot]));  // the rest is packed
        int k = -1;
        {
          std::unique_lock<std::mutex> lk(mu_);
          auto have_slot = [&] {
            if (stop_) return true;
            for (bool f : pinned_free_)
              if (f) return true;
            return false;
          };
          if (!have_slot()) {  // ring full: meanwhile, see the copies in flight land (link_idle_ms)
            const double tw = now_ms();
            while (!cv_.wait_for(lk, std::chrono::microseconds(200), have_slot)) poll_landings();
            step_.slot_wait_ms += now_ms() - tw;
          }
          if (stop_) return;
          for (int x = 0; x < (int)pinned_free_.size(); ++x)
            if (pinned_free_[x]) {
              k = x;
              break;
            }
          pinned_free_[k] = false;
        }
        uint8_t* dst = lay_.slot(ring_, k);
        const uint8_t* from = src + dp.src_off;
        int64_t copy_len = dp.len;
        bool packed = false;
        if (pack_) {
          const size_t pi = (size_t)dp.pack_index;
          if (pi >= ppieces.size() || (size_t)issued >= ppieces.size() || ppieces[pi].src_off != dp.src_off ||
              ppieces[pi].nrec * kTeraRecordBytes != dp.len)
            throw std::runtime_error("delivery_pack: piece list out of step with the copy loop");
          const ColpackResult pr = pres[issued];
          if (pr.packed) {
            packed = true;
            copy_len = lay_.packed_copy_len(pr.bytes, ppieces[pi].nrec);
            from = packed_slots_[r.slot].as<uint8_t>() + ppieces[pi].dst_off;
          }
        }
        if (sdma_) {
          SdmaEngine::arm(piece_sig_[k], sdma_->parts((size_t)copy_len, cfg_.d2h_engines));
          sdma_->copy_d2h(dst, from, (size_t)copy_len, piece_sig_[k], cfg_.d2h_engines);
        } else {
          HIP_CHECK(hipMemcpyAsync(dst, from, (size_t)copy_len, hipMemcpyDeviceToHost, s_copy_));
          HIP_CHECK(hipEventRecord(piece_ev_[k], s_copy_));
        }
        used.push_back(k);
        ++issued;
        {
          std::lock_guard<std::mutex> g(mu_);
          const double now = now_ms();
          note_issue(k, now);
          items_[dp.reducer].push_back(Item{k, dp.len, last_round && dp.last_of_reducer, now, r.q, packed, copy_len});
          step_.d2h_bytes += copy_len;
          ++(packed ? step_.packed : step_.raw);
          if (packed) {
            const ColpackResult pr = pres[issued - 1];
            step_.delta += pr.delta ? 1 : 0;
            step_.stride_min = step_.stride_min < 0 ? (int64_t)pr.stride : std::min<int64_t>(step_.stride_min, pr.stride);
            step_.stride_max = std::max<int64_t>(step_.stride_max, pr.stride);
          }
        }
        cv_.notify_all();
      }
      // the output slot is free once every piece of this round has landed in the ring
      for (int k : used) {
        if (sdma_)
          SdmaEngine::wait(piece_sig_[k]);
        else
          HIP_CHECK(hipEventSynchronize(piece_ev_[k]));
        std::lock_guard<std::mutex> g(mu_);
        note_landing(k, now_ms());
      }
      {
        std::lock_guard<std::mutex> g(mu_);
        out_free_[r.q] = 1;
      }
      cv_.notify_all();
    }
  } catch (const std::exception& e) {
    std::lock_guard<std::mutex> g(mu_);
    if (step_error_msg_.empty()) step_error_msg_ = std::string("delivery copy thread: ") + e.what();
    stop_ = true;
    cv_.notify_all();
  }
}

// Consumer thread of reducer i: the "Java side" hand-off. Every item is one landed piece (or the EOF
// alone) for deliver_fixed_piece (fixed_delivery.h): buffers of whole records, at most kv_buf_bytes, the
// reducer's final one carrying the IFile EOF marker (-1, -1).
void ShuffleJob::consume_loop(int i) {
  try {
    bind_thread_to_cpus(device_consumer_cpus(cfg_.device));
    HIP_CHECK(hipSetDevice(cfg_.device));
    FixedBuffers bufs;
    bufs.tail = eof_bufs_[i].get();
    if (pack_) {
      bufs.staging[0] = unpack_bufs_[i].get();
      bufs.staging[1] = bufs.staging[0] + (size_t)std::max(cfg_.kv_buf_bytes, lay_.buf_bytes) + 16;
    }
    for (;;) {
      Item it;
      bool check;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || !items_[i].empty(); });
        if (stop_) return;
        it = items_[i].front();
        items_[i].pop_front();
        check = step_.check_delivery;
      }
      double waited = 0;
      FixedPiece p;  // an EOF-only item: no records, only `last`
      p.last = it.last;
      if (it.pslot >= 0) {
        if (sdma_)
          SdmaEngine::wait(piece_sig_[it.pslot]);
        else
          HIP_CHECK(hipEventSynchronize(piece_ev_[it.pslot]));
        {
          std::lock_guard<std::mutex> g(mu_);
          const double now = now_ms();
          note_landing(it.pslot, now);
          waited = now - it.issued_ms;
        }
        p.base = lay_.slot(ring_, it.pslot);
        p.copied = it.copied;
        p.record_bytes = it.bytes;
        p.packed = it.packed;
      }
      // What the delivery hands its buffers to: the check_delivery checksum of their records (not of the
      // EOF marker) and the job's sink. A sink error ends that sink's part in this item and fails the
      // step in run_step; it never fails the delivery, whose threads go on to the next step. Neither a
      // sink nor a checksum: an empty FixedSink, and a packed piece is checked but not unpacked.
      uint64_t got_ck = 0;
      int err = 0;
      FixedSink take;
      if (sink_ || check)
        take = [&](const uint8_t* b, int64_t len) {
          if (check)
            for (int64_t o = 0; o + kTeraRecordBytes <= len; o += kTeraRecordBytes)
              got_ck += record_hash(b + o, kTeraRecordBytes);
          if (sink_ && !err) err = sink_(i, b, len);
          return 0;
        };
      FixedDeliveryCounters c;
      deliver_fixed_piece(p, lay_.buf_bytes, lay_.kv_buf_bytes, bufs, take, &c);
      {
        std::lock_guard<std::mutex> g(mu_);
        if (it.pslot >= 0) pinned_free_[it.pslot] = true;
        if (check && it.q >= 0 && it.q < Q_) delivered_ck_[(size_t)it.q * R_ + i] += got_ck;
        step_.buffers += c.buffers;
        step_.d2h_ms += waited;
        step_.unpack_ms += c.unpack_ms;
        if (err && !step_.error) step_.error = err;
        if (it.last && ++step_.eof_count == R_) step_.eof_done_ms = now_ms();
      }
      cv_.notify_all();
    }
  } catch (const std::exception& e) {
    std::lock_guard<std::mutex> g(mu_);
    if (step_error_msg_.empty()) step_error_msg_ = std::string("delivery consumer thread: ") + e.what();
    stop_ = true;
    cv_.notify_all();
  }
}

}  // namespace gpu
}  // namespace uda
