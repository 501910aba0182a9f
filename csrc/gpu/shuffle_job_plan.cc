// ShuffleJob's plan: the device work that feeds the host-only round planner (shuffle_plan.h) -- cell
// splits, slice checksums, the counts exchange -- and what turns the planner's offsets into buffers,
// spans and uploaded descriptor tables by adding base addresses.
#include "device_engine.h"
#include "engine_util.h"

#include <algorithm>
#include <stdexcept>

namespace uda {
namespace gpu {

namespace {
template <typename T>
void upload(DeviceBuffer& buf, const std::vector<T>& v) {
  buf.alloc(v.size() * sizeof(T));
  HIP_CHECK(hipMemcpy(buf.as(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
}
}  // namespace

// The cell split of every local run: (C + 1) record positions per run, as split_pos_ holds them.
std::vector<int64_t> ShuffleJob::split_runs() {
  const int nruns = cfg_.maps_per_rank * cfg_.world;
  const int64_t per = C_ + 1;
  for_run_batches([&](int r0, int nr, uint8_t* const* bases, const int64_t* nrec, const int* bset) {
    launch_split_fixed(bases, nrec, C_ > 1 ? d_bounds_.as<Elem>() : nullptr, bset, nr, C_ - 1,
                       d_split_out_.as<int64_t>() + (size_t)r0 * per, s_compute_);
  });
  std::vector<int64_t> pos((size_t)nruns * per, 0);
  HIP_CHECK(hipMemcpyAsync(pos.data(), d_split_out_.as(), pos.size() * 8, hipMemcpyDeviceToHost, s_compute_));
  HIP_CHECK(hipStreamSynchronize(s_compute_));
  return pos;
}

// Checksums of every (run, cell) slice of the local runs, [r * C + c]: what this rank sends (exchange
// verification at the peers) and its own cells (checked where the merge reads them).
std::vector<int64_t> ShuffleJob::checksum_cells() {
  const int nruns = cfg_.maps_per_rank * cfg_.world;
  const int64_t per = C_ + 1;
  auto pos = [&](int r, int c) { return split_pos_[(size_t)r * per + c]; };
  std::vector<int64_t> cell_ck((size_t)nruns * C_, 0);
  DeviceBuffer d_sl((size_t)nruns * C_ * sizeof(RunDesc)), d_ck((size_t)nruns * C_ * 8);
  for_run_batches([&](int r0, int nr, uint8_t* const* bases, const int64_t*, const int*) {
    std::vector<uint8_t*> hb(nr);
    HIP_CHECK(hipMemcpyAsync(hb.data(), bases, (size_t)nr * sizeof(uint8_t*), hipMemcpyDeviceToHost, s_compute_));
    HIP_CHECK(hipStreamSynchronize(s_compute_));
    std::vector<RunDesc> sl((size_t)nr * C_);
    int64_t max_n = 0;
    for (int k = 0; k < nr; ++k)
      for (int c = 0; c < C_; ++c) {
        RunDesc& d = sl[(size_t)k * C_ + c];
        d.base = hb[k] + pos(r0 + k, c) * kTeraRecordBytes;
        d.nrec = pos(r0 + k, c + 1) - pos(r0 + k, c);
        d.nbytes = d.nrec * kTeraRecordBytes;
        d.offsets = nullptr;
        max_n = std::max(max_n, d.nrec);
      }
    HIP_CHECK(hipMemcpyAsync(d_sl.as(), sl.data(), sl.size() * sizeof(RunDesc), hipMemcpyHostToDevice, s_compute_));
    for (size_t b = 0; b < sl.size(); b += 65535) {
      const int n = (int)std::min<size_t>(65535, sl.size() - b);
      launch_slice_checksums(d_sl.as<RunDesc>() + b, n, max_n, d_ck.as<unsigned long long>() + b, s_compute_);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(cell_ck.data() + (size_t)r0 * C_, d_ck.as(), sl.size() * 8, hipMemcpyDeviceToHost,
                             s_compute_));
    HIP_CHECK(hipStreamSynchronize(s_compute_));
  });
  return cell_ck;
}

// Round volumes, once per job: the cell split of every local run, the counts exchange (every
// reducer learns what each peer will send it in each round) and, for world > 1, the checksum of
// every slice a peer will send (exchange verification in validated steps). The arithmetic from there
// to every round's offsets is plan_rounds() (shuffle_plan.h); the rest turns offsets into buffers.
void ShuffleJob::compute_plans() {
  const int W = cfg_.world, me = cfg_.rank;
  const int nruns = cfg_.maps_per_rank * W;
  if (C_ > 1 && bounds_.empty()) throw std::runtime_error("reducers*rounds > 1 requires set_bounds()");
  d_split_out_.alloc((size_t)nruns * (C_ + 1) * 8);
  split_pos_ = split_runs();
  const std::vector<int64_t> send_counts = plan_send_counts(geo_, split_pos_);
  const std::vector<int64_t> cell_ck = checksum_cells();
  const std::vector<int64_t> send_ck = to_peer_layout(geo_, cell_ck);  // [p][q][i][m] like the counts
  std::vector<int64_t> recv_counts = send_counts, recv_ck = send_ck;
  if (W > 1) {
    if (!exchange_) throw std::runtime_error("world > 1 requires init_comm() or init_local()");
    exchange_->alltoall_i64(send_counts.data(), recv_counts.data(), geo_.n_per_peer(), s_comm_);
    exchange_->alltoall_i64(send_ck.data(), recv_ck.data(), geo_.n_per_peer(), s_comm_);
  }
  // The generation-time checksum of every run (what a validated step is checked against) must be what
  // the store holds: a mismatch is a wrong expectation, not a shuffle error. Checked after the
  // collectives, so a failing rank never leaves its peers waiting in one.
  for (int r = 0; r < nruns && (size_t)r < run_gen_ck_.size(); ++r) {
    uint64_t sum = 0;
    for (int c = 0; c < C_; ++c) sum += (uint64_t)cell_ck[(size_t)r * C_ + c];
    if (sum != run_gen_ck_[(size_t)r])
      throw std::runtime_error("plan: map output run " + std::to_string(r) + " of rank " + std::to_string(me) +
                               " holds records whose checksum differs from the one its generation computed");
  }
  plan_ = plan_rounds(geo_, spilled(), split_pos_, run_off_, recv_counts, recv_ck, cell_ck);
  alloc_round_buffers();
  build_round_spans();
  d_validate_.alloc(64 + (size_t)2 * R_ * sizeof(Elem));
  upload_check_tables();
  d_diag_.alloc((size_t)Q_ * diag_stride() * 8);
  d_d2h_runs_.alloc((size_t)R_ * sizeof(RunDesc));
  d_d2h_ck_.alloc((size_t)R_ * 8);
  upload_h2d_tables();
}

void ShuffleJob::alloc_round_buffers() {
  const int W = cfg_.world;
  merger_.reset(new DeviceMerger(plan_.max_round_records, R_ * W * cfg_.maps_per_rank));
  const size_t out_bytes = (size_t)std::max<int64_t>(1, plan_.max_round_records) * kTeraRecordBytes;
  out_slots_.clear();
  out_slots_.resize(kSlots);
  for (auto& b : out_slots_) b.alloc(out_bytes);
  plan_delivery_pack();
  recv_slots_.clear();
  if (staged()) {
    recv_slots_.resize(kSlots);
    for (auto& b : recv_slots_) b.alloc((size_t)std::max<int64_t>(plan_.max_slot_bytes, 16));
  }
  // spill tiers at world > 1: peers never read the host store (device memory only, for every
  // exchange backend); the round's outgoing slices are staged into HBM, double-buffered so the
  // staging of round q+1 overlaps the exchange of round q
  for (auto& b : send_staging_) b.reset();
  if (W > 1 && spilled())
    for (auto& b : send_staging_) b.alloc((size_t)std::max<int64_t>(plan_.max_send, 16));
  if (W > 1) exchange_->reserve(plan_.max_send);
}

// delivery bit-packing: every D2H piece of a round has a fixed region (its bound, at most 0.9 of the
// records plus header and padding) in the packed slot of the round's parity
void ShuffleJob::plan_delivery_pack() {
  packed_slots_.clear();
  d_pack_pieces_.clear();
  d_pack_results_.clear();
  h_pack_results_.clear();
  pack_n_.assign(Q_, 0);
  pack_max_nrec_.assign(Q_, 0);
  pack_early_.assign(Q_, 0);
  if (!pack_) return;
  int64_t packed_bytes = 64;
  int max_pieces = 1;
  std::vector<std::vector<PackPiece>> pieces(Q_);
  for (int q = 0; q < Q_; ++q) {
    pieces[q] = round_pieces(plan_.rounds[q].group_recs);
    if (pieces[q].size() > 65535) throw std::runtime_error("delivery_pack: more than 65535 D2H pieces in a round");
    pack_n_[q] = (int)pieces[q].size();
    max_pieces = std::max(max_pieces, pack_n_[q]);
    for (const PackPiece& pc : pieces[q]) {
      pack_max_nrec_[q] = std::max(pack_max_nrec_[q], pc.nrec);
      packed_bytes = std::max(packed_bytes, pc.dst_off + lay_.piece_bound(pc.nrec));
    }
  }
  packed_slots_.resize(kSlots);
  for (auto& b : packed_slots_) b.alloc((size_t)packed_bytes);
  d_pack_results_.resize(kSlots);
  h_pack_results_.resize(kSlots);
  for (int k = 0; k < kSlots; ++k) {
    d_pack_results_[k].alloc((size_t)max_pieces * sizeof(ColpackResult));
    h_pack_results_[k].alloc((size_t)max_pieces * sizeof(ColpackResult));
  }
  d_pack_table_.alloc(colpack_table_bytes(max_pieces));
  d_pack_pieces_.resize(Q_);
  for (int q = 0; q < Q_; ++q) {
    if (pieces[q].empty()) continue;
    // descriptors (and with them the results) in issue order; a piece's packed region stays where the
    // reducer-major list put it. Wave order: the first wave is packed by a launch of its own (run_step).
    std::vector<ColpackPieceDesc> v;
    int wave0 = 0;
    for (const DeliveryPiece& dp :
         delivery_schedule(plan_.rounds[q].group_recs, lay_.piece, cfg_.delivery_order, kTeraRecordBytes)) {
      const PackPiece& pc = pieces[q][(size_t)dp.pack_index];
      v.push_back(ColpackPieceDesc{out_slots_[q % kSlots].as<uint8_t>() + pc.src_off,
                                   packed_slots_[q % kSlots].as<uint8_t>() + pc.dst_off, pc.nrec});
    }
    for (int64_t g : plan_.rounds[q].group_recs) wave0 += g > 0 ? 1 : 0;
    if (cfg_.delivery_order == "wave" && wave0 < pack_n_[q]) pack_early_[q] = wave0;
    upload(d_pack_pieces_[q], v);
  }
}

// What Exchange::exchange() takes per round: the plan's slices and spans with their base addresses.
void ShuffleJob::build_round_spans() {
  const int W = cfg_.world, me = cfg_.rank, M = cfg_.maps_per_rank;
  xchg_.assign(Q_, RoundSpans());
  if (W == 1) return;
  for (int q = 0; q < Q_; ++q) {
    const ShuffleRoundPlan& rp = plan_.rounds[q];
    RoundSpans& x = xchg_[q];
    x.send.assign(W, {});
    x.recv.assign(W, {});
    uint8_t* rbuf = recv_slots_[q % kSlots].as<uint8_t>();
    uint8_t* sbuf = send_staging_[q & 1].as<uint8_t>();
    for (int p = 0; p < W; ++p) {
      if (spilled()) {
        for (const PlanSpan& sp : rp.staged_send[p]) x.send[p].push_back(Span{sbuf + sp.off, sp.bytes});
        for (const PlanSpan& sp : rp.staged_recv[p]) x.recv[p].push_back(Span{rbuf + sp.off, sp.bytes});
        continue;
      }
      for (const PlanSlice& sl : rp.send[p]) x.send[p].push_back(Span{store_base_ + sl.store_off, sl.bytes});
      if (p == me) continue;
      for (int i = 0; i < R_; ++i)
        for (int j = 0; j < M; ++j) {
          const size_t c = geo_.cell(p, i, j);
          if (rp.recv_cnt[c] > 0) x.recv[p].push_back(Span{rbuf + rp.recv_off[c], rp.recv_cnt[c] * kTeraRecordBytes});
        }
    }
  }
}

// Validate steps: per round, the received peer slices (exchange verification) and the own cells where
// the merge reads them, as RunDesc tables with the checksums expected of them.
void ShuffleJob::upload_check_tables() {
  d_verify_runs_.clear();
  d_verify_expect_.clear();
  d_verify_runs_.resize(Q_);
  d_verify_expect_.resize(Q_);
  d_own_runs_.clear();
  d_own_expect_.clear();
  d_own_runs_.resize(Q_);
  d_own_expect_.resize(Q_);
  size_t max_v = 0;
  for (int q = 0; q < Q_; ++q) {
    const ShuffleRoundPlan& rp = plan_.rounds[q];
    uint8_t* rbuf = staged() ? recv_slots_[q % kSlots].as<uint8_t>() : nullptr;
    std::vector<RunDesc> v;
    std::vector<int64_t> e;
    for (const PlanVerify& pv : rp.verify) {
      v.push_back(RunDesc{rbuf + pv.slot_off, pv.nrec, pv.nrec * kTeraRecordBytes, nullptr});
      e.push_back(pv.expect);
    }
    if (!v.empty()) {
      upload(d_verify_runs_[q], v);
      upload(d_verify_expect_[q], e);
    }
    max_v = std::max(max_v, v.size());
    v.clear();
    e.clear();
    for (const PlanOwn& o : rp.own) {
      const uint8_t* base = o.slot_off >= 0 ? rbuf + o.slot_off : store_dev_base_ + o.store_off;
      v.push_back(RunDesc{base, o.nrec, o.nrec * kTeraRecordBytes, nullptr});
      e.push_back(o.expect);
    }
    if (!v.empty()) {
      upload(d_own_runs_[q], v);
      upload(d_own_expect_[q], e);
    }
    max_v = std::max(max_v, v.size());
  }
  if (max_v > 65535) throw std::runtime_error("exchange verification: too many slices per round");
  if (max_v > 0) d_verify_got_.alloc(max_v * 8);
}

// pinned-DRAM tier: each round's H2D (own cells into the receive slot, and for W > 1 the outgoing
// slices into the send staging) is one batched-copy launch over fixed descriptors. The kernel reads
// the pinned store over PCIe; hipMemcpyAsync would queue these copies on the same SDMA engine as
// the D2H delivery and serialize the two directions of the link.
void ShuffleJob::upload_h2d_tables() {
  h2d_descs_.clear();
  if (const char* e = std::getenv("UDA_H2D_BLOCKS")) h2d_blocks_ = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("UDA_H2D_SDMA")) sdma_h2d_ = std::atoi(e) != 0;
  if (!host_store()) return;
  h2d_descs_.resize(Q_);
  for (int q = 0; q < Q_; ++q) {
    uint8_t* rbuf = recv_slots_[q % kSlots].as<uint8_t>();
    uint8_t* sbuf = send_staging_[q & 1].as<uint8_t>();
    std::vector<CopyDesc> v;
    for (const PlanCopy& c : plan_.rounds[q].h2d)
      v.push_back(CopyDesc{store_dev_base_ + c.store_off, (c.to_staging ? sbuf : rbuf) + c.dst_off, c.bytes});
    if (!v.empty()) upload(h2d_descs_[q], v);
  }
}

void ShuffleJob::refresh_plan() {
  const int W = cfg_.world;
  if (split_runs() != split_pos_) throw std::runtime_error("replan: the map outputs changed since plan()");
  if (W == 1) return;
  const std::vector<int64_t> send = plan_send_counts(geo_, split_pos_);
  std::vector<int64_t> recv(send.size());
  exchange_->alltoall_i64(send.data(), recv.data(), geo_.n_per_peer(), s_comm_);
  for (int q = 0; q < Q_; ++q)
    for (int s = 0; s < W; ++s)
      for (int i = 0; i < R_; ++i)
        for (int j = 0; j < cfg_.maps_per_rank; ++j)
          if (recv[geo_.peer_count(s, q, i, j)] != plan_.rounds[q].recv_cnt[geo_.cell(s, i, j)])
            throw std::runtime_error("replan: a peer's counts changed since plan()");
}

}  // namespace gpu
}  // namespace uda
