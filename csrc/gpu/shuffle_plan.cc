// Round planning of the shuffle job: see shuffle_plan.h.
#include "shuffle_plan.h"

#include <algorithm>
#include <stdexcept>

namespace uda {
namespace gpu {

std::vector<int64_t> to_peer_layout(const ShuffleGeometry& g, const std::vector<int64_t>& per_run_cell) {
  const int C = g.cells();
  std::vector<int64_t> out((size_t)g.W * g.n_per_peer());
  for (int p = 0; p < g.W; ++p)
    for (int q = 0; q < g.Q; ++q)
      for (int i = 0; i < g.R; ++i)
        for (int m = 0; m < g.M; ++m)
          out[g.peer_count(p, q, i, m)] = per_run_cell[(size_t)(m * g.W + p) * C + i * g.Q + q];
  return out;
}

std::vector<int64_t> plan_send_counts(const ShuffleGeometry& g, const std::vector<int64_t>& split_pos) {
  const int C = g.cells(), nruns = g.M * g.W;
  std::vector<int64_t> cnt((size_t)nruns * C);
  for (int r = 0; r < nruns; ++r)
    for (int c = 0; c < C; ++c)
      cnt[(size_t)r * C + c] = split_pos[(size_t)r * (C + 1) + c + 1] - split_pos[(size_t)r * (C + 1) + c];
  return to_peer_layout(g, cnt);
}

namespace {

// Receive side of round q: counts, the s-major slot layout, the verification and own-cell lists.
// Returns the bytes of the slot the layout uses.
int64_t plan_receive(const ShuffleGeometry& g, bool spilled, int q, const std::vector<int64_t>& recv_counts,
                     const std::vector<int64_t>& recv_ck,
                     const std::vector<int64_t>& cell_ck, ShuffleRoundPlan& rp, uint64_t* expect_ck) {
  const int W = g.W, R = g.R, M = g.M, me = g.me, C = g.cells();
  const int64_t rb = g.record_bytes;
  rp.recv_cnt.assign((size_t)W * R * M, 0);
  rp.recv_off.assign((size_t)W * R * M, -1);
  rp.group_recs.assign(R, 0);
  int64_t off = 0;
  for (int s = 0; s < W; ++s)
    for (int i = 0; i < R; ++i)
      for (int j = 0; j < M; ++j) {
        const size_t x = g.cell(s, i, j);
        const int64_t cnt = recv_counts[g.peer_count(s, q, i, j)];
        rp.recv_cnt[x] = cnt;
        rp.group_recs[i] += cnt;
        if (s != me || spilled) {  // else: read in place from the store
          rp.recv_off[x] = off;
          off += cnt * rb;
        }
        const int64_t ck = s == me ? cell_ck[(size_t)(j * W + me) * C + i * g.Q + q] : recv_ck[g.peer_count(s, q, i, j)];
        expect_ck[i] += (uint64_t)ck;
        if (cnt <= 0) continue;
        if (s == me) {
          rp.own.push_back(PlanOwn{rp.recv_off[x], rp.self_off[(size_t)i * M + j], cnt, ck, j});
          rp.own_max_nrec = std::max(rp.own_max_nrec, cnt);
        } else {
          rp.verify.push_back(PlanVerify{rp.recv_off[x], cnt, ck});
          rp.verify_max_nrec = std::max(rp.verify_max_nrec, cnt);
        }
      }
  for (int i = 0; i < R; ++i) rp.recv_records += rp.group_recs[i];
  return off;
}

// Spill tiers, world > 1: one staged region per peer (send) and per source (receive).
void plan_staged_spans(const ShuffleGeometry& g, ShuffleRoundPlan& rp) {
  int64_t off = 0;
  for (int p = 0; p < g.W; ++p) {
    const int64_t beg = off;
    for (const PlanSlice& sl : rp.send[p]) off += sl.bytes;
    if (off > beg) rp.staged_send[p].push_back(PlanSpan{beg, off - beg});
  }
  for (int s = 0; s < g.W; ++s) {
    if (s == g.me) continue;
    int64_t first = -1, total = 0;
    for (int i = 0; i < g.R; ++i)
      for (int j = 0; j < g.M; ++j) {
        const size_t x = g.cell(s, i, j);
        const int64_t b = rp.recv_cnt[x] * g.record_bytes;
        if (b <= 0) continue;
        if (first < 0) first = rp.recv_off[x];
        if (rp.recv_off[x] != first + total) throw std::runtime_error("plan: a source's slices are not contiguous");
        total += b;
      }
    if (total > 0) rp.staged_recv[s].push_back(PlanSpan{first, total});
  }
}

// Spill tiers: what the round copies from the store into HBM.
void plan_h2d(const ShuffleGeometry& g, ShuffleRoundPlan& rp) {
  for (const PlanOwn& o : rp.own) rp.h2d.push_back(PlanCopy{o.store_off, false, o.slot_off, o.nrec * g.record_bytes, o.map});
  int64_t off = 0;
  for (int p = 0; p < g.W; ++p)
    for (const PlanSlice& sl : rp.send[p]) {
      rp.h2d.push_back(PlanCopy{sl.store_off, true, off, sl.bytes, sl.map});
      off += sl.bytes;
    }
  for (const PlanCopy& c : rp.h2d) rp.h2d_max = std::max(rp.h2d_max, c.bytes);
}

}  // namespace

ShufflePlan plan_rounds(const ShuffleGeometry& g, bool spilled, const std::vector<int64_t>& split_pos,
                        const std::vector<int64_t>& run_off, const std::vector<int64_t>& recv_counts,
                        const std::vector<int64_t>& recv_ck, const std::vector<int64_t>& cell_ck) {
  const int W = g.W, R = g.R, Q = g.Q, M = g.M, me = g.me;
  const int64_t per = g.cells() + 1, rb = g.record_bytes;
  auto pos = [&](int r, int c) { return split_pos[(size_t)r * per + c]; };
  ShufflePlan out;
  out.rounds.assign(Q, ShuffleRoundPlan());
  out.reducer_records.assign(R, 0);
  out.expect_group_ck.assign((size_t)Q * R, 0);
  for (int q = 0; q < Q; ++q) {
    ShuffleRoundPlan& rp = out.rounds[q];
    rp.send.assign(W, {});
    rp.staged_send.assign(W, {});
    rp.staged_recv.assign(W, {});
    rp.self_beg.assign((size_t)R * M, 0);
    rp.self_off.assign((size_t)R * M, 0);
    for (int i = 0; i < R; ++i)
      for (int m = 0; m < M; ++m) {
        rp.self_beg[(size_t)i * M + m] = pos(m * W + me, i * Q + q);
        rp.self_off[(size_t)i * M + m] = run_off[m * W + me] + pos(m * W + me, i * Q + q) * rb;
      }
    for (int p = 0; p < W; ++p) {
      if (p == me) continue;
      for (int i = 0; i < R; ++i)
        for (int m = 0; m < M; ++m) {
          const int r = m * W + p, c = i * Q + q;
          const int64_t cnt = pos(r, c + 1) - pos(r, c);
          if (cnt <= 0) continue;
          rp.send[p].push_back(PlanSlice{run_off[r] + pos(r, c) * rb, cnt * rb, m});
          rp.send_bytes += cnt * rb;
        }
    }
    out.max_send = std::max(out.max_send, rp.send_bytes);
    const int64_t slot_bytes =
        plan_receive(g, spilled, q, recv_counts, recv_ck, cell_ck, rp, &out.expect_group_ck[(size_t)q * R]);
    out.max_slot_bytes = std::max(out.max_slot_bytes, slot_bytes);
    for (int i = 0; i < R; ++i) out.reducer_records[i] += rp.group_recs[i];
    out.max_round_records = std::max(out.max_round_records, rp.recv_records);
    if (W > 1 && spilled) plan_staged_spans(g, rp);
    if (spilled) plan_h2d(g, rp);
  }
  return out;
}

}  // namespace gpu
}  // namespace uda
