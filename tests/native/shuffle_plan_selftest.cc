// Self-test of the shuffle job's host-only round planner (csrc/gpu/shuffle_plan.cc): all W ranks of a job
// are simulated in one process from random split tables, and every rank's plan is compared with a
// brute-force oracle that never uses the planner's index helper (it numbers table entries by counting
// them in nested-loop order). Built and run by tests/test_shuffle_plan_cpu.py under ASan + UBSan.
#include <cstdint>
#include <cstdio>
#include <random>
#include <stdexcept>
#include <vector>

#include "shuffle_plan.h"

using namespace uda::gpu;

static long g_checks = 0, g_failures = 0;
#define CHECK(c)                                                              \
  do {                                                                        \
    ++g_checks;                                                               \
    if (!(c)) {                                                               \
      if (++g_failures <= 20) std::printf("FAIL %s:%d: %s [%s]\n", __FILE__, __LINE__, #c, g_ctx); \
    }                                                                         \
  } while (0)
static char g_ctx[160] = "";

namespace {
constexpr int64_t kRec = 104;

enum Feature { kZeroRun = 1, kEmptyCell = 2, kEmptyLastRound = 4, kSilentPeer = 8, kSparse = 16 };

struct Job {
  int W, R, Q, M;
  // per rank a: split[a][r * (C + 1) + c], run_off[a][r], ck[a][r * C + c]
  std::vector<std::vector<int64_t>> split, run_off, ck;
  int C() const { return R * Q; }
  // records / checksum / first record of rank a's map m for GPU d, reducer i, round q
  int64_t beg(int a, int m, int d, int i, int q) const { return split[a][(size_t)(m * W + d) * (C() + 1) + i * Q + q]; }
  int64_t cnt(int a, int m, int d, int i, int q) const {
    return split[a][(size_t)(m * W + d) * (C() + 1) + i * Q + q + 1] - beg(a, m, d, i, q);
  }
  int64_t sum(int a, int m, int d, int i, int q) const { return ck[a][(size_t)(m * W + d) * C() + i * Q + q]; }
  int64_t run_records(int a, int m, int d) const { return split[a][(size_t)(m * W + d) * (C() + 1) + C()]; }
};

Job make_job(int W, int R, int Q, int M, int features, std::mt19937_64& rng) {
  Job j{W, R, Q, M, {}, {}, {}};
  const int C = j.C(), nruns = M * W;
  j.split.assign(W, std::vector<int64_t>((size_t)nruns * (C + 1), 0));
  j.run_off.assign(W, std::vector<int64_t>(nruns, 0));
  j.ck.assign(W, std::vector<int64_t>((size_t)nruns * C, 0));
  const int empty_cell = (int)(rng() % (uint64_t)C);
  for (int a = 0; a < W; ++a) {
    int64_t off = 0;
    for (int m = 0; m < M; ++m) {
      for (int d = 0; d < W; ++d) {
        const int r = m * W + d;
        int64_t at = 0;
        for (int c = 0; c < C; ++c) {
          int64_t n = (int64_t)(rng() % 7);
          if ((features & kSparse) && rng() % 3) n = 0;
          if ((features & kZeroRun) && r == 0) n = 0;
          if ((features & kEmptyCell) && c == empty_cell) n = 0;
          if ((features & kEmptyLastRound) && c == (R - 1) * Q + (Q - 1)) n = 0;
          if ((features & kSilentPeer) && a == 0 && d == W - 1) n = 0;
          j.split[a][(size_t)r * (C + 1) + c] = at;
          j.ck[a][(size_t)r * C + c] = n ? (int64_t)rng() : 0;
          at += n;
        }
        j.split[a][(size_t)r * (C + 1) + C] = at;
        j.run_off[a][r] = off;
        off = (off + at * kRec + 2 + 15) / 16 * 16;
      }
      off = (off + 255) / 256 * 256;
    }
  }
  return j;
}

// What rank b receives: block s of the result is block b of rank s's send table (an all-to-all).
std::vector<int64_t> alltoall(const std::vector<std::vector<int64_t>>& send, int b, size_t n) {
  std::vector<int64_t> recv(send.size() * n);
  for (size_t s = 0; s < send.size(); ++s)
    for (size_t k = 0; k < n; ++k) recv[s * n + k] = send[s][(size_t)b * n + k];
  return recv;
}

void check_round(const Job& j, int b, bool spilled, int q, const ShufflePlan& plan, int64_t* reducer_total,
                 int64_t* max_round, int64_t* max_slot, int64_t* max_send) {
  const int W = j.W, R = j.R, M = j.M;
  const ShuffleRoundPlan& rp = plan.rounds[q];
  CHECK(rp.recv_cnt.size() == (size_t)W * R * M && rp.recv_off.size() == rp.recv_cnt.size());
  CHECK(rp.group_recs.size() == (size_t)R && rp.self_beg.size() == (size_t)R * M && rp.self_off.size() == rp.self_beg.size());
  CHECK(rp.send.size() == (size_t)W && rp.staged_send.size() == (size_t)W && rp.staged_recv.size() == (size_t)W);
  if (g_failures) return;

  // ---- receive side: entries numbered by counting them in (s, i, j) order
  std::vector<int64_t> group(R, 0);
  std::vector<uint64_t> group_ck(R, 0);
  size_t x = 0, nverify = 0, nown = 0;
  int64_t off = 0, records = 0;
  std::vector<int64_t> src_first(W, -1), src_bytes(W, 0);
  for (int s = 0; s < W; ++s)
    for (int i = 0; i < R; ++i)
      for (int m = 0; m < M; ++m, ++x) {
        const int64_t n = j.cnt(s, m, b, i, q);
        CHECK(rp.recv_cnt[x] == n);
        group[i] += n;
        group_ck[i] += (uint64_t)j.sum(s, m, b, i, q);
        const bool in_place = s == b && !spilled;
        CHECK((rp.recv_off[x] == -1) == in_place);
        if (!in_place) {  // source-major, contiguous, no overlap: each slice starts where the last ended
          CHECK(rp.recv_off[x] == off);
          if (n > 0 && src_first[s] < 0) src_first[s] = off;
          src_bytes[s] += n * kRec;
          off += n * kRec;
        }
        if (n <= 0) continue;
        if (s == b) {
          CHECK(nown < rp.own.size());
          if (nown < rp.own.size()) {
            const PlanOwn& o = rp.own[nown];
            CHECK(o.slot_off == (in_place ? -1 : rp.recv_off[x]) && o.nrec == n && o.expect == j.sum(b, m, b, i, q));
            CHECK(o.store_off == j.run_off[b][m * W + b] + j.beg(b, m, b, i, q) * kRec && o.map == m);
          }
          ++nown;
        } else {
          CHECK(nverify < rp.verify.size());
          if (nverify < rp.verify.size()) {
            const PlanVerify& v = rp.verify[nverify];
            CHECK(v.slot_off == rp.recv_off[x] && v.nrec == n && v.expect == j.sum(s, m, b, i, q));
          }
          ++nverify;
        }
      }
  CHECK(nown == rp.own.size() && nverify == rp.verify.size());
  int64_t vmax = 0, omax = 0;
  for (const PlanVerify& v : rp.verify) vmax = v.nrec > vmax ? v.nrec : vmax;
  for (const PlanOwn& o : rp.own) omax = o.nrec > omax ? o.nrec : omax;
  CHECK(rp.verify_max_nrec == vmax && rp.own_max_nrec == omax);
  for (int i = 0; i < R; ++i) {
    CHECK(rp.group_recs[i] == group[i]);
    CHECK(plan.expect_group_ck[(size_t)q * R + i] == group_ck[i]);
    for (int m = 0; m < M; ++m) {
      CHECK(rp.self_beg[(size_t)i * M + m] == j.beg(b, m, b, i, q));
      CHECK(rp.self_off[(size_t)i * M + m] == j.run_off[b][m * W + b] + j.beg(b, m, b, i, q) * kRec);
    }
    records += group[i];
    reducer_total[i] += group[i];
  }
  CHECK(rp.recv_records == records);
  if (records > *max_round) *max_round = records;
  if (off > *max_slot) *max_slot = off;

  // ---- send side: per peer in (reducer, map) order, empty cells skipped, inside their run
  int64_t send_bytes = 0, staged = 0;
  std::vector<PlanCopy> want_h2d;
  if (spilled)
    for (const PlanOwn& o : rp.own) want_h2d.push_back(PlanCopy{o.store_off, false, o.slot_off, o.nrec * kRec, o.map});
  for (int p = 0; p < W; ++p) {
    size_t k = 0;
    int64_t peer_bytes = 0;
    if (p != b)
      for (int i = 0; i < R; ++i)
        for (int m = 0; m < M; ++m) {
          const int64_t n = j.cnt(b, m, p, i, q);
          if (n <= 0) continue;
          CHECK(k < rp.send[p].size());
          if (k < rp.send[p].size()) {
            const PlanSlice& sl = rp.send[p][k];
            const int64_t run = j.run_off[b][m * W + p];
            CHECK(sl.store_off == run + j.beg(b, m, p, i, q) * kRec && sl.bytes == n * kRec && sl.map == m);
            CHECK(sl.store_off >= run && sl.store_off + sl.bytes <= run + j.run_records(b, m, p) * kRec);
            if (spilled) want_h2d.push_back(PlanCopy{sl.store_off, true, staged + peer_bytes, sl.bytes, m});
          }
          peer_bytes += n * kRec;
          ++k;
        }
    CHECK(k == rp.send[p].size());
    // the staged send span of a peer is the concatenation of its slices; the staged receive span of a
    // source covers exactly that source's slices
    const bool stage = spilled && W > 1;
    CHECK(rp.staged_send[p].size() == (stage && peer_bytes > 0 ? 1u : 0u));
    if (rp.staged_send[p].size() == 1) CHECK(rp.staged_send[p][0].off == staged && rp.staged_send[p][0].bytes == peer_bytes);
    const bool recv_span = stage && p != b && src_bytes[p] > 0;
    CHECK(rp.staged_recv[p].size() == (recv_span ? 1u : 0u));
    if (rp.staged_recv[p].size() == 1)
      CHECK(rp.staged_recv[p][0].off == src_first[p] && rp.staged_recv[p][0].bytes == src_bytes[p]);
    staged += peer_bytes;
    send_bytes += peer_bytes;
  }
  CHECK(rp.send_bytes == send_bytes);
  if (send_bytes > *max_send) *max_send = send_bytes;

  // ---- H2D list: the own cells and (W > 1) every send slice, each once, staging offsets as staged above;
  // nothing when the store is read in place
  CHECK(rp.h2d.size() == want_h2d.size());
  int64_t hmax = 0;
  for (size_t k = 0; k < rp.h2d.size() && k < want_h2d.size(); ++k) {
    const PlanCopy &c = rp.h2d[k], &w = want_h2d[k];
    CHECK(c.store_off == w.store_off && c.to_staging == w.to_staging && c.dst_off == w.dst_off && c.bytes == w.bytes &&
          c.map == w.map);
    hmax = c.bytes > hmax ? c.bytes : hmax;
  }
  CHECK(rp.h2d_max == hmax);
}

void check_job(const Job& j, bool spilled) {
  const int W = j.W, R = j.R, Q = j.Q, M = j.M;
  std::vector<std::vector<int64_t>> send(W), send_ck(W);
  std::vector<ShuffleGeometry> geo(W);
  for (int a = 0; a < W; ++a) {
    geo[a] = ShuffleGeometry{W, R, Q, M, a, kRec};
    send[a] = plan_send_counts(geo[a], j.split[a]);
    send_ck[a] = to_peer_layout(geo[a], j.ck[a]);
    CHECK(send[a].size() == (size_t)W * Q * R * M && send_ck[a].size() == send[a].size());
  }
  const size_t n = (size_t)Q * R * M;
  // rank a's send counts to b equal b's receive counts from a, entry by entry, and both are the oracle's
  for (int a = 0; a < W; ++a)
    for (int b = 0; b < W; ++b) {
      const std::vector<int64_t> recv = alltoall(send, b, n);
      size_t k = 0;
      for (int q = 0; q < Q; ++q)
        for (int i = 0; i < R; ++i)
          for (int m = 0; m < M; ++m, ++k) {
            CHECK(send[a][(size_t)b * n + k] == j.cnt(a, m, b, i, q));
            CHECK(recv[(size_t)a * n + k] == send[a][(size_t)b * n + k]);
            CHECK(send_ck[a][(size_t)b * n + k] == j.sum(a, m, b, i, q));
          }
    }
  for (int b = 0; b < W; ++b) {
    std::vector<int64_t> recv_ck = alltoall(send_ck, b, n);
    // the own entry of the exchanged checksums is not what the plan may rely on
    for (size_t k = 0; k < n; ++k) recv_ck[(size_t)b * n + k] = 0x5a5a5a5a;
    const ShufflePlan plan = plan_rounds(geo[b], spilled, j.split[b], j.run_off[b], alltoall(send, b, n), recv_ck, j.ck[b]);
    CHECK(plan.rounds.size() == (size_t)Q && plan.reducer_records.size() == (size_t)R);
    CHECK(plan.expect_group_ck.size() == (size_t)Q * R);
    if (g_failures) return;
    std::vector<int64_t> reducer_total(R, 0);
    int64_t max_round = 0, max_slot = 0, max_send = 0;
    for (int q = 0; q < Q; ++q) {
      std::snprintf(g_ctx, sizeof(g_ctx), "W=%d R=%d Q=%d M=%d spilled=%d rank=%d round=%d", W, R, Q, M, (int)spilled, b, q);
      check_round(j, b, spilled, q, plan, reducer_total.data(), &max_round, &max_slot, &max_send);
    }
    for (int i = 0; i < R; ++i) CHECK(plan.reducer_records[i] == reducer_total[i]);
    CHECK(plan.max_round_records == max_round && plan.max_slot_bytes == max_slot && plan.max_send == max_send);
  }
}

// The index helper itself: both functions number their tables densely in nested-loop order.
void check_geometry() {
  const ShuffleGeometry g{3, 2, 5, 3, 1, kRec};
  size_t x = 0;
  for (int s = 0; s < g.W; ++s)
    for (int i = 0; i < g.R; ++i)
      for (int m = 0; m < g.M; ++m) CHECK(g.cell(s, i, m) == x++);
  x = 0;
  for (int p = 0; p < g.W; ++p)
    for (int q = 0; q < g.Q; ++q)
      for (int i = 0; i < g.R; ++i)
        for (int m = 0; m < g.M; ++m) CHECK(g.peer_count(p, q, i, m) == x++);
  CHECK(g.n_per_peer() == 30 && g.cells() == 10);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20240607);
  check_geometry();
  const int features[] = {0, kZeroRun, kEmptyCell, kEmptyLastRound, kSilentPeer, kSparse,
                          kZeroRun | kEmptyCell | kEmptyLastRound | kSilentPeer | kSparse};
  for (int W : {1, 2, 3})
    for (int R : {1, 2, 3})
      for (int Q : {1, 2, 5})
        for (int M : {1, 3})
          for (int f : features)
            for (int spilled = 0; spilled < 2; ++spilled) {
              const Job j = make_job(W, R, Q, M, f, rng);
              check_job(j, spilled != 0);
            }
  std::printf("%ld checks, %ld failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
