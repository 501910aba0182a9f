// Round planning of the shuffle job (ShuffleJob, device_engine.h) as host-only code: index arithmetic
// from the cell splits and the exchanged counts to, per round, receive offsets, send slices, staged
// spans, verification lists and H2D copy lists. Everything is an offset (into the partition store, a
// receive slot or a send staging buffer); the job adds base addresses and uploads. No HIP, no device
// types: tests/native/shuffle_plan_selftest.cc runs it under sanitizers for all ranks of a job at once.
//
// Tables: split_pos[r * (C + 1) + c] is the first record of cell c in run r = m * W + d (map m,
// destination GPU d), C = R * Q cells per GPU, cell c = i * Q + q (reducer i, round q). Tables "per
// (run, cell)" are indexed [r * C + c]. Tables exchanged between ranks are laid out per peer,
// [p][q][i][m] (peer_count()); a round's receive tables per source, [s][i][j] (cell()).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace uda {
namespace gpu {

struct ShuffleGeometry {
  int W = 1;   // ranks (GPUs)
  int R = 1;   // reducers per GPU
  int Q = 1;   // rounds
  int M = 1;   // maps per rank
  int me = 0;  // this rank
  int64_t record_bytes = 104;

  int cells() const { return R * Q; }
  size_t n_per_peer() const { return (size_t)Q * R * M; }
  // a round's receive tables: source rank s, my reducer i, the source's map j
  size_t cell(int s, int i, int j) const { return ((size_t)s * R + i) * M + j; }
  // exchanged tables: peer p, round q, the receiver's reducer i, the sender's map m
  size_t peer_count(int p, int q, int i, int m) const { return (size_t)p * n_per_peer() + ((size_t)q * R + i) * M + m; }
};

struct PlanSlice {  // an outgoing slice: bytes of the partition store, in map `map`'s output
  int64_t store_off;
  int64_t bytes;
  int map;
};
struct PlanSpan {  // a region of a send staging buffer or a receive slot
  int64_t off;
  int64_t bytes;
};
struct PlanVerify {  // a received peer slice and the checksum its sender computed
  int64_t slot_off;
  int64_t nrec;
  int64_t expect;
};
struct PlanOwn {  // an own cell where the merge reads it
  int64_t slot_off;  // in the receive slot; -1: read in place from the store
  int64_t store_off;
  int64_t nrec;
  int64_t expect;
  int map;
};
struct PlanCopy {  // spill tiers: store bytes a round needs in HBM
  int64_t store_off;
  bool to_staging;  // destination: the round's send staging buffer, else its receive slot
  int64_t dst_off;
  int64_t bytes;
  int map;
};

struct ShuffleRoundPlan {
  // send[p]: slices to GPU p, order (reducer i, local map m), empty cells skipped; empty for p == me
  std::vector<std::vector<PlanSlice>> send;
  int64_t send_bytes = 0;
  std::vector<int64_t> recv_cnt;    // [cell(s, i, j)]: records of source s's map j for my reducer i
  std::vector<int64_t> recv_off;    // byte offset of that slice in the receive slot (s-major); -1: in place
  std::vector<int64_t> self_beg;    // [i * M + m]: first record of my own cell (i, q) in run (m, me)
  std::vector<int64_t> self_off;    // [i * M + m]: that record's byte offset in the store (empty cells too)
  std::vector<int64_t> group_recs;  // records per reducer this round
  int64_t recv_records = 0;
  // spill tiers, world > 1: the outgoing slices are staged into HBM, one contiguous region per peer, and
  // travel as one message per peer; the receive side takes them as one span per source (its slices from
  // a source are contiguous in the slot). At most one span per peer; none elsewhere.
  std::vector<std::vector<PlanSpan>> staged_send, staged_recv;
  std::vector<PlanVerify> verify;  // the non-empty peer slices, order (s, i, j)
  std::vector<PlanOwn> own;        // the non-empty own cells, order (i, j)
  // spill tiers: the own cells into the receive slot, then (world > 1) the outgoing slices into the send
  // staging, peer-major, in staged_send's layout; empty when the store is read in place
  std::vector<PlanCopy> h2d;
  int64_t verify_max_nrec = 0, own_max_nrec = 0, h2d_max = 0;  // largest entry of each list
};

struct ShufflePlan {
  std::vector<ShuffleRoundPlan> rounds;
  std::vector<int64_t> reducer_records;   // per reducer, over the rounds
  int64_t max_round_records = 0;
  int64_t max_slot_bytes = 0;             // largest receive-slot layout
  int64_t max_send = 0;                   // largest send_bytes
  std::vector<uint64_t> expect_group_ck;  // [q * R + i]: sum of the input slices' checksums
};

// A per-(run, cell) table in the per-peer layout: out[peer_count(p, q, i, m)] = t[(m * W + p) * C + i * Q + q].
std::vector<int64_t> to_peer_layout(const ShuffleGeometry& g, const std::vector<int64_t>& per_run_cell);

// Records of every (run, cell) slice, per-peer layout: what this rank sends (its own entry included).
std::vector<int64_t> plan_send_counts(const ShuffleGeometry& g, const std::vector<int64_t>& split_pos);

// run_off[r]: byte offset of run r in the store. recv_counts / recv_ck: per-peer layout by source, as the
// counts exchange delivered them (own entry included); own cells are checked against cell_ck, whatever
// recv_ck holds for this rank.
// cell_ck: per (run, cell) checksums of the local runs. spilled: own cells are staged into the receive
// slot (host / disk store), not read in place. Throws std::runtime_error on a layout it cannot stage.
ShufflePlan plan_rounds(const ShuffleGeometry& g, bool spilled, const std::vector<int64_t>& split_pos,
                        const std::vector<int64_t>& run_off, const std::vector<int64_t>& recv_counts,
                        const std::vector<int64_t>& recv_ck, const std::vector<int64_t>& cell_ck);

}  // namespace gpu
}  // namespace uda
