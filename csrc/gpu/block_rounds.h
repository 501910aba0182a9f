// The host arithmetic of the streaming block decode (device_reduce_fixed_blocks): which record starts in
// each block of a block-compressed FIXED10 partition, and which blocks, whole records and round-input
// offsets each key-range round takes of each partition. Pure host code (no HIP), so it is tested without
// a device.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace uda {
namespace gpu {

constexpr int64_t kBlockRecordBytes = 104;  // kTeraRecordBytes
constexpr int64_t kBlockKeyEnd = 13;        // kTeraKeyOffset + kTeraKeyBytes: record head and key

// A 10-byte key as the merge kernels compare it (Elem): the first 8 bytes big-endian, the last two in
// the top 16 bits of lo.
struct BlockKey {
  uint64_t hi = 0, lo = 0;
};
inline bool block_key_less(const BlockKey& a, const BlockKey& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

// The non-empty blocks of K streams in stream order: stream k's are [blk0[k], blk0[k + 1]).
struct BlockGeometry {
  std::vector<int64_t> nrec;  // per stream: records (its raw bytes are nrec * 104 + the 2-byte EOF)
  std::vector<int64_t> blk0;  // K + 1
  std::vector<int64_t> rel;   // per block: its first raw byte's offset in its stream
  std::vector<int64_t> raw;   // per block: raw bytes
};

// Per block: the offset in the block of the first record that starts in it, when that record is whole
// in its stream and its 13 bytes of head and key lie inside the block; -1 otherwise.
std::vector<int32_t> block_first_offsets(const BlockGeometry& g);

// The block first-key index: per stream the blocks with first[b] >= 0 and their keys, and all those
// keys sorted (the sample the round bounds are quantiles of).
struct BlockIndex {
  std::vector<std::vector<std::pair<int64_t, BlockKey>>> idx;
  std::vector<BlockKey> samp;
};
// false: the keys of some stream descend (not a sorted run).
bool build_block_index(const BlockGeometry& g, const std::vector<int32_t>& first, const std::vector<BlockKey>& keys,
                       BlockIndex* out);

struct RoundSpan {
  int64_t b0 = 0, b1 = -1;     // blocks [b0, b1]
  int64_t rec0 = 0, rec1 = 0;  // whole records inside, stream record indices
  int64_t in_off = 0;          // decoded byte rel[b0] lands here in the round input
};

struct RoundPlan {
  int Q = 1;
  std::vector<BlockKey> bounds;               // Q - 1: round q takes the keys in [bounds[q - 1], bounds[q])
  std::vector<std::vector<RoundSpan>> spans;  // [round][stream]
  std::vector<int64_t> in_bytes, in_recs;     // per round: input buffer bytes (a multiple of 256), records decoded whole
};

// Rounds of about round_bytes merged bytes. Per round and stream: the blocks from the last one whose
// first key is below the round's low bound to the first one whose first key reaches its high bound, the
// whole records they hold, and an input offset that puts record starts on 16-byte boundaries.
void plan_rounds(const BlockGeometry& g, const BlockIndex& index, int64_t round_bytes, RoundPlan* out);

}  // namespace gpu
}  // namespace uda
