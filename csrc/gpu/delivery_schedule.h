// The D2H pieces of one delivery round and the order the copy thread issues them in. Pure host code
// (no HIP): the one enumeration behind ShuffleJob::round_pieces(), the device piece descriptors and
// copy_loop.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace uda {
namespace gpu {

struct DeliveryPiece {
  int reducer;
  int64_t src_off;       // bytes into the round's output slot (reducers laid out back to back)
  int64_t len;           // bytes: whole records, at most the piece size
  int pack_index;        // position in the reducer-major enumeration (round_pieces(), the device descriptors)
  bool last_of_reducer;  // this reducer's final piece of the round
};

// "reducer" or "wave"; anything else throws.
void check_delivery_order(const std::string& order);

// group_recs[i]: records of reducer i this round. piece_bytes is rounded down to whole records (at
// least one). Order "reducer": every piece of reducer 0, then of reducer 1, ... "wave": piece 0 of
// every reducer that has one, in reducer order, then piece 1 of every reducer that has one, ... so
// every consumer gets work at once and a round ends on the reducers' short remainder pieces. Within a
// reducer the offsets ascend in both orders.
std::vector<DeliveryPiece> delivery_schedule(const std::vector<int64_t>& group_recs, int64_t piece_bytes,
                                             const std::string& order, int64_t record_bytes = 104);

}  // namespace gpu
}  // namespace uda
