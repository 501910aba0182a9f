// Reduce-side combiner of the merge (mapred.uda.merge.combine): the two built-in Hadoop sum combiners,
// IntSumReducer and LongSumReducer, run on the merged order before delivery.
//
// Two records are equal when key_compare(kind, ...) == 0. A group is a maximal run of equal records in the
// merged order. The delivered record of a group is its first record (lowest run, then position) with its
// value, W big-endian two's-complement bytes, replaced by the group's sum modulo 2^(8W): Java's wrapping
// add. Record length never changes. A record whose value is not W bytes long fails the merge.
//
// StreamCombiner is the host reference: the CPU backend's implementation (KVWriter) and the oracle of
// the device kernels (gpu/combine.hip).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "uda/compare.h"
#include "uda/ifile.h"

namespace uda {

enum class CombineOp : int { kNone = 0, kSumInt = 1, kSumLong = 2 };

constexpr const char* kCombineAllowed = "none, sum.int or sum.long";

// "none" / "" -> kNone, "sum.int", "sum.long"; false for anything else.
bool combine_op_from_conf(const std::string& v, CombineOp* op);
const char* combine_op_name(CombineOp op);
// Value width W of the op (0 for kNone).
inline int combine_value_bytes(CombineOp op) { return op == CombineOp::kSumInt ? 4 : op == CombineOp::kSumLong ? 8 : 0; }

// "value of 5 bytes under sum.int (4 expected), key \"abc\"": the error of a record the op cannot sum.
std::string combine_bad_value_message(CombineOp op, const uint8_t* key, int64_t klen, int64_t vlen);

// Streaming combiner over whole records in merged order.
class StreamCombiner {
 public:
  StreamCombiner(KeyKind kind, CombineOp op) : kind_(kind), op_(op), w_(combine_value_bytes(op)) {}
  // Feed the next merged record. True when it closed the previous group: *out is then that group's
  // record, valid until the next feed() or finish(). Throws UdaError on a value that is not W bytes.
  bool feed(const RecordView& r, RecordView* out);
  // After the last record: the open group's record, if any.
  bool finish(RecordView* out);
  int64_t records_in() const { return in_; }
  int64_t groups() const { return groups_; }

 private:
  void close(RecordView* out);
  KeyKind kind_;
  CombineOp op_;
  int w_;
  bool open_ = false;
  std::vector<uint8_t> cur_, done_;  // serialized key followed by the W value bytes
  int32_t cur_klen_ = 0, done_klen_ = 0;
  uint64_t acc_ = 0;
  int64_t in_ = 0, groups_ = 0;
};

// Combine a whole IFile stream (records, optional EOF marker) that is already in merged order; the
// result ends with the EOF marker iff the input did.
std::vector<uint8_t> combine_stream(const uint8_t* p, size_t n, KeyKind kind, CombineOp op);

}  // namespace uda
