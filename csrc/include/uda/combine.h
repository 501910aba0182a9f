// Reduce-side combiner of the merge (mapred.uda.merge.combine): associative, order-independent folds over
// the values of equal keys, run on the merged order before delivery. The sums are Hadoop's IntSumReducer
// and LongSumReducer (and their VIntWritable / VLongWritable forms); min and max are the other two folds
// over the same value types.
//
// Two records are equal when key_compare(kind, ...) == 0. A group is a maximal run of equal records in the
// merged order. The delivered record of a group is its first record (lowest run, then position), with its
// serialized key bytes, and the group's folded value:
//   sum.int / sum.long   W = 4 / 8 big-endian two's-complement bytes: the sum modulo 2^(8W), Java's wrapping add
//   min.* / max.*        the same W bytes: the signed minimum / maximum
//   sum.vlong            one Hadoop VLong (uda/vint.h, 1..9 bytes) filling the value exactly: the sum modulo
//                        2^64 as a signed long, re-encoded canonically
//   sum.vint             one VInt (1..5 bytes, decoding into int32 range): the sum wrapped to 32 bits and
//                        sign-extended (Java's int add), re-encoded canonically
// A record whose value the op cannot read (not W bytes; for the v ops empty, not the length its first byte
// announces, or out of int32 range under sum.vint) fails the merge. The v ops accept a non-canonical
// encoding, as Hadoop's readVLong does, and always deliver the canonical one, also for a group of one.
//
// Record length never changes under the fixed-width ops. Under the v ops the value, and with it the
// one-byte value-length header (the length is 1..9), is rewritten, so a delivered record can be shorter or
// longer than its group's first record. The bound the device relies on (output capacity, round sizing):
// a combined group never has more bytes than its input records. A group of n >= 2 records drops n - 1
// records of at least 3 bytes each (key-length header, value-length header, one value byte), and its value
// grows by far less: the sum of n values of at most s bytes has fewer than 8 (s - 1) + log2(n) + 1
// magnitude bits, at most two bytes more for n <= 3 (three 1-byte values reach 381, a 3-byte VInt), and never
// more than 8 bytes more, which 3 (n - 1) covers from n = 4 on. A group of one is only re-encoded to canonical form, which is never longer. A single delivered
// record is at most 8 bytes longer than its group's first record.
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

enum class CombineOp : int {
  kNone = 0,
  kSumInt = 1,
  kSumLong = 2,
  kMinInt = 3,
  kMaxInt = 4,
  kMinLong = 5,
  kMaxLong = 6,
  kSumVInt = 7,
  kSumVLong = 8
};

constexpr const char* kCombineAllowed =
    "none, sum.int or sum.long; also min.int, max.int, min.long, max.long, sum.vint, sum.vlong";

// "none" / "" -> kNone, and the op names of the table above; false for anything else.
bool combine_op_from_conf(const std::string& v, CombineOp* op);
const char* combine_op_name(CombineOp op);
// Value width W of a fixed-width op (0 for kNone and for the variable-width ops).
constexpr int combine_value_bytes(CombineOp op) {
  switch (op) {
    case CombineOp::kSumInt: case CombineOp::kMinInt: case CombineOp::kMaxInt: return 4;
    case CombineOp::kSumLong: case CombineOp::kMinLong: case CombineOp::kMaxLong: return 8;
    default: return 0;
  }
}
// The value is one VInt / VLong: its length, and the record's, can change.
constexpr bool combine_variable_width(CombineOp op) { return op == CombineOp::kSumVInt || op == CombineOp::kSumVLong; }
// How far a delivered record can outgrow the longest input record (a 1-byte VLong becoming 9 bytes).
constexpr int combine_record_growth(CombineOp op) { return combine_variable_width(op) ? 8 : 0; }

// True when [val, val + vlen) is a value the op reads: W bytes, or for the v ops one whole VLong (in int32
// range under sum.vint).
bool combine_value_ok(CombineOp op, const uint8_t* val, int64_t vlen);

// "combine sum.int: value of 5 bytes (4 expected), key \"abc\"": the error of a record the op cannot fold;
// under the v ops "(one VInt expected)" / "(one VLong expected)" in place of the byte count.
std::string combine_bad_value_message(CombineOp op, const uint8_t* key, int64_t klen, int64_t vlen);

// Streaming combiner over whole records in merged order.
class StreamCombiner {
 public:
  StreamCombiner(KeyKind kind, CombineOp op) : kind_(kind), op_(op), w_(combine_value_bytes(op)) {}
  // Feed the next merged record. True when it closed the previous group: *out is then that group's
  // record, valid until the next feed() or finish(). Throws UdaError on a value the op cannot read.
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
  std::vector<uint8_t> cur_, done_;  // serialized key followed by room for the value (W, or 9 bytes)
  int32_t cur_klen_ = 0, done_klen_ = 0;
  uint64_t acc_ = 0;  // the fold so far: sums as unsigned bits, min / max as the signed value's bits
  int64_t in_ = 0, groups_ = 0;
};

// Combine a whole IFile stream (records, optional EOF marker) that is already in merged order; the
// result ends with the EOF marker iff the input did.
std::vector<uint8_t> combine_stream(const uint8_t* p, size_t n, KeyKind kind, CombineOp op);

}  // namespace uda
