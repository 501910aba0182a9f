// Host reference of the reduce-side combiner. See uda/combine.h.
#include "uda/combine.h"

#include <cstdio>

#include "uda/error.h"
#include "uda/vint.h"

namespace uda {

namespace {
constexpr struct {
  const char* name;
  CombineOp op;
} kOps[] = {{"sum.int", CombineOp::kSumInt},   {"sum.long", CombineOp::kSumLong}, {"min.int", CombineOp::kMinInt},
            {"max.int", CombineOp::kMaxInt},   {"min.long", CombineOp::kMinLong}, {"max.long", CombineOp::kMaxLong},
            {"sum.vint", CombineOp::kSumVInt}, {"sum.vlong", CombineOp::kSumVLong}};
}  // namespace

bool combine_op_from_conf(const std::string& v, CombineOp* op) {
  if (v.empty() || v == "none") {
    *op = CombineOp::kNone;
    return true;
  }
  for (const auto& o : kOps)
    if (v == o.name) {
      *op = o.op;
      return true;
    }
  return false;
}

const char* combine_op_name(CombineOp op) {
  for (const auto& o : kOps)
    if (op == o.op) return o.name;
  return "none";
}

bool combine_value_ok(CombineOp op, const uint8_t* val, int64_t vlen) {
  if (!combine_variable_width(op)) return vlen == combine_value_bytes(op);
  if (vlen < 1 || vlen != vint_decode_size((int8_t)val[0])) return false;
  if (op == CombineOp::kSumVLong) return true;
  int64_t v = 0;
  vint_decode(val, (size_t)vlen, &v);
  return v >= INT32_MIN && v <= INT32_MAX;
}

std::string combine_bad_value_message(CombineOp op, const uint8_t* key, int64_t klen, int64_t vlen) {
  std::string k;
  const int64_t shown = klen < 64 ? klen : 64;
  for (int64_t i = 0; i < shown; ++i) {
    const uint8_t c = key[i];
    if (c >= 0x20 && c < 0x7F && c != '"' && c != '\\') {
      k.push_back((char)c);
    } else {
      char esc[8];
      snprintf(esc, sizeof(esc), "\\x%02x", (unsigned)c);
      k += esc;
    }
  }
  if (shown < klen) k += "...";
  const std::string expected = op == CombineOp::kSumVInt    ? "one VInt"
                               : op == CombineOp::kSumVLong ? "one VLong"
                                                            : std::to_string(combine_value_bytes(op));
  return "combine " + std::string(combine_op_name(op)) + ": value of " + std::to_string(vlen) + " bytes (" + expected +
         " expected), key \"" + k + "\" (" + std::to_string(klen) + " serialized bytes)";
}

namespace {
uint64_t load_be(const uint8_t* p, int w) {
  uint64_t v = 0;
  for (int i = 0; i < w; ++i) v = (v << 8) | p[i];
  return v;
}
void store_be(uint8_t* p, int w, uint64_t v) {
  for (int i = w - 1; i >= 0; --i) {
    p[i] = (uint8_t)v;
    v >>= 8;
  }
}
// The value as the fold sees it: sums take the bits (a VLong's are its signed value's), min / max the
// sign-extended value.
uint64_t load_value(CombineOp op, const uint8_t* p, int64_t vlen) {
  switch (op) {
    case CombineOp::kSumVInt:
    case CombineOp::kSumVLong: {
      int64_t v = 0;
      vint_decode(p, (size_t)vlen, &v);
      return (uint64_t)v;
    }
    case CombineOp::kMinInt:
    case CombineOp::kMaxInt:
      return (uint64_t)(int64_t)(int32_t)(uint32_t)load_be(p, 4);
    default:
      return load_be(p, (int)vlen);
  }
}
uint64_t fold(CombineOp op, uint64_t a, uint64_t b) {
  switch (op) {
    case CombineOp::kMinInt:
    case CombineOp::kMinLong:
      return (int64_t)b < (int64_t)a ? b : a;
    case CombineOp::kMaxInt:
    case CombineOp::kMaxLong:
      return (int64_t)b > (int64_t)a ? b : a;
    default:
      return a + b;  // unsigned: wraps like Java's int / long add
  }
}
}  // namespace

void StreamCombiner::close(RecordView* out) {
  done_.swap(cur_);
  done_klen_ = cur_klen_;
  int vlen = w_;
  if (op_ == CombineOp::kSumVInt) {
    vlen = vint_encode((int64_t)(int32_t)(uint32_t)acc_, done_.data() + done_klen_);  // Java's int add
  } else if (op_ == CombineOp::kSumVLong) {
    vlen = vint_encode((int64_t)acc_, done_.data() + done_klen_);
  } else {
    store_be(done_.data() + done_klen_, w_, acc_);  // the low 8W bits: the sum modulo 2^(8W), or the extreme
  }
  out->key = done_.data();
  out->klen = done_klen_;
  out->val = done_.data() + done_klen_;
  out->vlen = vlen;
  out->hdr = vint_size(done_klen_) + vint_size(vlen);
  open_ = false;
  ++groups_;
}

bool StreamCombiner::feed(const RecordView& r, RecordView* out) {
  if (!combine_value_ok(op_, r.val, r.vlen)) throw UdaError(combine_bad_value_message(op_, r.key, r.klen, r.vlen));
  ++in_;
  const uint64_t v = load_value(op_, r.val, r.vlen);
  if (open_ && key_compare(kind_, cur_.data(), cur_klen_, r.key, r.klen) == 0) {
    acc_ = fold(op_, acc_, v);
    return false;
  }
  const bool closed = open_;
  if (closed) close(out);
  cur_.resize((size_t)r.klen + (size_t)(w_ ? w_ : 9));  // close() writes the value: W bytes, or a VLong's 9 at most
  if (r.klen) std::memcpy(cur_.data(), r.key, (size_t)r.klen);
  cur_klen_ = r.klen;
  acc_ = v;
  open_ = true;
  return closed;
}

bool StreamCombiner::finish(RecordView* out) {
  if (!open_) return false;
  close(out);
  return true;
}

std::vector<uint8_t> combine_stream(const uint8_t* p, size_t n, KeyKind kind, CombineOp op) {
  std::vector<uint8_t> out;
  if (op == CombineOp::kNone) {
    out.assign(p, p + n);
    return out;
  }
  StreamCombiner c(kind, op);
  RecordView r, g;
  size_t pos = 0;
  bool eof = false;
  while (pos < n) {
    const Parse s = ifile_parse(p + pos, n - pos, &r);
    if (s == Parse::kEof) {
      eof = true;
      break;
    }
    if (s != Parse::kRecord) throw UdaError("corrupt or truncated IFile stream");
    pos += (size_t)r.size();
    if (c.feed(r, &g)) ifile_append(&out, g.key, g.klen, g.val, g.vlen);
  }
  if (c.finish(&g)) ifile_append(&out, g.key, g.klen, g.val, g.vlen);
  if (eof) ifile_append_eof(&out);
  return out;
}

}  // namespace uda
