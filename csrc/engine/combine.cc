// Host reference of the reduce-side combiner. See uda/combine.h.
#include "uda/combine.h"

#include <cstdio>

#include "uda/error.h"

namespace uda {

bool combine_op_from_conf(const std::string& v, CombineOp* op) {
  if (v.empty() || v == "none") {
    *op = CombineOp::kNone;
  } else if (v == "sum.int") {
    *op = CombineOp::kSumInt;
  } else if (v == "sum.long") {
    *op = CombineOp::kSumLong;
  } else {
    return false;
  }
  return true;
}

const char* combine_op_name(CombineOp op) {
  return op == CombineOp::kSumInt ? "sum.int" : op == CombineOp::kSumLong ? "sum.long" : "none";
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
  return "combine " + std::string(combine_op_name(op)) + ": value of " + std::to_string(vlen) + " bytes (" +
         std::to_string(combine_value_bytes(op)) + " expected), key \"" + k + "\" (" + std::to_string(klen) +
         " serialized bytes)";
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
}  // namespace

void StreamCombiner::close(RecordView* out) {
  done_.swap(cur_);
  done_klen_ = cur_klen_;
  store_be(done_.data() + done_klen_, w_, acc_);  // the low 8W bits: the sum modulo 2^(8W)
  out->key = done_.data();
  out->klen = done_klen_;
  out->val = done_.data() + done_klen_;
  out->vlen = w_;
  out->hdr = vint_size(done_klen_) + vint_size(w_);
  open_ = false;
  ++groups_;
}

bool StreamCombiner::feed(const RecordView& r, RecordView* out) {
  if (r.vlen != w_) throw UdaError(combine_bad_value_message(op_, r.key, r.klen, r.vlen));
  ++in_;
  const uint64_t v = load_be(r.val, w_);
  if (open_ && key_compare(kind_, cur_.data(), cur_klen_, r.key, r.klen) == 0) {
    acc_ += v;  // unsigned: wraps like Java's int / long add
    return false;
  }
  const bool closed = open_;
  if (closed) close(out);
  cur_.resize((size_t)r.klen + (size_t)w_);
  if (r.klen) std::memcpy(cur_.data(), r.key, (size_t)r.klen);
  std::memcpy(cur_.data() + r.klen, r.val, (size_t)w_);
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
