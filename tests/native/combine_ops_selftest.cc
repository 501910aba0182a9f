// Stand-alone self-test of the host combiner's further ops (csrc/engine/combine.cc: min / max over 4- and
// 8-byte values, sums of one VInt / VLong), built with ASan + UBSan by tests/test_combine_ops_cpu.py: exact-size
// heap buffers for every record fed (a VLong must never be read past its value), the closed group's view
// (value length and header bytes of a re-encoded value), every length boundary of the encoding, the wraps,
// non-canonical input, the values a v op refuses, and the KVWriter hook with records that change length.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "uda/combine.h"
#include "uda/error.h"
#include "uda/ifile.h"
#include "uda/vint.h"

using namespace uda;

static int failures = 0;
#define EXPECT(c)                                               \
  do {                                                          \
    if (!(c)) {                                                 \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      ++failures;                                               \
    }                                                           \
  } while (0)

using Rec = std::pair<std::string, std::string>;

static std::string vl(int64_t v) {
  uint8_t b[9];
  const int n = vint_encode(v, b);
  return std::string(reinterpret_cast<char*>(b), (size_t)n);
}
static std::string text_key(const std::string& s) { return vl((int64_t)s.size()) + s; }
static std::string be(uint64_t v, int w) {
  std::string s((size_t)w, '\0');
  for (int i = w - 1; i >= 0; --i) {
    s[(size_t)i] = (char)(uint8_t)v;
    v >>= 8;
  }
  return s;
}
static std::vector<uint8_t> stream_of(const std::vector<Rec>& recs, bool eof) {
  std::vector<uint8_t> out;
  for (const Rec& r : recs)
    ifile_append(&out, reinterpret_cast<const uint8_t*>(r.first.data()), (int32_t)r.first.size(),
                 reinterpret_cast<const uint8_t*>(r.second.data()), (int32_t)r.second.size());
  if (eof) ifile_append_eof(&out);
  return out;
}

// every record fed from its own exact-size heap copy, freed right after the feed
static std::vector<Rec> feed_all(KeyKind kind, CombineOp op, const std::vector<Rec>& in, int64_t* groups) {
  StreamCombiner c(kind, op);
  std::vector<Rec> out;
  RecordView g;
  auto take = [&] {
    EXPECT(g.hdr == vint_size(g.klen) + vint_size(g.vlen));
    EXPECT(g.val == g.key + g.klen);
    out.push_back({std::string(reinterpret_cast<const char*>(g.key), (size_t)g.klen),
                   std::string(reinterpret_cast<const char*>(g.val), (size_t)g.vlen)});
  };
  for (const Rec& r : in) {
    std::unique_ptr<uint8_t[]> k(new uint8_t[r.first.size()]), v(new uint8_t[r.second.size()]);
    std::memcpy(k.get(), r.first.data(), r.first.size());
    std::memcpy(v.get(), r.second.data(), r.second.size());
    RecordView rv;
    rv.key = k.get();
    rv.klen = (int32_t)r.first.size();
    rv.val = v.get();
    rv.vlen = (int32_t)r.second.size();
    const bool closed = c.feed(rv, &g);
    k.reset();
    v.reset();
    if (closed) take();  // the view must not point into the fed record
  }
  if (c.finish(&g)) take();
  EXPECT(!c.finish(&g));
  EXPECT(c.records_in() == (int64_t)in.size());
  *groups = c.groups();
  return out;
}

static bool refuses(CombineOp op, const std::string& value, const char* says) {
  int64_t groups = 0;
  try {
    feed_all(KeyKind::kText, op, {{text_key("ok"), op == CombineOp::kMinInt ? be(1, 4) : vl(1)}, {text_key("bad-key"), value}},
             &groups);
  } catch (const UdaError& e) {
    const std::string w = e.what();
    return w.find(says) != std::string::npos && w.find("bad-key") != std::string::npos;
  }
  return false;
}

int main() {
  int64_t groups = 0;
  {  // conf parser, names, widths
    const struct {
      const char* name;
      CombineOp op;
      int w;
      bool var;
    } ops[] = {{"min.int", CombineOp::kMinInt, 4, false},   {"max.int", CombineOp::kMaxInt, 4, false},
               {"min.long", CombineOp::kMinLong, 8, false}, {"max.long", CombineOp::kMaxLong, 8, false},
               {"sum.vint", CombineOp::kSumVInt, 0, true},  {"sum.vlong", CombineOp::kSumVLong, 0, true}};
    for (const auto& o : ops) {
      CombineOp op = CombineOp::kNone;
      EXPECT(combine_op_from_conf(o.name, &op) && op == o.op);
      EXPECT(std::string(combine_op_name(o.op)) == o.name);
      EXPECT(combine_value_bytes(o.op) == o.w && combine_variable_width(o.op) == o.var);
    }
    CombineOp op;
    EXPECT(!combine_op_from_conf("sum.float", &op) && !combine_op_from_conf("min", &op) &&
           !combine_op_from_conf("SUM.VINT", &op) && !combine_op_from_conf("max.vint", &op));
    EXPECT(!combine_variable_width(CombineOp::kSumInt) && !combine_variable_width(CombineOp::kNone));
    EXPECT(std::string(kCombineAllowed).find("none, sum.int or sum.long") == 0);
  }
  {  // min / max are signed, and keep the first record's key bytes
    const uint64_t lo4 = 0x80000000u, hi4 = 0x7fffffffu, m1 = 0xffffffffu;
    const std::vector<Rec> in = {{text_key("a"), be(m1, 4)},  {text_key("a"), be(0, 4)},   {text_key("b"), be(hi4, 4)},
                                 {text_key("b"), be(lo4, 4)}, {text_key("c"), be(lo4, 4)}, {text_key("d"), be(5, 4)},
                                 {text_key("d"), be(3, 4)},   {text_key("d"), be(4, 4)}};
    std::vector<Rec> out = feed_all(KeyKind::kText, CombineOp::kMinInt, in, &groups);
    EXPECT(groups == 4 && out.size() == 4);
    EXPECT(out[0] == Rec(text_key("a"), be(m1, 4)) && out[1] == Rec(text_key("b"), be(lo4, 4)));
    EXPECT(out[2] == Rec(text_key("c"), be(lo4, 4)) && out[3] == Rec(text_key("d"), be(3, 4)));
    out = feed_all(KeyKind::kText, CombineOp::kMaxInt, in, &groups);
    EXPECT(out[0] == Rec(text_key("a"), be(0, 4)) && out[1] == Rec(text_key("b"), be(hi4, 4)));
    EXPECT(out[2] == Rec(text_key("c"), be(lo4, 4)) && out[3] == Rec(text_key("d"), be(5, 4)));
    const uint64_t lo8 = 1ull << 63, hi8 = ~lo8;
    const std::vector<Rec> in8 = {{text_key("a"), be(~0ull, 8)}, {text_key("a"), be(0, 8)}, {text_key("b"), be(hi8, 8)},
                                  {text_key("b"), be(lo8, 8)},   {text_key("b"), be(7, 8)}};
    out = feed_all(KeyKind::kText, CombineOp::kMinLong, in8, &groups);
    EXPECT(out.size() == 2 && out[0] == Rec(text_key("a"), be(~0ull, 8)) && out[1] == Rec(text_key("b"), be(lo8, 8)));
    out = feed_all(KeyKind::kText, CombineOp::kMaxLong, in8, &groups);
    EXPECT(out.size() == 2 && out[0] == Rec(text_key("a"), be(0, 8)) && out[1] == Rec(text_key("b"), be(hi8, 8)));
  }
  {  // every length boundary of the encoding, reached from 1-byte inputs or a 1-byte head (the record grows)
     // and from long inputs that cancel (it shrinks)
    std::vector<int64_t> edges = {0, -1, -112, -113, 127, 128, INT64_MAX, INT64_MIN};
    for (int k = 1; k < 8; ++k)
      for (int64_t x : {(int64_t)((1ull << (8 * k)) - 1), (int64_t)(1ull << (8 * k))}) {
        edges.push_back(x);
        edges.push_back(x ^ -1ll);
      }
    for (int64_t t : edges) {
      const int64_t one = t > 0 ? 1 : -1;
      const int64_t rest = (int64_t)((uint64_t)t - (uint64_t)one);
      std::vector<Rec> out = feed_all(KeyKind::kText, CombineOp::kSumVLong, {{text_key("k"), vl(one)}, {text_key("k"), vl(rest)}}, &groups);
      EXPECT(out.size() == 1 && out[0] == Rec(text_key("k"), vl(t)));
      const int64_t big = (1ll << 60) + 12345;
      out = feed_all(KeyKind::kText, CombineOp::kSumVLong,
                     {{text_key("k"), vl(big)}, {text_key("k"), vl(-big)}, {text_key("k"), vl(t)}}, &groups);
      EXPECT(out.size() == 1 && out[0] == Rec(text_key("k"), vl(t)));
      if (t >= INT32_MIN && t <= INT32_MAX) {
        out = feed_all(KeyKind::kText, CombineOp::kSumVInt, {{text_key("k"), vl(one)}, {text_key("k"), vl(rest)}}, &groups);
        EXPECT(out.size() == 1 && out[0] == Rec(text_key("k"), vl(t)));
      }
    }
    std::vector<Rec> many(300, Rec(text_key("m"), vl(127)));
    std::vector<Rec> out = feed_all(KeyKind::kText, CombineOp::kSumVInt, many, &groups);
    EXPECT(groups == 1 && out[0] == Rec(text_key("m"), vl(38100)));
  }
  {  // wraps: 2^63 under sum.vlong, 2^31 under sum.vint
    std::vector<Rec> out = feed_all(KeyKind::kText, CombineOp::kSumVLong,
                                    {{text_key("a"), vl(INT64_MAX)}, {text_key("a"), vl(1)}, {text_key("b"), vl(INT64_MIN)},
                                     {text_key("b"), vl(-1)}}, &groups);
    EXPECT(out.size() == 2 && out[0] == Rec(text_key("a"), vl(INT64_MIN)) && out[1] == Rec(text_key("b"), vl(INT64_MAX)));
    out = feed_all(KeyKind::kText, CombineOp::kSumVInt,
                   {{text_key("a"), vl(INT32_MAX)}, {text_key("a"), vl(1)}, {text_key("b"), vl(INT32_MIN)},
                    {text_key("b"), vl(-1)}, {text_key("c"), vl(INT32_MAX)}, {text_key("c"), vl(INT32_MAX)},
                    {text_key("c"), vl(INT32_MAX)}}, &groups);
    EXPECT(out.size() == 3 && out[0] == Rec(text_key("a"), vl(INT32_MIN)) && out[1] == Rec(text_key("b"), vl(INT32_MAX)));
    EXPECT(out[2] == Rec(text_key("c"), vl(INT32_MAX - 2)));
  }
  {  // non-canonical input is read as Hadoop reads it and delivered canonically, a group of one included
    const std::string nc5("\x8f\x05", 2), nc9 = std::string("\x88", 1) + be(7, 8);
    for (CombineOp op : {CombineOp::kSumVInt, CombineOp::kSumVLong}) {
      const std::vector<Rec> out =
          feed_all(KeyKind::kText, op, {{text_key("a"), nc5}, {text_key("b"), nc9}, {text_key("b"), nc5}, {text_key("c"), vl(300)}}, &groups);
      EXPECT(out.size() == 3 && out[0] == Rec(text_key("a"), vl(5)) && out[1] == Rec(text_key("b"), vl(12)));
      EXPECT(out[2] == Rec(text_key("c"), vl(300)));
    }
  }
  {  // the values a v op refuses, and a wrong width under min.int with the fixed-width wording
    EXPECT(refuses(CombineOp::kSumVLong, "", "value of 0 bytes (one VLong expected)"));
    EXPECT(refuses(CombineOp::kSumVLong, std::string("\x8e\x01", 2), "value of 2 bytes (one VLong expected)"));
    EXPECT(refuses(CombineOp::kSumVLong, std::string("\x05\x05", 2), "value of 2 bytes (one VLong expected)"));
    EXPECT(refuses(CombineOp::kSumVInt, vl(1ll << 32), "value of 6 bytes (one VInt expected)"));
    EXPECT(refuses(CombineOp::kSumVInt, vl((int64_t)INT32_MAX + 1), "value of 5 bytes (one VInt expected)"));
    EXPECT(refuses(CombineOp::kSumVInt, vl((int64_t)INT32_MIN - 1), "value of 5 bytes (one VInt expected)"));
    EXPECT(refuses(CombineOp::kMinInt, "12345", "value of 5 bytes (4 expected)"));
    EXPECT(combine_value_ok(CombineOp::kSumVInt, reinterpret_cast<const uint8_t*>("\x8b\0\0\0\0\x05"), 6));  // 5, six bytes
  }
  {  // combine_stream and the KVWriter hook over records that change length, packed into 64-byte buffers
    std::mt19937_64 rng(9);
    std::vector<Rec> in, want;
    for (int g = 0; g < 300; ++g) {
      char name[16];
      std::snprintf(name, sizeof(name), "key%05d", g);
      const int n = 1 + (int)(rng() % 5) * (int)(rng() % 40);
      uint64_t sum = 0;
      for (int j = 0; j < n; ++j) {
        const int64_t v = (int64_t)rng() >> (rng() % 64);  // every encoded length
        sum += (uint64_t)v;
        in.push_back({text_key(name), vl(v)});
      }
      want.push_back({text_key(name), vl((int64_t)sum)});
    }
    for (bool eof : {true, false}) {
      const std::vector<uint8_t> s = stream_of(in, eof);
      std::unique_ptr<uint8_t[]> exact(new uint8_t[s.size()]);
      std::memcpy(exact.get(), s.data(), s.size());
      EXPECT(combine_stream(exact.get(), s.size(), KeyKind::kText, CombineOp::kSumVLong) == stream_of(want, eof));
    }
    std::vector<std::vector<Rec>> parts(4);
    for (size_t i = 0; i < in.size(); ++i) parts[i % 4].push_back(in[i]);
    MergeQueue q(KeyKind::kText);
    for (int p = 0; p < 4; ++p) {
      auto seg = std::make_unique<MemorySegment>(stream_of(parts[(size_t)p], p % 2 == 0));
      seg->index = p;
      q.insert(std::move(seg));
    }
    KVWriter w(&q, KeyKind::kText, CombineOp::kSumVLong);
    std::vector<uint8_t> all;
    bool done = false;
    int buffers = 0;
    while (!done) {
      std::unique_ptr<uint8_t[]> buf(new uint8_t[64]);
      int64_t len = 0;
      done = w.fill(buf.get(), 64, &len);
      EXPECT(len <= 64);
      all.insert(all.end(), buf.get(), buf.get() + len);
      ++buffers;
    }
    EXPECT(buffers > 10 && w.records_in() == (int64_t)in.size() && w.records() == (int64_t)want.size());
    EXPECT(all == stream_of(want, true));
  }
  std::printf("combine ops selftest: %d failures\n", failures);
  return failures ? 1 : 0;
}
