// Stand-alone self-test of the host combiner (csrc/engine/combine.cc), built with ASan + UBSan by
// tests/test_combine_cpu.py: exact-size heap buffers for every record fed, the streaming contract
// (a closed group's view stays valid until the next feed), wrap-around, comparator equality per key
// class, the KVWriter hook over a MergeQueue with small buffers, and the wrong-length error.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "uda/combine.h"
#include "uda/error.h"
#include "uda/ifile.h"

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

static std::string text_key(const std::string& s) {
  uint8_t b[9];
  const int n = vint_encode((int64_t)s.size(), b);
  return std::string(reinterpret_cast<char*>(b), (size_t)n) + s;
}
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
static std::vector<Rec> records_of(const std::vector<uint8_t>& s) {
  std::vector<Rec> out;
  size_t pos = 0;
  RecordView r;
  while (pos < s.size() && ifile_parse(s.data() + pos, s.size() - pos, &r) == Parse::kRecord) {
    out.push_back({std::string(reinterpret_cast<const char*>(r.key), (size_t)r.klen),
                   std::string(reinterpret_cast<const char*>(r.val), (size_t)r.vlen)});
    pos += (size_t)r.size();
  }
  return out;
}

// every record fed from its own exact-size heap copy, freed right after the feed
static std::vector<Rec> feed_all(KeyKind kind, CombineOp op, const std::vector<Rec>& in, int64_t* groups) {
  StreamCombiner c(kind, op);
  std::vector<Rec> out;
  RecordView g;
  auto take = [&] {
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

int main() {
  int64_t groups = 0;
  {  // conf parser
    CombineOp op = CombineOp::kSumLong;
    EXPECT(combine_op_from_conf("none", &op) && op == CombineOp::kNone);
    EXPECT(combine_op_from_conf("", &op) && op == CombineOp::kNone);
    EXPECT(combine_op_from_conf("sum.int", &op) && op == CombineOp::kSumInt && combine_value_bytes(op) == 4);
    EXPECT(combine_op_from_conf("sum.long", &op) && op == CombineOp::kSumLong && combine_value_bytes(op) == 8);
    EXPECT(!combine_op_from_conf("sum", &op) && !combine_op_from_conf("SUM.INT", &op));
    EXPECT(combine_value_bytes(CombineOp::kNone) == 0);
  }
  {  // wrap-around and the first record's key bytes
    const std::vector<Rec> in = {{text_key("a"), be(0x7fffffffu, 4)}, {text_key("a"), be(1, 4)},
                                 {text_key("b"), be(0x80000000u, 4)}, {text_key("b"), be(0x80000000u, 4)},
                                 {text_key("c"), be(0xfffffffbu, 4)}};
    const std::vector<Rec> out = feed_all(KeyKind::kText, CombineOp::kSumInt, in, &groups);
    EXPECT(groups == 3 && out.size() == 3);
    EXPECT(out[0] == Rec(text_key("a"), be(0x80000000u, 4)));
    EXPECT(out[1] == Rec(text_key("b"), be(0, 4)));
    EXPECT(out[2] == Rec(text_key("c"), be(0xfffffffbu, 4)));
  }
  {  // sum.long
    const std::vector<Rec> in = {{text_key("k"), be(0x7fffffffffffffffull, 8)}, {text_key("k"), be(1, 8)},
                                 {text_key("k"), be(~0ull, 8)}};
    const std::vector<Rec> out = feed_all(KeyKind::kText, CombineOp::kSumLong, in, &groups);
    EXPECT(groups == 1 && out.size() == 1 && out[0] == Rec(text_key("k"), be(0x7fffffffffffffffull, 8)));
  }
  {  // equality is the comparator's: a Text key with a non-canonical (5-byte) length prefix equals the
     // canonical one and the group keeps the first record's serialized bytes; raw keys compare whole
    std::string wide = std::string("\x8c", 1) + std::string("\0\0\0\x01", 4) + "a";  // VInt -116: 4 length bytes
    const std::vector<Rec> in = {{wide, be(2, 4)}, {text_key("a"), be(3, 4)},
                                 {text_key(std::string("a\0", 2)), be(4, 4)}};
    const std::vector<Rec> out = feed_all(KeyKind::kText, CombineOp::kSumInt, in, &groups);
    EXPECT(groups == 2 && out.size() == 2 && out[0] == Rec(wide, be(5, 4)));
    const std::vector<Rec> raw = {{be(7, 4), be(1, 4)}, {be(7, 4), be(1, 4)}, {be(8, 4), be(1, 4)}};
    EXPECT(feed_all(KeyKind::kRaw, CombineOp::kSumInt, raw, &groups).size() == 2);
    const std::vector<Rec> byt = {{be(0, 4), be(1, 4)}, {be(0, 4), be(9, 4)}, {be(1, 4) + "x", be(1, 4)}};
    const std::vector<Rec> bo = feed_all(KeyKind::kBytes, CombineOp::kSumInt, byt, &groups);
    EXPECT(bo.size() == 2 && bo[0] == Rec(be(0, 4), be(10, 4)));
  }
  {  // a value of the wrong length names the key and the length
    bool threw = false;
    try {
      feed_all(KeyKind::kText, CombineOp::kSumInt, {{text_key("ok"), be(1, 4)}, {text_key("bad-key"), "12345"}}, &groups);
    } catch (const UdaError& e) {
      threw = true;
      const std::string w = e.what();
      EXPECT(w.find("value of 5 bytes") != std::string::npos && w.find("bad-key") != std::string::npos);
    }
    EXPECT(threw);
  }
  {  // combine_stream against a plain map, EOF kept iff present, none = identity
    std::mt19937 rng(5);
    std::vector<Rec> in;
    std::vector<Rec> want;
    for (int g = 0; g < 300; ++g) {
      char name[16];
      std::snprintf(name, sizeof(name), "key%05d", g);
      const int n = 1 + (int)(rng() % 5) * (int)(rng() % 40);
      uint32_t sum = 0;
      for (int j = 0; j < n; ++j) {
        const uint32_t v = (uint32_t)rng();
        sum += v;
        in.push_back({text_key(name), be(v, 4)});
      }
      want.push_back({text_key(name), be(sum, 4)});
    }
    for (bool eof : {true, false}) {
      const std::vector<uint8_t> s = stream_of(in, eof);
      std::unique_ptr<uint8_t[]> exact(new uint8_t[s.size()]);
      std::memcpy(exact.get(), s.data(), s.size());
      const std::vector<uint8_t> out = combine_stream(exact.get(), s.size(), KeyKind::kText, CombineOp::kSumInt);
      EXPECT(out == stream_of(want, eof));
      EXPECT(combine_stream(exact.get(), s.size(), KeyKind::kText, CombineOp::kNone) == s);
    }
    EXPECT(combine_stream(nullptr, 0, KeyKind::kText, CombineOp::kSumInt).empty());
    // the KVWriter hook: the same records dealt over 4 segments, packed into 64-byte buffers
    std::vector<std::vector<Rec>> parts(4);
    for (size_t i = 0; i < in.size(); ++i) parts[i % 4].push_back(in[i]);
    for (CombineOp op : {CombineOp::kSumInt, CombineOp::kNone}) {
      MergeQueue q(KeyKind::kText);
      for (int p = 0; p < 4; ++p) {
        auto seg = std::make_unique<MemorySegment>(stream_of(parts[(size_t)p], p % 2 == 0));
        seg->index = p;
        q.insert(std::move(seg));
      }
      KVWriter w(&q, KeyKind::kText, op);
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
      EXPECT(buffers > 10);
      EXPECT(w.records_in() == (int64_t)in.size());
      if (op == CombineOp::kSumInt) {
        EXPECT(all == stream_of(want, true));
        EXPECT(w.records() == (int64_t)want.size());
      } else {
        EXPECT(records_of(all).size() == in.size() && w.records() == (int64_t)in.size());
      }
    }
  }
  std::printf("combine selftest: %d failures\n", failures);
  return failures ? 1 : 0;
}
