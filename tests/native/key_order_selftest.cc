// Stand-alone self-test of mapred.uda.key.order=hadoop on the host (csrc/include/uda/compare.h), built with
// ASan + UBSan by tests/test_key_order_cpu.py: key_sortable, key_compare and key_normalize over the edge values
// of every numeric kind, every key read from its own exact-size heap copy (a key must never be read past its
// length, a key of the wrong length not at all past it), and the CPU merge (MergeQueue) over signed keys and
// over a key of the wrong length.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "uda/compare.h"
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

static std::string be(uint64_t v, int w) {
  std::string s((size_t)w, '\0');
  for (int i = w - 1; i >= 0; --i) {
    s[(size_t)i] = (char)(uint8_t)v;
    v >>= 8;
  }
  return s;
}
static std::string vl(int64_t v) {
  uint8_t b[9];
  const int n = vint_encode(v, b);
  return std::string(reinterpret_cast<char*>(b), (size_t)n);
}

// key_sortable of an exact-size heap copy
static uint64_t word(KeyKind kind, const std::string& k, bool* ok) {
  std::unique_ptr<uint8_t[]> p(new uint8_t[k.size()]);
  std::memcpy(p.get(), k.data(), k.size());
  return key_sortable(kind, p.get(), (int)k.size(), ok);
}
static int cmp(KeyKind kind, const std::string& a, const std::string& b) {
  std::unique_ptr<uint8_t[]> pa(new uint8_t[a.size()]), pb(new uint8_t[b.size()]);
  std::memcpy(pa.get(), a.data(), a.size());
  std::memcpy(pb.get(), b.data(), b.size());
  return key_compare(kind, pa.get(), (int)a.size(), pb.get(), (int)b.size());
}

// keys in strictly ascending order of the class's Hadoop comparator
static void ascending(KeyKind kind, const std::vector<std::string>& keys) {
  for (size_t i = 0; i < keys.size(); ++i) {
    bool ok = false;
    const uint64_t wi = word(kind, keys[i], &ok);
    EXPECT(ok);
    std::unique_ptr<uint8_t[]> p(new uint8_t[keys[i].size()]);
    std::memcpy(p.get(), keys[i].data(), keys[i].size());
    const KeyNorm n = key_normalize(kind, p.get(), (int)keys[i].size());
    EXPECT(n.k0 == wi && n.k1 == 0 && n.len == 8 && n.off == 0);
    for (size_t j = 0; j < keys.size(); ++j) {
      const int c = cmp(kind, keys[i], keys[j]);
      EXPECT((c < 0) == (i < j) && (c > 0) == (i > j));
    }
  }
}

static void equal(KeyKind kind, const std::string& a, const std::string& b) {
  bool oa = false, ob = false;
  EXPECT(word(kind, a, &oa) == word(kind, b, &ob) && oa && ob);
  EXPECT(cmp(kind, a, b) == 0 && cmp(kind, b, a) == 0);
}

static void refused(KeyKind kind, const std::string& k) {
  bool ok = true;
  EXPECT(word(kind, k, &ok) == 0 && !ok);
}

static std::vector<uint8_t> stream_of(const std::vector<std::pair<std::string, std::string>>& recs) {
  std::vector<uint8_t> out;
  for (const auto& r : recs)
    ifile_append(&out, reinterpret_cast<const uint8_t*>(r.first.data()), (int32_t)r.first.size(),
                 reinterpret_cast<const uint8_t*>(r.second.data()), (int32_t)r.second.size());
  ifile_append_eof(&out);
  return out;
}

int main() {
  const int64_t i64min = std::numeric_limits<int64_t>::min(), i64max = std::numeric_limits<int64_t>::max();
  {  // fixed-width integers: min, -1, 0, 1, max and both sides of every byte boundary
    ascending(KeyKind::kByte, {be(0x80, 1), be(0x81, 1), be(0xff, 1), be(0, 1), be(1, 1), be(0x7f, 1)});
    ascending(KeyKind::kShort, {be(0x8000, 2), be(0xff00, 2), be(0xffff, 2), be(0, 2), be(0xff, 2), be(0x100, 2), be(0x7fff, 2)});
    ascending(KeyKind::kInt, {be(0x80000000u, 4), be(0xff000000u, 4), be(0xffff0000u, 4), be(0xfffffeffu, 4), be(0xffffff00u, 4),
                              be(0xffffffffu, 4), be(0, 4), be(1, 4), be(0xff, 4), be(0x100, 4), be(0xffff, 4), be(0x10000, 4),
                              be(0xffffff, 4), be(0x1000000, 4), be(0x7fffffff, 4)});
    std::vector<std::string> longs = {be((uint64_t)i64min, 8)};
    for (int b = 56; b >= 8; b -= 8) longs.push_back(be((uint64_t)(-(1ll << b)), 8));
    longs.push_back(be((uint64_t)-1ll, 8));
    longs.push_back(be(0, 8));
    for (int b = 8; b <= 56; b += 8) {
      longs.push_back(be((1ull << b) - 1, 8));
      longs.push_back(be(1ull << b, 8));
    }
    longs.push_back(be((uint64_t)i64max, 8));
    ascending(KeyKind::kLong, longs);
  }
  {  // VLong at every encoded length, both signs; VInt within int
    std::vector<int64_t> vals = {i64min};
    for (int b = 56; b >= 8; b -= 8) {
      vals.push_back(-(1ll << b) - 1);
      vals.push_back(-(1ll << b));
    }
    for (int64_t v : {-129ll, -128ll, -113ll, -112ll, -1ll, 0ll, 1ll, 127ll, 128ll, 255ll}) vals.push_back(v);
    for (int b = 8; b <= 56; b += 8) {
      vals.push_back(1ll << b);
      vals.push_back((1ll << b) + 1);
    }
    vals.push_back(i64max);
    std::vector<std::string> vlongs, vints;
    bool sizes[10] = {false};
    for (int64_t v : vals) {
      vlongs.push_back(vl(v));
      sizes[vlongs.back().size()] = true;
      if (v >= INT32_MIN && v <= INT32_MAX) vints.push_back(vl(v));
    }
    for (int n = 1; n <= 9; ++n) EXPECT(sizes[n]);
    ascending(KeyKind::kVLong, vlongs);
    ascending(KeyKind::kVInt, vints);
    // a non-canonical encoding is the value it holds
    equal(KeyKind::kVLong, vl(300), std::string("\x8c", 1) + be(300, 4));
    equal(KeyKind::kVInt, vl(-1), std::string("\x86", 1) + be(0, 2));
    equal(KeyKind::kVLong, vl(5), std::string("\x8f", 1) + be(5, 1));
    refused(KeyKind::kVInt, vl((int64_t)INT32_MAX + 1));
    refused(KeyKind::kVInt, vl((int64_t)INT32_MIN - 1));
    refused(KeyKind::kVInt, "");
    refused(KeyKind::kVLong, std::string("\x8e\x01", 2));          // announces 3 bytes, has 2
    refused(KeyKind::kVLong, std::string("\x05\x00", 2));          // announces 1 byte, has 2
    refused(KeyKind::kVLong, std::string("\x88", 1) + be(1, 9));   // longer than any VLong
  }
  {  // floats: Java's Float.compare / Double.compare
    ascending(KeyKind::kFloat, {be(0xff800000u, 4), be(0xff7fffffu, 4), be(0xbf800001u, 4), be(0xbf800000u, 4), be(0xbf7fffffu, 4),
                                be(0x80800000u, 4), be(0x807fffffu, 4), be(0x80000001u, 4), be(0x80000000u, 4), be(0, 4), be(1, 4),
                                be(0x007fffffu, 4), be(0x00800000u, 4), be(0x3f7fffffu, 4), be(0x3f800000u, 4), be(0x3f800001u, 4),
                                be(0x7f7fffffu, 4), be(0x7f800000u, 4), be(0x7fc00000u, 4)});
    equal(KeyKind::kFloat, be(0x7fc00000u, 4), be(0xffc00001u, 4));
    equal(KeyKind::kFloat, be(0x7f800001u, 4), be(0xffffffffu, 4));
    ascending(KeyKind::kDouble,
              {be(0xfff0000000000000ull, 8), be(0xffefffffffffffffull, 8), be(0xbff0000000000001ull, 8), be(0xbff0000000000000ull, 8),
               be(0xbfefffffffffffffull, 8), be(0x8010000000000000ull, 8), be(0x800fffffffffffffull, 8), be(0x8000000000000001ull, 8),
               be(0x8000000000000000ull, 8), be(0, 8), be(1, 8), be(0x000fffffffffffffull, 8), be(0x0010000000000000ull, 8),
               be(0x3fefffffffffffffull, 8), be(0x3ff0000000000000ull, 8), be(0x3ff0000000000001ull, 8), be(0x7fefffffffffffffull, 8),
               be(0x7ff0000000000000ull, 8), be(0x7ff8000000000000ull, 8)});
    equal(KeyKind::kDouble, be(0x7ff8000000000000ull, 8), be(0xfff8000000000001ull, 8));
    equal(KeyKind::kDouble, be(0x7ff0000000000001ull, 8), be(0xffffffffffffffffull, 8));
  }
  // fixed widths refuse every other length, the empty key included
  for (KeyKind kind : {KeyKind::kByte, KeyKind::kShort, KeyKind::kInt, KeyKind::kLong, KeyKind::kFloat, KeyKind::kDouble})
    for (int n = 0; n <= 10; ++n)
      if (n != key_fixed_bytes(kind)) refused(kind, std::string((size_t)n, '\x01'));
  // the byte kinds are untouched: memcmp, the reference's order
  EXPECT(cmp(KeyKind::kRaw, be(0xffffffffu, 4), be(3, 4)) > 0);
  EXPECT(!key_kind_numeric(KeyKind::kText) && !key_kind_numeric(KeyKind::kRaw) && !key_kind_numeric(KeyKind::kBytes) &&
         !key_kind_numeric(KeyKind::kUnsupported) && key_kind_numeric(KeyKind::kByte) && key_kind_numeric(KeyKind::kDouble));
  {  // the CPU merge: runs [-1, 3] and [3] come out -1, 3, 3; a 3-byte IntWritable key throws and names its map output
    const std::vector<uint8_t> a = stream_of({{be(0xffffffffu, 4), "a"}, {be(3, 4), "b"}}), b = stream_of({{be(3, 4), "c"}});
    MergeQueue q(KeyKind::kInt);
    auto sa = std::make_unique<MemorySegment>(a.data(), a.size());
    auto sb = std::make_unique<MemorySegment>(b.data(), b.size());
    sb->index = 1;
    q.insert(std::move(sa));
    q.insert(std::move(sb));
    std::string vals;
    while (q.next()) vals.append(reinterpret_cast<const char*>(q.cur().val), (size_t)q.cur().vlen);
    EXPECT(vals == "abc");
    const std::vector<uint8_t> bad = stream_of({{be(1, 4), "x"}, {be(7, 3), "y"}, {be(9, 4), "z"}});
    MergeQueue q2(KeyKind::kInt);
    auto sc = std::make_unique<MemorySegment>(bad.data(), bad.size());
    sc->name = "attempt_m_7";
    q2.insert(std::move(sc));
    bool threw = false;
    try {
      while (q2.next()) {
      }
    } catch (const UdaError& e) {
      threw = std::string(e.what()).find("IntWritable key of 3 bytes (4 expected) in map output attempt_m_7") != std::string::npos;
    }
    EXPECT(threw);
  }
  std::printf("key_order_selftest: %d failures\n", failures);
  return failures ? 1 : 0;
}
