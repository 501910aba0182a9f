// Stand-alone check of the FIXED10 piece delivery in csrc/gpu/fixed_delivery.cc, meant to be built with
// -fsanitize=address,undefined together with csrc/codec/colpack.cc: pieces, staging buffers and the tail
// buffer are exact-size heap allocations, so a read past a piece or a write past kv_buf + 16 is
// reported. Every delivery is compared with plain slicing of the records plus the EOF rule, and repeated
// with an empty sink over staging and tail buffers of one byte: it counts the same buffers and writes nothing.
// Prints "<n> checks, <m> failures".
#include "fixed_delivery.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "codec/colpack.h"

using namespace uda;
using namespace uda::gpu;

static int g_checks = 0, g_failures = 0;
#define CHECK(c)                                               \
  do {                                                         \
    ++g_checks;                                                \
    if (!(c)) {                                                \
      ++g_failures;                                            \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                          \
  } while (0)

constexpr int L = 104;

// n sorted TeraSort IFile records; values 'A'..'Z' (packed pieces) or any byte (raw pieces)
static std::vector<uint8_t> records(int64_t n, bool wide_values, std::mt19937_64& rng) {
  std::vector<uint8_t> v((size_t)(n * L));
  uint64_t key = 0;
  for (int64_t r = 0; r < n; ++r) {
    uint8_t* rec = v.data() + r * L;
    rec[0] = 0x0B, rec[1] = 0x5B, rec[2] = 0x0A;
    key += rng() >> 24;
    for (int k = 0; k < 8; ++k) rec[3 + k] = (uint8_t)(key >> (56 - 8 * k));
    rec[11] = (uint8_t)rng(), rec[12] = (uint8_t)rng();
    rec[13] = 0x5A;
    for (int c = 14; c < L; ++c) rec[c] = wide_values ? (uint8_t)rng() : (uint8_t)('A' + rng() % 26);
  }
  return v;
}

static std::unique_ptr<uint8_t[]> exact(const uint8_t* p, size_t n) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(b.get(), p, n);
  return b;
}

static std::vector<std::string> expected(const std::vector<uint8_t>& raw, int64_t buf_bytes, int64_t kv_buf, bool last) {
  std::vector<std::string> out;
  for (size_t o = 0; o < raw.size(); o += (size_t)buf_bytes)
    out.emplace_back((const char*)raw.data() + o, std::min((size_t)buf_bytes, raw.size() - o));
  if (last) {
    if (!out.empty() && (int64_t)out.back().size() + 2 <= kv_buf)
      out.back() += "\xff\xff";
    else
      out.emplace_back("\xff\xff");
  }
  return out;
}

struct Run {
  std::vector<std::string> bufs;
  FixedDeliveryCounters c;
  bool threw = false;
  std::string what;
};

// piece: exactly `len` heap bytes; staging and tail exactly as large as the header says they must be.
// drop: an empty sink, and staging and tail of one byte each (nothing may be written to them)
static Run deliver(const uint8_t* piece, int64_t len, int64_t record_bytes, int64_t buf_bytes, int64_t kv_buf, bool packed,
                   bool last, bool drop = false) {
  Run r;
  auto p = exact(piece, (size_t)len);
  const size_t one = drop ? 1 : (size_t)std::max(kv_buf, buf_bytes) + 16;
  std::unique_ptr<uint8_t[]> s0(new uint8_t[one]), s1(new uint8_t[one]), tail(new uint8_t[drop ? 1 : (size_t)kv_buf + 16]);
  s0[0] = s1[0] = tail[0] = 0x5C;
  FixedBuffers b;
  b.staging[0] = s0.get();
  b.staging[1] = s1.get();
  b.tail = tail.get();
  FixedPiece fp;
  fp.base = p.get();
  fp.copied = len;
  fp.record_bytes = record_bytes;
  fp.packed = packed;
  fp.last = last;
  FixedSink sink;
  if (!drop)
    sink = [&](const uint8_t* d, int64_t n) {
      r.bufs.emplace_back((const char*)d, (size_t)n);
      return 0;
    };
  try {
    deliver_fixed_piece(fp, buf_bytes, kv_buf, b, sink, &r.c);
  } catch (const std::runtime_error& e) {
    r.threw = true;
    r.what = e.what();
  }
  if (drop) CHECK(s0[0] == 0x5C && s1[0] == 0x5C && tail[0] == 0x5C && r.c.unpack_ms == 0);
  return r;
}

static std::vector<uint8_t> encode(const std::vector<uint8_t>& raw, int64_t buf_records, bool* packed) {
  const int64_t n = (int64_t)raw.size() / L;
  auto src = exact(raw.data(), raw.size());
  std::vector<uint8_t> dst((size_t)colpack2_bound(L, n, buf_records));
  const int64_t len = colpack2_encode(src.get(), n, L, buf_records, 3, 10, dst.data());
  dst.resize((size_t)len);
  *packed = len > (int64_t)kColpackHeaderBytes;
  return dst;
}

// both forms of a piece against the slicing
static void both_ways(const std::vector<uint8_t>& raw, int64_t buf_records, int64_t kv_buf, bool last) {
  const int64_t buf_bytes = buf_records * L;
  const auto want = expected(raw, buf_bytes, kv_buf, last);
  bool packed = false;
  const auto piece = encode(raw, buf_records, &packed);
  CHECK(packed);
  Run a = deliver(piece.data(), (int64_t)piece.size(), (int64_t)raw.size(), buf_bytes, kv_buf, true, last);
  CHECK(!a.threw && a.bufs == want);
  CHECK(a.c.buffers == (int64_t)want.size() && a.c.eof_sent == last);
  Run b = deliver(raw.data(), (int64_t)raw.size(), (int64_t)raw.size(), buf_bytes, kv_buf, false, last);
  CHECK(!b.threw && b.bufs == want);
  CHECK(b.c.buffers == (int64_t)want.size() && b.c.eof_sent == last);
  // no sink: the same count, nothing built
  Run c = deliver(piece.data(), (int64_t)piece.size(), (int64_t)raw.size(), buf_bytes, kv_buf, true, last, true);
  CHECK(!c.threw && c.c.buffers == a.c.buffers && c.c.eof_sent == a.c.eof_sent);
  Run d = deliver(raw.data(), (int64_t)raw.size(), (int64_t)raw.size(), buf_bytes, kv_buf, false, last, true);
  CHECK(!d.threw && d.c.buffers == b.c.buffers && d.c.eof_sent == b.c.eof_sent);
}

static void rejected(const std::vector<uint8_t>& piece, int64_t record_bytes, bool packed, const char* reason) {
  Run r = deliver(piece.data(), (int64_t)piece.size(), record_bytes, 78 * L, 8192, packed, true);
  CHECK(r.threw && r.bufs.empty());
  CHECK(r.what.find(reason) != std::string::npos);
  Run e = deliver(piece.data(), (int64_t)piece.size(), record_bytes, 78 * L, 8192, packed, true, true);  // no sink
  CHECK(e.threw && e.c.buffers == 0 && e.what == r.what);
}

static bool copy_len_throws(const FixedLayout& l, int64_t bytes, int64_t nrec) {
  try {
    CHECK(l.packed_copy_len(bytes, nrec) == bytes);
    return false;
  } catch (const std::runtime_error&) {
    return true;
  }
}

int main() {
  std::mt19937_64 rng(20240611);
  const auto recs = records(400, false, rng);
  auto first = [&](int64_t n) { return std::vector<uint8_t>(recs.begin(), recs.begin() + n * L); };

  // the named cases
  both_ways(first(312), 78, 8192, false);     // four full buffers
  both_ways(first(1), 78, 8192, false);       // a piece longer packed than plain
  both_ways(first(300), 78, 8192, false);     // a short last buffer
  both_ways(first(300), 78, 8192, true);      // EOF in the final buffer
  both_ways(first(312), 78, 8192, true);      // final buffer full, EOF still fits kv_buf
  both_ways(first(312), 78, 78 * L, true);    // final buffer exactly kv_buf: EOF in a buffer of its own
  both_ways(first(1), 78, 8192, true);
  both_ways(first(5), 1, L, true);
  {
    Run r = deliver(nullptr, 0, 0, 78 * L, 8192, false, true);  // the marker alone
    CHECK(!r.threw && r.bufs.size() == 1 && r.bufs[0] == "\xff\xff");
    Run e = deliver(nullptr, 0, 0, 78 * L, 8192, false, true, true);
    CHECK(!e.threw && e.c.buffers == 1 && e.c.eof_sent);
  }
  {
    // values of any byte: the encoder says raw, the records travel as they are
    const auto wide = records(200, true, rng);
    bool packed = true;
    const auto hdr = encode(wide, 78, &packed);
    CHECK(!packed && hdr.size() == kColpackHeaderBytes);
    Run r = deliver(wide.data(), (int64_t)wide.size(), (int64_t)wide.size(), 78 * L, 8192, false, true);
    CHECK(!r.threw && r.bufs == expected(wide, 78 * L, 8192, true));
    rejected(hdr, (int64_t)wide.size(), true, "not marked packed");
  }
  // rejections: nothing reaches the sink
  {
    const auto raw = first(312);
    bool packed = false;
    const auto piece = encode(raw, 78, &packed);
    auto bad = piece;
    bad[1] ^= 1;
    rejected(bad, (int64_t)raw.size(), true, "bad magic");
    rejected(piece, 311 * L, true, "record count");
    bad = piece;
    bad[16] ^= 3;  // header record count
    rejected(bad, (int64_t)raw.size(), true, "record count");
    rejected(std::vector<uint8_t>(piece.begin(), piece.end() - 64), (int64_t)raw.size(), true, "exceed the piece's length");
    rejected(std::vector<uint8_t>(piece.begin(), piece.begin() + 100), (int64_t)raw.size(), true, "shorter than its header");
    rejected(std::vector<uint8_t>(raw.begin(), raw.end() - L), (int64_t)raw.size(), false, "another length");
  }
  // a packed length from the device: a header at least, the piece's bound and a ring slot at most
  {
    const FixedLayout l = fixed_layout(8192, 32 << 10, 4, 2);
    const int64_t bound = l.piece_bound(312);
    CHECK(l.piece_recs == 312 && bound <= l.slot_bytes);
    CHECK(!copy_len_throws(l, (int64_t)kColpackHeaderBytes, 312) && !copy_len_throws(l, bound, 312));
    CHECK(copy_len_throws(l, (int64_t)kColpackHeaderBytes - 1, 312) && copy_len_throws(l, bound + 1, 312));
    CHECK(copy_len_throws(l, l.piece_bound(1) + 1, 1));  // the bound of this piece, not of a full one
    const FixedLayout tiny = fixed_layout(104, 104, 2, 2);
    CHECK(tiny.slot_bytes == 832 && !copy_len_throws(tiny, 832, 1) && copy_len_throws(tiny, 833, 1));
    CHECK(copy_len_throws(tiny, 896, 400));  // within the bound of 400 records, past the slot
  }
  // sweep: every piece size against three buffer sizes, as the task's last piece and not
  for (int64_t buf_records : {1, 13, 78})
    for (int64_t n = 1; n <= 400; ++n) {
      both_ways(first(n), buf_records, buf_records * L + 2, n % 2 == 0);  // EOF fits
      if (n % 7 == 0) both_ways(first(n), buf_records, buf_records * L, true);  // EOF never fits a full buffer
    }
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
