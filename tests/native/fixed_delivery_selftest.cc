// Stand-alone check of the FIXED10 piece delivery in csrc/gpu/fixed_delivery.cc, meant to be built with
// -fsanitize=address,undefined together with csrc/codec/colpack.cc: pieces, staging buffers and the tail
// buffer are exact-size heap allocations, so a read past a piece or a write past kv_buf + 16 is
// reported. Every delivery is compared with plain slicing of the records plus the EOF rule.
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

// piece: exactly `len` heap bytes; staging and tail exactly as large as the header says they must be
static Run deliver(const uint8_t* piece, int64_t len, int64_t record_bytes, int64_t buf_bytes, int64_t kv_buf, bool packed,
                   bool last) {
  Run r;
  auto p = exact(piece, (size_t)len);
  const size_t one = (size_t)std::max(kv_buf, buf_bytes) + 16;
  std::unique_ptr<uint8_t[]> s0(new uint8_t[one]), s1(new uint8_t[one]), tail(new uint8_t[(size_t)kv_buf + 16]);
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
  try {
    deliver_fixed_piece(fp, buf_bytes, kv_buf, b, [&](const uint8_t* d, int64_t n) {
      r.bufs.emplace_back((const char*)d, (size_t)n);
      return 0;
    }, &r.c);
  } catch (const std::runtime_error& e) {
    r.threw = true;
    r.what = e.what();
  }
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
}

static void rejected(const std::vector<uint8_t>& piece, int64_t record_bytes, bool packed, const char* reason) {
  Run r = deliver(piece.data(), (int64_t)piece.size(), record_bytes, 78 * L, 8192, packed, true);
  CHECK(r.threw && r.bufs.empty());
  CHECK(r.what.find(reason) != std::string::npos);
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
  // sweep: every piece size against three buffer sizes, as the task's last piece and not
  for (int64_t buf_records : {1, 13, 78})
    for (int64_t n = 1; n <= 400; ++n) {
      both_ways(first(n), buf_records, buf_records * L + 2, n % 2 == 0);  // EOF fits
      if (n % 7 == 0) both_ways(first(n), buf_records, buf_records * L, true);  // EOF never fits a full buffer
    }
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
