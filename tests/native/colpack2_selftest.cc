// Stand-alone check of colpack version 2 in csrc/codec/colpack.cc, meant to be built with
// -fsanitize=address,undefined: the encoder, both decoders and the header checks run on exact-size heap
// buffers, and every destination has guard bytes on both sides, so a read past a piece or a write
// outside rows * L is reported. Prints "<n> checks, <m> failures".
#include "codec/colpack.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

using namespace uda;

static int g_checks = 0, g_failures = 0;
#define CHECK(c)                                               \
  do {                                                         \
    ++g_checks;                                                \
    if (!(c)) {                                                \
      ++g_failures;                                            \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                          \
  } while (0)

// n records of L bytes with columns in [lo, lo + span]; the key field holds ascending (sorted) or
// random big-endian keys whose steps stay below 2^step_bits.
static std::vector<uint8_t> make(int64_t n, int L, int lo, int span, int ko, int kl, int step_bits, bool sorted,
                                 std::mt19937_64& rng) {
  std::vector<uint8_t> v((size_t)(n * L));
  unsigned __int128 key = 0;
  for (int64_t r = 0; r < n; ++r) {
    uint8_t* rec = v.data() + r * L;
    for (int c = 0; c < L; ++c) rec[c] = (uint8_t)(lo + (int)(rng() % (uint64_t)(span + 1)));
    unsigned __int128 step = rng();
    if (step_bits > 64) step = (step << (step_bits - 64)) | (rng() >> (128 - step_bits));
    else if (step_bits < 64) step &= (((unsigned __int128)1) << step_bits) - 1;
    key = sorted ? key + step : (((unsigned __int128)rng()) << 64) | rng();
    for (int k = 0; k < kl; ++k) rec[ko + kl - 1 - k] = (uint8_t)(key >> (8 * k));
  }
  return v;
}

static std::unique_ptr<uint8_t[]> exact(const uint8_t* p, size_t n) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(b.get(), p, n);
  return b;
}

constexpr size_t kGuard = 32;

// Unpack a range into the middle of a guarded buffer: the records come back and the guards stay.
template <typename F>
static void unpack_guarded(F&& f, const std::vector<uint8_t>& recs, int L, int64_t row0, int64_t rows) {
  const size_t bytes = (size_t)(rows * L);
  std::unique_ptr<uint8_t[]> buf(new uint8_t[bytes + 2 * kGuard]);
  std::memset(buf.get(), 0xA5, bytes + 2 * kGuard);
  f(buf.get() + kGuard);
  CHECK(std::memcmp(buf.get() + kGuard, recs.data() + row0 * L, bytes) == 0);
  bool intact = true;
  for (size_t k = 0; k < kGuard; ++k) intact = intact && buf[k] == 0xA5 && buf[kGuard + bytes + k] == 0xA5;
  CHECK(intact);
}

enum Expect { kPlain, kDelta, kRaw, kAny };

static void roundtrip(const std::vector<uint8_t>& recs, int L, int64_t buf, int ko, int kl, Expect expect) {
  const int64_t n = (int64_t)recs.size() / L;
  auto src = exact(recs.data(), recs.size());
  const int64_t bound = colpack2_bound(L, n, buf);
  std::unique_ptr<uint8_t[]> dst(new uint8_t[(size_t)bound]);
  const int64_t len = colpack2_encode(src.get(), n, L, buf, ko, kl, dst.get());
  CHECK(len >= (int64_t)kColpackHeaderBytes && len <= bound && len % 64 == 0);
  auto piece = exact(dst.get(), (size_t)len);
  ColpackPiece p;
  const char* why = nullptr;
  CHECK(colpack_open(piece.get(), len, L, n, &p, &why));
  CHECK(p.version == 2);
  if (expect == kRaw) CHECK(!p.packed);
  if (expect == kDelta) CHECK(p.packed && p.delta);
  if (expect == kPlain) CHECK(p.packed && !p.delta);
  if (!p.packed) {
    CHECK(len == (int64_t)kColpackHeaderBytes);
    return;
  }
  CHECK(len == colpack2_packed_bytes(p.stride, n, p.delta ? colpack2_table_bytes(n, buf) : 0));
  CHECK(p.rows + p.stride * n + 8 <= piece.get() + len);
  const int64_t b = std::max<int64_t>(buf, 1);
  const int64_t ranges[][2] = {{0, n}, {0, 1}, {n - 1, 1}, {n / 2, n - n / 2}, {n, 0},
                               {std::min(n - 1, b), 1}, {std::min(n - 1, b + 1), std::min<int64_t>(n - std::min(n - 1, b + 1), b)},
                               {std::min(n - 1, 2 * b - 1), n - std::min(n - 1, 2 * b - 1)}};
  for (const auto& rg : ranges) {
    unpack_guarded([&](uint8_t* d) { colpack_unpack_scalar(p, rg[0], rg[1], d); }, recs, L, rg[0], rg[1]);
    if (colpack_have_bmi2())
      unpack_guarded([&](uint8_t* d) { CHECK(colpack_unpack_bmi2(p, rg[0], rg[1], d)); }, recs, L, rg[0], rg[1]);
    unpack_guarded([&](uint8_t* d) { colpack_unpack(p, rg[0], rg[1], d); }, recs, L, rg[0], rg[1]);
  }
}

static void rejections(const std::vector<uint8_t>& recs, int L, int64_t buf, int ko, int kl) {
  const int64_t n = (int64_t)recs.size() / L;
  std::vector<uint8_t> good((size_t)colpack2_bound(L, n, buf));
  const int64_t len = colpack2_encode(recs.data(), n, L, buf, ko, kl, good.data());
  good.resize((size_t)len);
  ColpackPiece p;
  CHECK(colpack_open(good.data(), len, L, n, &p) && p.packed && p.delta);
  auto rejected = [&](const std::vector<uint8_t>& v, int64_t vlen) {
    auto piece = exact(v.data(), (size_t)vlen);
    ColpackPiece q;
    const char* why = nullptr;
    const bool ok = colpack_open(piece.get(), vlen, L, n, &q, &why);
    CHECK(!ok);
    CHECK(ok || (why && *why));
  };
  ColpackHeader h;
  std::memcpy(&h, good.data(), sizeof(h));
  auto with = [&](const ColpackHeader& hh) {
    std::vector<uint8_t> v = good;
    std::memcpy(v.data(), &hh, sizeof(hh));
    return v;
  };
  ColpackHeader x = h;
  x.version = 3;
  rejected(with(x), len);
  x = h;
  x.version = 1;  // a version 2 header read as version 1: its offsets are no group sizes
  rejected(with(x), len);
  x = h;
  x.key_off = (uint32_t)(L - kl + 1);
  rejected(with(x), len);
  x = h;
  x.key_len = 17;
  rejected(with(x), len);
  x = h;
  x.key_len = 0;
  rejected(with(x), len);
  x = h;
  x.buf_records = 0;
  rejected(with(x), len);
  x = h;
  x.buf_records = 1;  // a table of n entries: table and rows no longer fit
  rejected(with(x), len);
  x = h;
  x.bo[1] += 1;
  rejected(with(x), len);
  x = h;
  x.bo[kColpackMaxGroups - 1] = 8;
  rejected(with(x), len);
  x = h;
  x.stride += 1;
  rejected(with(x), len);
  x = h;
  x.flags |= 4;
  rejected(with(x), len);
  x = h;
  x.mask[1] ^= 0x02;
  rejected(with(x), len);
  for (int64_t k = 0; k < len; k += (k < (int64_t)kColpackHeaderBytes + 8 ? 1 : 61)) rejected(good, k);
  rejected(good, len - 1);
}

int main() {
  std::mt19937_64 rng(4242);
  // TeraSort shape: sorted, shuffled (differences wrap: plain or raw), duplicate keys
  const int64_t counts[] = {1, 77, 78, 79, 2520, 2479};
  for (int64_t n : counts) roundtrip(make(n, 104, 'A', 25, 3, 10, 56, true, rng), 104, 78, 3, 10, n > 78 ? kDelta : kAny);
  roundtrip(make(2520, 104, 'A', 25, 3, 10, 56, false, rng), 104, 78, 3, 10, kAny);
  roundtrip(make(2520, 104, 'A', 25, 3, 10, 0, true, rng), 104, 78, 3, 10, kPlain);  // every key equal: no bits either way
  // buf_records 1: the table turns delta off; buf_records 0 and key_len 0: no key
  roundtrip(make(400, 104, 'A', 25, 3, 10, 56, true, rng), 104, 1, 3, 10, kPlain);
  roundtrip(make(400, 104, 'A', 25, 3, 10, 56, true, rng), 104, 0, 3, 10, kPlain);
  roundtrip(make(400, 104, 'A', 25, 0, 0, 56, true, rng), 104, 78, 0, 0, kPlain);
  // a key across group boundaries, at the record's end, 16 bytes at offset 0, L no multiple of 8
  roundtrip(make(600, 40, 0, 1, 5, 12, 40, true, rng), 40, 50, 5, 12, kDelta);
  roundtrip(make(600, 27, 0, 1, 19, 8, 24, true, rng), 27, 50, 19, 8, kDelta);
  roundtrip(make(500, 24, 0, 1, 0, 16, 100, true, rng), 24, 64, 0, 16, kDelta);
  roundtrip(make(333, 21, 0, 7, 2, 6, 20, true, rng), 21, 40, 2, 6, kDelta);
  // widths that fill a group's 64 bits after a misaligned neighbour; incompressible records
  roundtrip(make(300, 80, 0, 3, 8, 8, 64, false, rng), 80, 64, 8, 8, kAny);
  roundtrip(make(300, 24, 0, 127, 0, 0, 0, true, rng), 24, 64, 0, 0, kPlain);
  roundtrip(make(3000, 104, 0, 255, 3, 10, 56, false, rng), 104, 78, 3, 10, kRaw);
  const int lens[] = {1, 5, 7, 9, 13, 100, 255, 256};
  for (int L : lens) roundtrip(make(333, L, 48, 9, 0, std::min(L, 4), 12, true, rng), L, 30, 0, std::min(L, 4), kAny);
  rejections(make(2520, 104, 'A', 25, 3, 10, 56, true, rng), 104, 78, 3, 10);
  rejections(make(600, 27, 0, 1, 19, 8, 24, true, rng), 27, 50, 19, 8);
  // out-of-range arguments
  {
    uint8_t b[8] = {0};
    std::vector<uint8_t> d((size_t)colpack2_bound(8, 1, 1));
    CHECK(colpack2_encode(b, 0, 8, 1, 0, 4, d.data()) == 0);
    CHECK(colpack2_encode(b, 1, 0, 1, 0, 0, d.data()) == 0);
    CHECK(colpack2_encode(b, 1, 8, 1, 4, 5, d.data()) == 0);
    CHECK(colpack2_encode(b, 1, 8, 1, 0, 17, d.data()) == 0);
    CHECK(colpack2_encode(b, 1, 8, 1, -1, 2, d.data()) == 0);
  }
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
