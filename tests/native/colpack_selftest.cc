// Stand-alone check of csrc/codec/colpack.cc, meant to be built with -fsanitize=address,undefined:
// encode, both decoders and the header checks run on exact-size heap buffers, so a read or write
// past a piece, a row range or a destination is reported by the sanitizer. Prints "<n> checks, <m> failures".
#include "codec/colpack.h"

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

// n records of L bytes; column c takes values in [lo[c], lo[c] + span[c]].
static std::vector<uint8_t> make(int64_t n, int L, const std::vector<int>& lo, const std::vector<int>& span,
                                 std::mt19937_64& rng) {
  std::vector<uint8_t> v((size_t)(n * L));
  for (int64_t r = 0; r < n; ++r)
    for (int c = 0; c < L; ++c) v[(size_t)(r * L + c)] = (uint8_t)(lo[c] + (int)(rng() % (uint64_t)(span[c] + 1)));
  return v;
}

// Exact-size heap copy, so the sanitizer sees the first byte past it.
static std::unique_ptr<uint8_t[]> exact(const uint8_t* p, size_t n) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(b.get(), p, n);
  return b;
}

static void roundtrip(const std::vector<uint8_t>& recs, int L, bool expect_packed) {
  const int64_t n = (int64_t)recs.size() / L;
  auto src = exact(recs.data(), recs.size());
  std::unique_ptr<uint8_t[]> dst(new uint8_t[(size_t)colpack_bound(L, n)]);
  const int64_t len = colpack_encode(src.get(), n, L, 100, dst.get());
  CHECK(len >= (int64_t)kColpackHeaderBytes && len <= colpack_bound(L, n) && len % 64 == 0);
  auto piece = exact(dst.get(), (size_t)len);
  ColpackPiece p;
  const char* why = nullptr;
  CHECK(colpack_open(piece.get(), len, L, n, &p, &why));
  CHECK(p.packed == expect_packed);
  if (!p.packed) {
    CHECK(len == (int64_t)kColpackHeaderBytes);
    return;
  }
  CHECK(len == colpack_packed_bytes(p.stride, n));
  const int64_t ranges[][2] = {{0, n}, {0, 1}, {n - 1, 1}, {n / 2, n - n / 2}, {n, 0}};
  for (const auto& rg : ranges) {
    const size_t bytes = (size_t)(rg[1] * L);
    std::unique_ptr<uint8_t[]> a(new uint8_t[bytes ? bytes : 1]), b(new uint8_t[bytes ? bytes : 1]);
    colpack_unpack_scalar(p, rg[0], rg[1], a.get());
    CHECK(std::memcmp(a.get(), recs.data() + rg[0] * L, bytes) == 0);
    if (colpack_unpack_bmi2(p, rg[0], rg[1], b.get())) CHECK(std::memcmp(a.get(), b.get(), bytes) == 0);
    colpack_unpack(p, rg[0], rg[1], b.get());
    CHECK(std::memcmp(b.get(), recs.data() + rg[0] * L, bytes) == 0);
  }
}

static void rejections(const std::vector<uint8_t>& recs, int L) {
  const int64_t n = (int64_t)recs.size() / L;
  std::vector<uint8_t> good((size_t)colpack_bound(L, n));
  const int64_t len = colpack_encode(recs.data(), n, L, 100, good.data());
  good.resize((size_t)len);
  ColpackPiece p;
  CHECK(colpack_open(good.data(), len, L, n, &p));
  auto rejected = [&](const std::vector<uint8_t>& v, int64_t vlen, int eL, int64_t en) {
    auto piece = exact(v.data(), (size_t)vlen);
    ColpackPiece q;
    const char* why = nullptr;
    const bool ok = colpack_open(piece.get(), vlen, eL, en, &q, &why);
    CHECK(!ok);
    CHECK(ok || (why && *why));
  };
  ColpackHeader h;
  auto with = [&](const ColpackHeader& hh) {
    std::vector<uint8_t> v = good;
    std::memcpy(v.data(), &hh, sizeof(hh));
    return v;
  };
  std::memcpy(&h, good.data(), sizeof(h));
  ColpackHeader x = h;
  x.magic ^= 1;
  rejected(with(x), len, L, n);
  x = h;
  x.version = 7;
  rejected(with(x), len, L, n);
  x = h;
  x.record_bytes = (uint32_t)L + 8;
  rejected(with(x), len, L, n);
  rejected(with(x), len, 0, 0);  // the groups no longer match the length
  x = h;
  x.record_bytes = 0;
  rejected(with(x), len, 0, 0);
  x = h;
  x.record_bytes = 100000;
  rejected(with(x), len, 0, 0);
  x = h;
  x.stride += 1;
  rejected(with(x), len, L, n);
  x = h;
  x.stride = 0;
  rejected(with(x), len, L, n);
  x = h;
  x.records = (uint64_t)n + 1;
  rejected(with(x), len, L, n);
  x.records = (uint64_t)n + 64;  // more rows than the piece holds, whatever its padding
  rejected(with(x), len, L, 0);
  x = h;
  x.records = ~0ull;
  rejected(with(x), len, L, 0);
  x = h;
  x.records = 0;
  rejected(with(x), len, L, 0);
  x = h;
  x.groups += 1;
  rejected(with(x), len, L, n);
  x = h;
  x.gb[0] = 9;
  rejected(with(x), len, L, n);
  x = h;
  x.mask[0] ^= 0x02;
  rejected(with(x), len, L, n);
  // truncated pieces: every length short of the whole piece
  for (int64_t k = 0; k < len; k += (k < (int64_t)kColpackHeaderBytes + 8 ? 1 : 61)) rejected(good, k, L, n);
  rejected(good, len - 1, L, n);
  // a null piece
  ColpackPiece q;
  CHECK(!colpack_open(nullptr, 0, L, n, &q));
}

int main() {
  std::mt19937_64 rng(42);
  // TeraSort layout: header bytes, key, 0x5A, letters
  {
    std::vector<int> lo(104, 'A'), span(104, 25);
    lo[0] = 0x0B, lo[1] = 0x5B, lo[2] = 0x0A, lo[13] = 0x5A;
    span[0] = span[1] = span[2] = span[13] = 0;
    for (int c = 3; c < 13; ++c) lo[c] = 0, span[c] = 255;
    const int64_t counts[] = {1, 7, 255, 256, 257, 10082, 10083};
    for (int64_t n : counts) roundtrip(make(n, 104, lo, span, rng), 104, true);
    rejections(make(300, 104, lo, span, rng), 104);
  }
  // width boundaries in one column, the rest constant
  const int spans[] = {0, 1, 127, 128, 255};
  for (int s : spans) {
    std::vector<int> lo(104, 7), span(104, 0);
    lo[21] = s == 255 ? 0 : 3;
    span[21] = s;
    roundtrip(make(500, 104, lo, span, rng), 104, true);
  }
  // one group of eight 8-bit columns among constant groups; all constant; incompressible
  {
    std::vector<int> lo(104, 9), span(104, 0);
    for (int c = 40; c < 48; ++c) lo[c] = 0, span[c] = 255;
    roundtrip(make(2000, 104, lo, span, rng), 104, true);
    roundtrip(make(1000, 104, std::vector<int>(104, 200), std::vector<int>(104, 0), rng), 104, true);
    roundtrip(make(3000, 104, std::vector<int>(104, 0), std::vector<int>(104, 255), rng), 104, false);
  }
  // tail groups: record lengths that are no multiple of 8
  const int lens[] = {1, 5, 7, 9, 13, 100, 255, 256};
  for (int L : lens) {
    roundtrip(make(333, L, std::vector<int>((size_t)L, 48), std::vector<int>((size_t)L, 9), rng), L, L > 1);
    if (L > 1) rejections(make(50, L, std::vector<int>((size_t)L, 48), std::vector<int>((size_t)L, 9), rng), L);
  }
  // out-of-range arguments
  {
    uint8_t b[8] = {0};
    std::vector<uint8_t> d((size_t)colpack_bound(8, 1));
    CHECK(colpack_encode(b, 0, 8, 1, d.data()) == 0);
    CHECK(colpack_encode(b, 1, 0, 1, d.data()) == 0);
    CHECK(colpack_encode(b, 1, 257, 1, d.data()) == 0);
  }
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
