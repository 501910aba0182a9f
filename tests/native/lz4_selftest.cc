// Stand-alone memory-safety check of the host LZ4 decoder, meant to be built together with
// csrc/codec/lz4.cc under AddressSanitizer + UBSan and run on a CPU machine:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Icsrc/include \
//       tests/native/lz4_selftest.cc csrc/codec/lz4.cc -o build/lz4_selftest && build/lz4_selftest
//
// Every call hands lz4_decompress heap copies of exactly the input's and the output's size, so a read
// or write one byte outside either is a sanitizer report. Hand-assembled vectors, encoder round trips,
// and a few thousand single-byte mutations and truncations of valid streams are compared with a
// slow reference decoder written here from the format (bounds-checked containers, one byte at a time):
// the decoder must accept exactly what the reference accepts within `cap`, with the same bytes.
// Exit status 0: all agreed; 1: a wrong acceptance, a wrong rejection or wrong bytes.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "uda/codec.h"

namespace {

using Bytes = std::vector<uint8_t>;

// Reference: false when the format forbids the stream or the output would pass `cap`.
bool ref_decode(const Bytes& in, size_t cap, Bytes* out) {
  out->clear();
  size_t ip = 0;
  for (;;) {
    if (ip >= in.size()) return false;
    const uint8_t token = in.at(ip++);
    size_t len = token >> 4;
    if (len == 15) {
      uint8_t b;
      do {
        if (ip >= in.size()) return false;
        b = in.at(ip++);
        len += b;
      } while (b == 255);
    }
    for (size_t i = 0; i < len; ++i) {
      if (ip >= in.size() || out->size() >= cap) return false;
      out->push_back(in.at(ip++));
    }
    if (ip == in.size()) return true;
    if (in.size() - ip < 2) return false;
    const size_t off = in.at(ip) | (size_t)in.at(ip + 1) << 8;
    ip += 2;
    if (off == 0 || off > out->size()) return false;
    len = token & 15;
    if (len == 15) {
      uint8_t b;
      do {
        if (ip >= in.size()) return false;
        b = in.at(ip++);
        len += b;
      } while (b == 255);
    }
    len += 4;
    for (size_t i = 0; i < len; ++i) {
      if (out->size() >= cap) return false;
      out->push_back(out->at(out->size() - off));
    }
  }
}

int failures = 0;
long checks = 0;

void fail(const char* what, const std::string& name, size_t a, size_t b) {
  std::fprintf(stderr, "FAIL %s: %s (%zu, %zu)\n", name.c_str(), what, a, b);
  ++failures;
}

// One decoder call on exact-size heap buffers, compared with the reference.
void check(const std::string& name, const Bytes& in, size_t cap) {
  ++checks;
  std::unique_ptr<uint8_t[]> src(new uint8_t[in.size()]);  // new[0] is a valid, unreadable pointer
  if (!in.empty()) std::memcpy(src.get(), in.data(), in.size());
  std::unique_ptr<uint8_t[]> dst(new uint8_t[cap]);
  size_t got = (size_t)-1;
  const bool ok = uda::lz4_decompress(src.get(), in.size(), dst.get(), cap, &got);
  Bytes want;
  const bool ref_ok = ref_decode(in, cap, &want);
  if (ok && !ref_ok) return fail("wrong acceptance", name, in.size(), cap);
  if (!ok && ref_ok) return fail("wrong rejection", name, in.size(), cap);
  if (!ok) return;
  if (got != want.size()) return fail("wrong length", name, got, want.size());
  if (got && std::memcmp(dst.get(), want.data(), got) != 0) fail("wrong bytes", name, got, cap);
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

Bytes cat(std::initializer_list<Bytes> parts) {
  Bytes r;
  for (const Bytes& p : parts) r.insert(r.end(), p.begin(), p.end());
  return r;
}
Bytes pattern(size_t n, uint32_t mul, uint32_t add) {
  Bytes r(n);
  for (size_t i = 0; i < n; ++i) r[i] = (uint8_t)(i * mul + add);
  return r;
}

struct Vec {
  std::string name;
  Bytes stream;
  size_t out_len;
};

std::vector<Vec> vectors() {
  std::vector<Vec> v;
  v.push_back({"literals_only", {0x30, 'a', 'b', 'c'}, 3});
  v.push_back({"empty", {0x00}, 0});
  v.push_back({"offset1_fill", {0x16, 'a', 0x01, 0x00, 0x00}, 11});
  v.push_back({"offset_equals_length", {0x40, 'a', 'b', 'c', 'd', 0x04, 0x00, 0x00}, 8});
  v.push_back({"offset_below_length_over_64", {0x3f, 'a', 'b', 'c', 0x03, 0x00, 0x51, 0x10, 'Z'}, 104});
  v.push_back({"literal_run_15", cat({{0xf0, 0x00}, pattern(15, 1, 65)}), 15});
  v.push_back({"literal_run_270", cat({{0xf0, 0xff, 0x00}, pattern(270, 3, 0)}), 270});
  v.push_back({"literal_run_273", cat({{0xf0, 0xff, 0x03}, pattern(273, 11, 2)}), 273});
  v.push_back({"match_length_19", {0x4f, 'a', 'b', 'c', 'd', 0x04, 0x00, 0x00, 0x00}, 23});
  v.push_back({"match_length_ff_extension", {0x2f, 'x', 'y', 0x02, 0x00, 0xff, 0x07, 0x20, '!', '?'}, 285});
  v.push_back({"literal_run_over_64", cat({{0xf0, 0x55}, pattern(100, 7, 3)}), 100});
  v.push_back({"offset_over_64_short_match", cat({{0xff, 0xb9}, pattern(200, 5, 1), {0x96, 0x00, 0x15, 0x30, 'e', 'n', 'd'}}), 243});
  v.push_back({"offset_65535", cat({{0xf4}, Bytes(256, 0xff), {0xf0}, pattern(65535, 13, 5), {0xff, 0xff, 0x00}}), 65543});
  return v;
}

std::vector<Bytes> payloads() {
  std::vector<Bytes> p;
  p.push_back({});
  p.push_back({'q'});
  p.push_back(Bytes(12, 'a'));
  p.push_back(Bytes(13, 'a'));
  p.push_back(Bytes(70000, 0));
  Bytes r(20000);
  for (auto& b : r) b = (uint8_t)rnd();
  p.push_back(r);
  Bytes mixed;  // runs, short repeats and noise: literal and match extensions, every offset size
  while (mixed.size() < 90000) {
    const uint32_t k = rnd() % 3, n = 1 + rnd() % 400;
    if (k == 0) {
      mixed.insert(mixed.end(), n, (uint8_t)rnd());
    } else if (k == 1 || mixed.size() < 100) {
      for (uint32_t i = 0; i < n; ++i) mixed.push_back((uint8_t)rnd());
    } else {
      const size_t from = rnd() % (mixed.size() - 50);
      for (uint32_t i = 0; i < n && from + i < mixed.size(); ++i) mixed.push_back(mixed[from + i]);
    }
  }
  p.push_back(mixed);
  Bytes text;
  for (int i = 0; text.size() < 30000; ++i) {
    char line[64];
    const int n = std::snprintf(line, sizeof(line), "key%08d\tvalue%d\n", i * 7919 % 100000, i % 97);
    text.insert(text.end(), line, line + n);
  }
  p.push_back(text);
  return p;
}

}  // namespace

int main() {
  std::vector<std::pair<Bytes, size_t>> valid;  // (stream, output length)
  for (const Vec& v : vectors()) {
    Bytes want;
    if (!ref_decode(v.stream, v.out_len, &want) || want.size() != v.out_len) fail("vector is not what it says", v.name, want.size(), v.out_len);
    check(v.name, v.stream, v.out_len);
    if (v.out_len) check(v.name + " cap-1", v.stream, v.out_len - 1);
    check(v.name + " cap+7", v.stream, v.out_len + 7);
    valid.push_back({v.stream, v.out_len});
  }
  int k = 0;
  for (const Bytes& p : payloads()) {
    const std::string name = "payload " + std::to_string(k++);
    Bytes c(uda::lz4_max_compressed_length(p.size()));
    std::unique_ptr<uint8_t[]> src(new uint8_t[p.size()]);
    if (!p.empty()) std::memcpy(src.get(), p.data(), p.size());
    const size_t n = uda::lz4_compress(src.get(), p.size(), c.data());
    if (n > c.size()) fail("encoder passed its bound", name, n, c.size());
    c.resize(n);
    Bytes back;
    if (!ref_decode(c, p.size(), &back) || back != p) fail("encoder output does not decode to the input", name, n, p.size());
    check(name, c, p.size());
    valid.push_back({c, p.size()});
  }
  for (size_t i = 0; i < valid.size(); ++i) {
    const Bytes& s = valid[i].first;
    const size_t cap = valid[i].second;
    const std::string name = "stream " + std::to_string(i);
    // truncations: every prefix of a short stream, 300 random ones of a long one; none may produce `cap` bytes
    // unless the reference agrees (it never does for a stream whose last sequence carries bytes)
    for (int t = 0; t < 300; ++t) {
      const size_t cut = s.size() <= 300 ? (size_t)t : rnd() % s.size();
      if (cut >= s.size()) break;
      check(name + " cut", Bytes(s.begin(), s.begin() + (long)cut), cap);
    }
    // single-byte mutations; tokens, extension bytes and offsets sit at the front of most sequences, and the
    // small streams are all structure
    for (int t = 0; t < 400; ++t) {
      Bytes m = s;
      const size_t at = (t & 1) ? rnd() % m.size() : rnd() % (m.size() < 64 ? m.size() : 64);
      const uint8_t choices[] = {0x00, 0xff, 0x0f, 0xf0, (uint8_t)rnd(), (uint8_t)(m[at] ^ (1u << (rnd() % 8)))};
      m[at] = choices[rnd() % 6];
      check(name + " mutated", m, cap);
    }
  }
  std::printf("lz4_selftest: %ld decoder calls, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
