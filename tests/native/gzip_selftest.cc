// Stand-alone memory-safety check of the host inflater in gzip mode (gzip_decompress and the gzip Inflater of
// csrc/codec/inflate.cc), meant to be built together with that file under AddressSanitizer + UBSan and run on a
// CPU machine:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Icsrc/include \
//       tests/native/gzip_selftest.cc csrc/codec/inflate.cc -o build/gzip_selftest
//   build/gzip_selftest <case directory>
//
// The case directory is what tests/test_gzip_codec.py dumps from tests/gzip_cases.py (members that Python's
// zlib module has judged): a file `manifest` with one line per case, "V <name>" (one valid member), "M <name>"
// (several) or "I <name>", and per case <name>.in and, for a valid one, <name>.out (the bytes it decodes to).
// Every call gets heap copies of exactly the input's and the output's size, so a read or write one byte
// outside either is a sanitizer report. Valid cases must decode to their bytes, one shot and incrementally at
// several feed and read sizes (1 byte at a time cuts every header field and the trailer at every place), and
// must be refused with one byte of output less; invalid ones must be refused or never finish. Every proper
// prefix of the short single members must be refused, and a few thousand single-byte
// mutations run for memory safety alone (a mutation may still be valid).
// Exit status 0: all as expected; 1: a wrong acceptance, a wrong rejection or wrong bytes.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "uda/codec.h"
#include "uda/error.h"

namespace {

using Bytes = std::vector<uint8_t>;
int checks = 0, failures = 0;

void expect(bool ok, const std::string& what) {
  ++checks;
  if (!ok) {
    ++failures;
    std::printf("FAIL %s\n", what.c_str());
  }
}

bool read_file(const std::string& path, Bytes* out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  out->assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  return true;
}

// exact-size heap copy (a vector's capacity may exceed its size)
std::unique_ptr<uint8_t[]> exact(const Bytes& b) {
  std::unique_ptr<uint8_t[]> p(new uint8_t[b.size() ? b.size() : 1]);
  if (!b.empty()) std::memcpy(p.get(), b.data(), b.size());
  return p;
}

bool one_shot(const Bytes& in, size_t cap, Bytes* out, size_t* used) {
  auto src = exact(in);
  std::unique_ptr<uint8_t[]> dst(new uint8_t[cap ? cap : 1]);
  size_t n = 0;
  const bool ok = uda::gzip_decompress(src.get(), in.size(), dst.get(), cap, &n, used);
  out->assign(dst.get(), dst.get() + (ok ? n : 0));
  return ok;
}

// 1 = finished with these bytes and every input byte taken, 0 = never finished (or input left), -1 = refused
int incremental(const Bytes& in, size_t feed, size_t read, Bytes* out) {
  out->clear();
  try {
    uda::Inflater inf(uda::Inflater::Container::kGzip);
    std::unique_ptr<uint8_t[]> buf(new uint8_t[read]);
    for (size_t off = 0; off < in.size() || off == 0; off += feed) {
      const size_t k = off < in.size() ? std::min(feed, in.size() - off) : 0;
      Bytes piece(in.begin() + (long)off, in.begin() + (long)(off + k));
      auto p = exact(piece);
      inf.feed(p.get(), k);
      for (size_t n; (n = inf.read(buf.get(), read)) > 0;) out->insert(out->end(), buf.get(), buf.get() + n);
      if (in.empty()) break;
    }
    (void)inf.read(buf.get(), read);  // (a last member of no output is entered only by a read)
    return inf.finished() && inf.idle() && inf.consumed() == in.size() ? 1 : 0;
  } catch (const uda::UdaError&) {
    return -1;
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: gzip_selftest <case directory>\n");
    return 2;
  }
  const std::string dir = argv[1];
  std::ifstream mf(dir + "/manifest");
  if (!mf) {
    std::printf("no manifest in %s\n", dir.c_str());
    return 2;
  }
  std::vector<std::pair<Bytes, Bytes>> shorts;  // short valid cases for the prefix and mutation runs
  std::string kind, name;
  int valid = 0, invalid = 0;
  while (mf >> kind >> name) {
    Bytes in, want, got;
    if (!read_file(dir + "/" + name + ".in", &in)) {
      expect(false, name + ": no .in file");
      continue;
    }
    if (kind == "V" || kind == "M") {
      ++valid;
      if (!read_file(dir + "/" + name + ".out", &want)) {
        expect(false, name + ": no .out file");
        continue;
      }
      size_t used = 0;
      expect(one_shot(in, want.size(), &got, &used) && got == want && used == in.size(), name + ": one shot");
      if (!want.empty()) expect(!one_shot(in, want.size() - 1, &got, &used), name + ": one byte of room too few");
      for (size_t feed : {(size_t)1, (size_t)7, (size_t)4096})
        for (size_t read : {(size_t)1, (size_t)13, (size_t)65536}) {
          if (feed == 1 && in.size() > 4096 && (read == 1 || in.size() > 20000)) continue;  // (quadratic enough)
          expect(incremental(in, feed, read, &got) == 1 && got == want,
                 name + ": feed " + std::to_string(feed) + " read " + std::to_string(read));
        }
      if (kind == "V" && in.size() <= 400 && shorts.size() < 24) shorts.emplace_back(in, want);  // (single members)
    } else {
      ++invalid;
      size_t used = 0;
      expect(!one_shot(in, 1 << 20, &got, &used), name + ": one shot accepted");
      for (size_t feed : {(size_t)1, (size_t)7, (size_t)4096})
        expect(incremental(in, feed, 4096, &got) != 1, name + ": accepted at feed " + std::to_string(feed));
    }
  }
  expect(valid >= 65 && invalid >= 50, "case counts " + std::to_string(valid) + " / " + std::to_string(invalid));
  uint32_t rng = 54321;
  int mutations = 0;
  for (const auto& sw : shorts) {
    const Bytes& in = sw.first;
    Bytes got;
    size_t used = 0;
    for (size_t k = 0; k < in.size(); ++k) {
      Bytes cut(in.begin(), in.begin() + (long)k);
      expect(!one_shot(cut, sw.second.size(), &got, &used), "prefix " + std::to_string(k) + " accepted");
    }
    for (int m = 0; m < 60; ++m) {
      rng = rng * 1664525u + 1013904223u;
      Bytes mut = in;
      mut[(rng >> 8) % mut.size()] ^= (uint8_t)(1u << ((rng >> 4) & 7));
      const bool ok = one_shot(mut, sw.second.size() + 64, &got, &used);
      expect(!ok || got.size() <= sw.second.size() + 64, "mutation past cap");
      (void)incremental(mut, 5, 33, &got);
      ++mutations;
    }
  }
  std::printf("%d valid, %d invalid cases, %zu short streams, %d mutations: %d checks, %d failures\n", valid, invalid,
              shorts.size(), mutations, checks, failures);
  return failures ? 1 : 0;
}
