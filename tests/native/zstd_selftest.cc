// Stand-alone memory-safety check of the host zstd codec (zstd_decompress, ZstdDecoder and zstd_compress of
// csrc/codec/zstd.cc with the table builders of csrc/codec/zstd_tables.h, which the device kernel runs too), meant
// to be built together with that file under AddressSanitizer + UBSan and run on a CPU machine:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Icsrc/include \
//       tests/native/zstd_selftest.cc csrc/codec/zstd.cc -o build/zstd_selftest
//   build/zstd_selftest <case directory>
//
// The case directory is what tests/test_zstd_codec.py dumps from tests/zstd_cases.py and tests/zstd_vectors.py
// (frames that libzstd has judged or written): a file `manifest` with one line per case, "V <name>" (valid),
// "W <name>" (valid, but the incremental decoder refuses it: a Window_Size above its limit, or an offset beyond
// Window_Size) or "I <name>" (invalid), and
// per case <name>.in and, for a valid one, <name>.out (the bytes it decodes to).
// Every call gets heap copies of exactly the input's and the output's size, so a read or write one byte outside
// either is a sanitizer report. Valid cases must decode to their bytes, one shot and incrementally at several feed
// and read sizes, and must be refused with one byte of output less; invalid ones must be refused or never finish.
// Every proper prefix of the short frames must be refused, a few thousand single-byte mutations of frames with
// Huffman literals and described tables run for memory safety alone (a mutation may still be valid), and the
// encoder's output must come back through the decoder at sizes around its block and count boundaries.
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
  const bool ok = uda::zstd_decompress(src.get(), in.size(), dst.get(), cap, &n, used);
  out->assign(dst.get(), dst.get() + (ok ? n : 0));
  return ok;
}

// 1 = finished with every input byte taken, 0 = never finished (or input left), -1 = refused
int incremental(const Bytes& in, size_t feed, size_t read, Bytes* out) {
  out->clear();
  try {
    uda::ZstdDecoder dec;
    std::unique_ptr<uint8_t[]> buf(new uint8_t[read]);
    for (size_t off = 0; off < in.size(); off += feed) {
      const size_t k = std::min(feed, in.size() - off);
      Bytes piece(in.begin() + (long)off, in.begin() + (long)(off + k));
      auto p = exact(piece);
      dec.feed(p.get(), k);
      for (size_t n; (n = dec.read(buf.get(), read)) > 0;) out->insert(out->end(), buf.get(), buf.get() + n);
    }
    for (size_t n; (n = dec.read(buf.get(), read)) > 0;) out->insert(out->end(), buf.get(), buf.get() + n);
    return dec.finished() && dec.idle() && dec.consumed() == in.size() ? 1 : 0;
  } catch (const uda::UdaError&) {
    return -1;
  }
}

void round_trip(const Bytes& raw, const std::string& what) {
  std::unique_ptr<uint8_t[]> dst(new uint8_t[uda::zstd_max_compressed_length(raw.size())]);
  auto src = exact(raw);
  const size_t n = uda::zstd_compress(src.get(), raw.size(), dst.get());
  expect(n <= uda::zstd_max_compressed_length(raw.size()), what + ": encoder past its bound");
  Bytes frame(dst.get(), dst.get() + n), got;
  size_t used = 0;
  expect(one_shot(frame, raw.size(), &got, &used) && got == raw && used == n, what + ": round trip");
  expect(incremental(frame, 977, 4096, &got) == 1 && got == raw, what + ": round trip, incremental");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: zstd_selftest <case directory>\n");
    return 2;
  }
  const std::string dir = argv[1];
  std::ifstream mf(dir + "/manifest");
  if (!mf) {
    std::printf("no manifest in %s\n", dir.c_str());
    return 2;
  }
  std::vector<std::pair<Bytes, Bytes>> shorts;  // short valid frames for the prefix and mutation runs
  std::string kind, name;
  int valid = 0, invalid = 0;
  while (mf >> kind >> name) {
    Bytes in, want, got;
    if (!read_file(dir + "/" + name + ".in", &in)) {
      expect(false, name + ": no .in file");
      continue;
    }
    if (kind == "V" || kind == "W") {
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
          if ((feed == 1 || read == 1) && in.size() + want.size() > 8192) continue;  // (slow under the sanitizers)
          const int r = incremental(in, feed, read, &got);
          if (kind == "W")
            expect(r == -1, name + ": the incremental decoder took what it is to refuse");
          else
            expect(r == 1 && got == want, name + ": feed " + std::to_string(feed) + " read " + std::to_string(read));
        }
      if (kind == "V" && in.size() <= 1200 && shorts.size() < 40) shorts.emplace_back(in, want);
    } else {
      ++invalid;
      size_t used = 0;
      expect(!one_shot(in, 1 << 20, &got, &used), name + ": one shot accepted");
      for (size_t feed : {(size_t)1, (size_t)7, (size_t)4096})
        expect(incremental(in, feed, 4096, &got) != 1, name + ": accepted at feed " + std::to_string(feed));
    }
  }
  expect(valid >= 65 && invalid >= 20, "case counts " + std::to_string(valid) + " / " + std::to_string(invalid));
  uint32_t rng = 54321;
  int mutations = 0;
  for (const auto& sw : shorts) {
    const Bytes& in = sw.first;
    Bytes got;
    size_t used = 0;
    // (a prefix that ends where a frame ends is a whole stream: multi-frame cases have those)
    for (size_t k = 0; k < in.size() && k < 300; ++k) {
      Bytes cut(in.begin(), in.begin() + (long)k);
      const bool ok = one_shot(cut, sw.second.size(), &got, &used);
      expect(!ok || got.size() < sw.second.size() || got == sw.second, "prefix " + std::to_string(k) + " decoded to other bytes");
    }
    for (int m = 0; m < 120; ++m) {
      rng = rng * 1664525u + 1013904223u;
      Bytes mut = in;
      mut[(rng >> 8) % mut.size()] ^= (uint8_t)(1u << ((rng >> 4) & 7));
      const bool ok = one_shot(mut, sw.second.size() + 64, &got, &used);
      expect(!ok || got.size() <= sw.second.size() + 64, "mutation past cap");
      (void)incremental(mut, 5, 33, &got);
      ++mutations;
    }
  }
  // the encoder: sizes around the block boundary, a repeated byte, records, incompressible bytes
  for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)100, (size_t)131071, (size_t)131072, (size_t)131073, (size_t)300000}) {
    Bytes text(n), same(n, 0x42), noise(n);
    for (size_t i = 0; i < n; ++i) {
      text[i] = (uint8_t)("the quick brown fox jumps over the lazy dog "[(i * 7 + (i >> 6)) % 44]);
      rng = rng * 1664525u + 1013904223u;
      noise[i] = (uint8_t)(rng >> 24);
    }
    round_trip(text, "text " + std::to_string(n));
    round_trip(same, "same " + std::to_string(n));
    round_trip(noise, "noise " + std::to_string(n));
  }
  std::printf("%d valid, %d invalid cases, %zu short frames, %d mutations: %d checks, %d failures\n", valid, invalid,
              shorts.size(), mutations, checks, failures);
  return failures ? 1 : 0;
}
