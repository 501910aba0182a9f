// uda_colpack_bench: per-thread rate of the delivery consumers' unpack (codec/colpack.h) on this host,
// with no GPU involved. Every thread owns one packed piece of TeraSort-shaped records (encoded by the
// host reference encoder) and, like a consumer thread, unpacks it 1 MiB buffer by buffer into a
// staging buffer; "unpack+copy" also copies every buffer into a KVBuf as the J2C sink does, and "copy"
// is that memcpy alone from the unpacked records. Rates are in unpacked bytes per second per thread.
//
//   uda_colpack_bench [--threads N] [--mib M] [--reps R] [--scalar] [--v2]
//
// --v2: the piece is a version 2 piece (key differences of the 10-byte key, bit-contiguous rows) of
// sorted records whose keys step as a flagship piece's do (differences of up to 54 bits).
//
// stdout: one JSON line.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "codec/colpack.h"

namespace {

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// [0x0B 0x5B 0x0A] key[10] [0x5A] value[90]: ascending keys in a narrow range, values 'A'..'Z'
void fill(std::vector<uint8_t>& v, int64_t n, uint64_t seed, uint64_t step_mask = 0xFFFFFF) {
  uint64_t key = seed << 40;
  for (int64_t r = 0; r < n; ++r) {
    uint8_t* p = v.data() + r * 104;
    p[0] = 0x0B, p[1] = 0x5B, p[2] = 0x0A, p[13] = 0x5A;
    key += splitmix(seed) & step_mask;
    for (int b = 0; b < 8; ++b) p[3 + b] = (uint8_t)(key >> (56 - 8 * b));
    const uint64_t t = splitmix(seed);
    p[11] = (uint8_t)t, p[12] = (uint8_t)(t >> 8);
    for (int c = 14; c < 104; ++c) p[c] = (uint8_t)('A' + splitmix(seed) % 26);
  }
}

struct Result {
  double unpack = 0, unpack_copy = 0, copy = 0;
  int64_t stride = 0;
};

}  // namespace

int main(int argc, char** argv) {
  int threads = 1, reps = 3;
  int64_t mib = 128;
  bool scalar = false, v2 = false;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--threads" && i + 1 < argc) threads = std::atoi(argv[++i]);
    else if (a == "--mib" && i + 1 < argc) mib = std::atoll(argv[++i]);
    else if (a == "--reps" && i + 1 < argc) reps = std::atoi(argv[++i]);
    else if (a == "--scalar") scalar = true;
    else if (a == "--v2") v2 = true;
    else {
      std::fprintf(stderr, "usage: uda_colpack_bench [--threads N] [--mib M] [--reps R] [--scalar] [--v2]\n");
      return 2;
    }
  }
  threads = threads < 1 ? 1 : threads;
  const int64_t buf_records = (1 << 20) / 104;
  const int64_t n = (mib << 20) / (buf_records * 104) * buf_records;
  if (n < buf_records || reps < 1) return 2;
  std::vector<Result> res((size_t)threads);
  std::vector<std::thread> thr;
  for (int t = 0; t < threads; ++t)
    thr.emplace_back([&, t] {
      std::vector<uint8_t> raw((size_t)(n * 104));
      // --v2: the top 8 key bytes step by up to 2^38, the low two are random: differences below 2^54
      fill(raw, n, 1234567 + (uint64_t)t, v2 ? (1ull << 38) - 1 : 0xFFFFFF);
      std::vector<uint8_t> piece((size_t)(v2 ? uda::colpack2_bound(104, n, buf_records) : uda::colpack_bound(104, n)));
      const int64_t len = v2 ? uda::colpack2_encode(raw.data(), n, 104, buf_records, 3, 10, piece.data())
                             : uda::colpack_encode(raw.data(), n, 104, buf_records, piece.data());
      uda::ColpackPiece p;
      if (!uda::colpack_open(piece.data(), len, 104, n, &p) || !p.packed || p.delta != v2) return;
      res[(size_t)t].stride = p.stride;
      std::vector<uint8_t> stg((size_t)(buf_records * 104) * 2), kv((size_t)(buf_records * 104));
      auto pass = [&](int mode) {  // 0: unpack, 1: unpack + copy, 2: copy
        double best = 0;
        for (int r = 0; r < reps; ++r) {
          const double t0 = now_s();
          int64_t turn = 0;
          for (int64_t row = 0; row < n; row += buf_records) {
            uint8_t* s = stg.data() + (size_t)(turn++ & 1) * (size_t)(buf_records * 104);
            if (mode != 2) {
              if (scalar) uda::colpack_unpack_scalar(p, row, buf_records, s);
              else uda::colpack_unpack(p, row, buf_records, s);
            }
            if (mode == 1) std::memcpy(kv.data(), s, kv.size());
            if (mode == 2) std::memcpy(kv.data(), raw.data() + row * 104, kv.size());
            asm volatile("" ::"r"(kv.data()), "r"(s) : "memory");
          }
          const double rate = (double)(n * 104) / (now_s() - t0);
          if (rate > best) best = rate;
        }
        return best;
      };
      res[(size_t)t].unpack = pass(0);
      res[(size_t)t].unpack_copy = pass(1);
      res[(size_t)t].copy = pass(2);
    });
  for (auto& t : thr) t.join();
  double u = 0, uc = 0, c = 0;
  for (const Result& r : res) {
    if (r.stride == 0) {
      std::fprintf(stderr, "a thread's piece did not pack\n");
      return 1;
    }
    u += r.unpack, uc += r.unpack_copy, c += r.copy;
  }
  std::printf("{\"threads\": %d, \"mib_per_thread\": %lld, \"version\": %d, \"stride\": %lld, \"bmi2\": %s, \"path\": \"%s\", "
              "\"unpack_GBps_per_thread\": %.2f, \"unpack_copy_GBps_per_thread\": %.2f, \"copy_GBps_per_thread\": %.2f}\n",
              threads, (long long)mib, v2 ? 2 : 1, (long long)res[0].stride, uda::colpack_have_bmi2() ? "true" : "false",
              scalar || !uda::colpack_have_bmi2() ? "scalar" : "bmi2", u / threads / 1e9, uc / threads / 1e9,
              c / threads / 1e9);
  return 0;
}
