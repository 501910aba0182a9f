// XXH64 (seed 0) of device-resident byte ranges: the content checksum of zstd frames decoded by zstd.hip is its
// low 32 bits. Launched only when a frame of the task carries that checksum (Hadoop's frames should not).
//
// Four lanes per range hold XXH64's four accumulators: lane j takes bytes [32 i + 8 j, 32 i + 8 j + 8) of stripe
// i, so a stripe is one 32-byte access of the four lanes and sixteen ranges share a wave. Then lane 0 of the four
// merges the accumulators and runs the tail (under 32 bytes). Every load lies inside its range: a stripe is read
// only when all 32 of its bytes are there, the tail byte by byte below the range's end.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace uda {
namespace gpu {

namespace {

constexpr uint64_t kP1 = 0x9E3779B185EBCA87ull, kP2 = 0xC2B2AE3D27D4EB4Full, kP3 = 0x165667B19E3779F9ull,
                   kP4 = 0x85EBCA77C2B2AE63ull, kP5 = 0x27D4EB2F165667C5ull;
constexpr int kThreads = 64;
constexpr int kRangesPerBlock = kThreads / 4;

struct __attribute__((packed, aligned(1))) U64p {
  uint64_t v;
};

__device__ __forceinline__ uint64_t rotl(uint64_t v, int r) { return (v << r) | (v >> (64 - r)); }
__device__ __forceinline__ uint64_t xround(uint64_t acc, uint64_t in) { return rotl(acc + in * kP2, 31) * kP1; }
__device__ __forceinline__ uint64_t xmerge(uint64_t h, uint64_t v) { return (h ^ xround(0, v)) * kP1 + kP4; }
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}

__global__ void __launch_bounds__(kThreads) xxh64_kernel(const uint8_t* const* ptrs, const int64_t* lens, int n, uint64_t* out) {
  const int lane = (int)threadIdx.x, j = lane & 3;
  const int idx = (int)blockIdx.x * kRangesPerBlock + (lane >> 2);
  const bool live = idx < n;  // (no early return: the shuffles below are wave-wide)
  const uint8_t* p = live ? ptrs[idx] : nullptr;
  const int64_t len = live ? lens[idx] : 0;
  uint64_t acc = j == 0 ? kP1 + kP2 : j == 1 ? kP2 : j == 2 ? 0 : 0 - kP1;
  const int64_t stripes = len >> 5;
  for (int64_t i = 0; i < stripes; ++i) acc = xround(acc, reinterpret_cast<const U64p*>(p + 32 * i + 8 * j)->v);
  const int first = lane & ~3;
  const uint64_t v0 = shfl64(acc, first), v1 = shfl64(acc, first + 1), v2 = shfl64(acc, first + 2), v3 = shfl64(acc, first + 3);
  if (!live || j != 0) return;
  uint64_t h;
  if (len >= 32) {
    h = rotl(v0, 1) + rotl(v1, 7) + rotl(v2, 12) + rotl(v3, 18);
    h = xmerge(h, v0);
    h = xmerge(h, v1);
    h = xmerge(h, v2);
    h = xmerge(h, v3);
  } else {
    h = kP5;
  }
  h += (uint64_t)len;
  int64_t at = stripes << 5;
  auto byte = [&](int64_t k) { return (uint64_t)p[k]; };
  for (; at + 8 <= len; at += 8) {
    uint64_t w = 0;
    for (int k = 0; k < 8; ++k) w |= byte(at + k) << (8 * k);
    h = rotl(h ^ xround(0, w), 27) * kP1 + kP4;
  }
  if (at + 4 <= len) {
    uint64_t w = 0;
    for (int k = 0; k < 4; ++k) w |= byte(at + k) << (8 * k);
    h = rotl(h ^ (w * kP1), 23) * kP2 + kP3;
    at += 4;
  }
  for (; at < len; ++at) h = rotl(h ^ (byte(at) * kP5), 11) * kP1;
  h ^= h >> 33;
  h *= kP2;
  h ^= h >> 29;
  h *= kP3;
  h ^= h >> 32;
  out[idx] = h;
}

}  // namespace

void launch_xxh64(const uint8_t* const* ptrs, const int64_t* lens, int n, uint64_t* out, hipStream_t s) {
  if (n <= 0) return;
  const int blocks = (n + kRangesPerBlock - 1) / kRangesPerBlock;
  hipLaunchKernelGGL(xxh64_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, ptrs, lens, n, out);
}

}  // namespace gpu
}  // namespace uda
