// Adler-32 (RFC 1950) of device-resident byte ranges in one launch: the integrity check a zlib stream carries
// over its decoded bytes, run right behind the inflate launch (inflate.hip) and compared on the host.
//
// For a range x[0, n):  a = 1 + sum x[i],  b = n + sum (n - i) * x[i]   (both mod 65521),  adler = b << 16 | a.
// Both sums split over any partition of the range, a byte's weight n - i being its distance to the range's
// end, so a range is summed by kPiecesPerRange workgroups striding over its 4 KiB pieces: a thread takes 16
// bytes at offset j of the range (one unaligned 16-byte load), adds  ((n - j) mod 65521) * sum x[k]  and
// subtracts  sum k * x[k]  (k = 0..15). One modulo per 16 bytes; every product is below 2^28 and the
// accumulators are 64-bit, so nothing overflows for any length. The workgroups' residues are added into two
// 64-bit words per range (atomics) and a second kernel folds them into the 32-bit value.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "kernels.h"

namespace uda {
namespace gpu {

namespace {

constexpr uint32_t kMod = 65521;
constexpr int kThreads = 256;
constexpr int kLaneBytes = 16;
constexpr int64_t kPieceBytes = (int64_t)kThreads * kLaneBytes;
constexpr int kPiecesPerRange = 32;  // workgroups per range (grid.x)
constexpr int kMaxRangesPerLaunch = 32768;

struct __attribute__((packed, aligned(1))) U128 {
  uint32_t a, b, c, d;
};

__device__ __forceinline__ void add_word(uint32_t w, uint32_t k0, uint32_t& a, uint32_t& kx) {
  const uint32_t x0 = w & 0xFF, x1 = (w >> 8) & 0xFF, x2 = (w >> 16) & 0xFF, x3 = w >> 24;
  a += x0 + x1 + x2 + x3;
  kx += k0 * x0 + (k0 + 1) * x1 + (k0 + 2) * x2 + (k0 + 3) * x3;
}

__global__ void __launch_bounds__(kThreads)
adler32_sum_kernel(const uint8_t* const* ptrs, const int64_t* lens, int first, unsigned long long* work) {
  const int r = first + (int)blockIdx.y;
  const uint8_t* p = ptrs[r];
  const int64_t n = lens[r];
  uint64_t s1 = 0, pos = 0, neg = 0;
  for (int64_t i0 = (int64_t)blockIdx.x * kPieceBytes; i0 < n; i0 += (int64_t)gridDim.x * kPieceBytes) {
    const int64_t j = i0 + (int64_t)threadIdx.x * kLaneBytes;
    if (j >= n) continue;
    uint32_t a = 0, kx = 0;
    if (j + kLaneBytes <= n) {
      const U128 v = *reinterpret_cast<const U128*>(p + j);
      add_word(v.a, 0, a, kx);
      add_word(v.b, 4, a, kx);
      add_word(v.c, 8, a, kx);
      add_word(v.d, 12, a, kx);
    } else {
      for (int k = 0; j + k < n; ++k) {
        const uint32_t x = p[j + k];
        a += x;
        kx += (uint32_t)k * x;
      }
    }
    s1 += a;
    pos += (uint64_t)((uint64_t)(n - j) % kMod) * a;
    neg += kx;
  }
  unsigned long long r1 = s1 % kMod, r2 = (pos % kMod + kMod - neg % kMod) % kMod;
  for (int off = 32; off > 0; off >>= 1) {
    r1 += __shfl_down(r1, off, 64);
    r2 += __shfl_down(r2, off, 64);
  }
  __shared__ unsigned long long part[2][kThreads / 64];
  const int wave = (int)(threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0) {
    part[0][wave] = r1;
    part[1][wave] = r2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t1 = 0, t2 = 0;
    for (int w = 0; w < kThreads / 64; ++w) {
      t1 += part[0][w];
      t2 += part[1][w];
    }
    if (t1) atomicAdd(&work[2 * r], t1);
    if (t2) atomicAdd(&work[2 * r + 1], t2);
  }
}

__global__ void adler32_fold_kernel(const int64_t* lens, int n, const unsigned long long* work, uint32_t* out) {
  const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (r >= n) return;
  const uint32_t a = (uint32_t)((1 + work[2 * r]) % kMod);
  const uint32_t b = (uint32_t)(((uint64_t)lens[r] % kMod + work[2 * r + 1]) % kMod);
  out[r] = (b << 16) | a;
}

}  // namespace

void launch_adler32(const uint8_t* const* ptrs, const int64_t* lens, int n, uint32_t* out, uint64_t* work, hipStream_t s) {
  if (n <= 0) return;
  auto* w = reinterpret_cast<unsigned long long*>(work);
  // (a failed memset would leave stale sums and read as an Adler-32 mismatch of good data: say what failed)
  const hipError_t e = hipMemsetAsync(w, 0, (size_t)n * 2 * sizeof(unsigned long long), s);
  if (e != hipSuccess) throw std::runtime_error(std::string("launch_adler32: hipMemsetAsync: ") + hipGetErrorString(e));
  for (int first = 0; first < n; first += kMaxRangesPerLaunch) {
    const int m = n - first < kMaxRangesPerLaunch ? n - first : kMaxRangesPerLaunch;
    hipLaunchKernelGGL(adler32_sum_kernel, dim3(kPiecesPerRange, (unsigned)m), dim3(kThreads), 0, s, ptrs, lens, first, w);
  }
  hipLaunchKernelGGL(adler32_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lens, n, w, out);
}

}  // namespace gpu
}  // namespace uda
