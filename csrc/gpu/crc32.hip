// CRC32 (zlib / IEEE, reflected 0xEDB88320) of device-resident byte ranges: the IFile checksum of the
// partitions a reduce task fetched (uda/ifile.h), in one batched launch per task. See kernels.h.
//
// Two levels. A range is cut into chunks of 256 KiB at 16-byte-aligned ADDRESSES (the first chunk starts
// at the range's first byte, wherever that lies); one wave computes each chunk's CRC state, a second
// kernel folds a range's chunk states in order.
//
// Chunk kernel. CRC is linear over GF(2), so the 64 lanes of a wave need not own contiguous bytes:
// lane l takes the 16-byte words l, l + 64, ... of the chunk (one coalesced 1 KiB row per load) and
// accumulates, per word, acc = acc * x^(8 * 1024) + crc16(word): its own bytes in place and zeros where
// the other lanes' bytes are. The rows are aligned to the END of the word range (virtual zero words in
// front, which leave a zero state zero), so after the last row lane l is always 63 - l words short of
// the end: a per-lane constant multiply, then an xor-reduction over the lanes. Up to 15 bytes before
// the first aligned word and after the last go bytewise; the state ahead of the first word (the CRC's
// 0xFFFFFFFF preset in a range's first chunk, carried over the head bytes) is xored into that word.
//
// Tables: 16 byte tables of slice-by-16 and 4 of the x^(8 * 1024) multiply, built at compile time
// (crc32_tables.h), 20 KiB staged in LDS per workgroup of 4 waves. The gfx950 ISA has no carry-less
// multiply, so table lookups it is. Every lookup is a ds_read_b32 at a data-dependent index: banked
// (a / 4) % 32 within each 32-lane half (lanes l and l + 32 never conflict). A table is 256 consecutive
// dwords, so entry b lies on bank b % 32 and 32 random bytes land ~3.5 deep on the fullest bank;
// replicating a table per lane to avoid that would take 32 KiB per table. Nibble tables could be
// replicated per bank (2 KiB each, conflict-free) but double the lookups and their address arithmetic,
// and the VALU work per lookup, not the LDS, is the larger share per byte already. Wider slices than 16
// only add tables: one 16-byte load per lane and row is what the memory system coalesces best.
//
// Fold kernel: one wave per range. Every chunk but a range's first and last holds exactly 256 KiB,
// and the first one's missing front does not matter (zeros ahead of a zero state), so the states of
// all chunks but the last fold with one constant per lane (x^(8 * 256 KiB * d)) and an xor-reduction,
// 64 chunks per step; the result is carried over the last chunk's length (square and multiply, once
// per range) and xored with the last chunk's state.
//
// State mode (launch_crc32_states, the kState instantiations): the raw register after a range from a ZERO
// register, no preset and no final inversion, so a host can chain ranges of one stream:
// s' = s * x^(8 * len) + state (uda::crc32_fold_state). A range's first chunk then starts from 0 like
// every other chunk. The virtual zero words in front of a chunk's rows, and the first chunk's missing
// front in the fold, rest on "zeros ahead of a zero state leave it zero"; that holds for a zero
// register unchanged (it is where the preset mode's argument starts: its preset enters behind them).
#include <stdexcept>

#include "crc32_tables.h"
#include "kernels.h"

namespace uda {
namespace gpu {

namespace {
using namespace crc32tab;

constexpr int kCrcWaves = 4;
constexpr int kCrcThreads = kCrcWaves * kLanes;

__device__ const ByteTables g_bytes = make_byte_tables();
__device__ const FoldTables g_fold = make_fold_tables();

__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll 8
  for (int i = 0; i < 32; ++i) {
    p ^= b & (0u - (a >> 31));
    a <<= 1;
    b = (b >> 1) ^ (kPoly & (0u - (b & 1)));
  }
  return p;
}

// x^(8 * n)
__device__ uint32_t gf_xpow8(uint64_t n) {
  uint32_t pw = 0x80000000u, sq = 0x00800000u;  // x^0, x^8
  for (; n; n >>= 1) {
    if (n & 1) pw = gf_mul(pw, sq);
    sq = gf_mul(sq, sq);
  }
  return pw;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d, 64);
  return v;
}

// tab: the byte tables in LDS, [table][byte]
__device__ __forceinline__ uint32_t crc_byte(const uint32_t* tab, uint32_t s, uint8_t b) {
  return tab[(s ^ b) & 0xFF] ^ (s >> 8);
}

// acc * x^(8 * 1024) + the state of the 16 bytes of w from a zero state
__device__ __forceinline__ uint32_t crc_step(const uint32_t* tab, uint32_t acc, const uint4& w) {
  uint32_t r = tab[16 * 256 + (acc & 0xFF)] ^ tab[17 * 256 + ((acc >> 8) & 0xFF)] ^
               tab[18 * 256 + ((acc >> 16) & 0xFF)] ^ tab[19 * 256 + (acc >> 24)];
  r ^= tab[15 * 256 + (w.x & 0xFF)] ^ tab[14 * 256 + ((w.x >> 8) & 0xFF)] ^ tab[13 * 256 + ((w.x >> 16) & 0xFF)] ^
       tab[12 * 256 + (w.x >> 24)];
  r ^= tab[11 * 256 + (w.y & 0xFF)] ^ tab[10 * 256 + ((w.y >> 8) & 0xFF)] ^ tab[9 * 256 + ((w.y >> 16) & 0xFF)] ^
       tab[8 * 256 + (w.y >> 24)];
  r ^= tab[7 * 256 + (w.z & 0xFF)] ^ tab[6 * 256 + ((w.z >> 8) & 0xFF)] ^ tab[5 * 256 + ((w.z >> 16) & 0xFF)] ^
       tab[4 * 256 + (w.z >> 24)];
  r ^= tab[3 * 256 + (w.w & 0xFF)] ^ tab[2 * 256 + ((w.w >> 8) & 0xFF)] ^ tab[1 * 256 + ((w.w >> 16) & 0xFF)] ^
       tab[0 * 256 + (w.w >> 24)];
  return r;
}

// chunk_crc[c]: the CRC state (not inverted) at the end of chunk c from a zero state at its start, or
// from the 0xFFFFFFFF preset for a range's first chunk (kState: from a zero state there too)
template <bool kState>
__global__ void __launch_bounds__(kCrcThreads) crc32_chunks_kernel(const CrcDesc* descs, int n, const int64_t* chunk_first,
                                                                   int64_t total_chunks, uint32_t* chunk_crc) {
  __shared__ uint32_t tab[kTables * 256];
  {
    const uint32_t* src = &g_bytes.t[0][0];
    for (int i = threadIdx.x; i < kTables * 256; i += kCrcThreads) tab[i] = src[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & (kLanes - 1);
  const int64_t wave = (int64_t)blockIdx.x * kCrcWaves + (threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * kCrcWaves;
  for (int64_t c = wave; c < total_chunks; c += waves) {
    // the range of chunk c: the last i with chunk_first[i] <= c (ranges without chunks share their
    // successor's chunk_first and lose the tie)
    int lo = 0, hi = n;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (chunk_first[mid] <= c) lo = mid;
      else hi = mid;
    }
    const CrcDesc d = descs[lo];
    const int64_t k = c - chunk_first[lo];
    const uintptr_t base = (uintptr_t)d.p, end = base + (uintptr_t)d.len;
    const uintptr_t grid0 = base & ~(uintptr_t)15;  // chunk boundaries: grid0 + j * kChunkBytes
    uintptr_t b = grid0 + (uintptr_t)k * kChunkBytes, e = b + kChunkBytes;
    if (b < base) b = base;
    if (e > end) e = end;
    uintptr_t w0 = (b + 15) & ~(uintptr_t)15;  // [b, w0) head bytes, [w0, w1) words, [w1, e) tail bytes
    if (w0 > e) w0 = e;
    uintptr_t w1 = e & ~(uintptr_t)15;
    if (w1 < w0) w1 = w0;
    uint32_t st = !kState && k == 0 ? 0xFFFFFFFFu : 0u;
    for (const uint8_t* q = (const uint8_t*)b; q < (const uint8_t*)w0; ++q) st = crc_byte(tab, st, *q);
    const int64_t nw = (int64_t)((w1 - w0) >> 4);
    if (nw > 0) {
      const int64_t z = (kLanes - (nw & (kLanes - 1))) & (kLanes - 1);  // virtual zero words in front
      const int64_t rows = (z + nw) >> 6;
      const uint4* wp = reinterpret_cast<const uint4*>(w0);
      const uint4 zero = make_uint4(0, 0, 0, 0);
      int64_t j = (int64_t)lane - z;  // this lane's word of row 0 (none if negative)
      uint4 w = j >= 0 ? wp[j] : zero;
      if (j == 0) w.x ^= st;  // the state ahead of the first word continues into it
      uint32_t acc = crc_step(tab, 0u, w);
      j += kLanes;
      int64_t r = 1;
      for (; r + 4 <= rows; r += 4, j += 4 * kLanes) {  // four loads in flight per lane
        const uint4 a0 = wp[j], a1 = wp[j + kLanes], a2 = wp[j + 2 * kLanes], a3 = wp[j + 3 * kLanes];
        acc = crc_step(tab, acc, a0);
        acc = crc_step(tab, acc, a1);
        acc = crc_step(tab, acc, a2);
        acc = crc_step(tab, acc, a3);
      }
      for (; r < rows; ++r, j += kLanes) acc = crc_step(tab, acc, wp[j]);
      st = wave_xor(gf_mul(acc, g_fold.lane[kLanes - 1 - lane]));
    }
    for (const uint8_t* q = (const uint8_t*)w1; q < (const uint8_t*)e; ++q) st = crc_byte(tab, st, *q);
    if (lane == 0) chunk_crc[c] = st;
  }
}

// out[i]: the CRC of range i; kState: its raw state, not inverted
template <bool kState>
__global__ void __launch_bounds__(kLanes) crc32_fold_kernel(const CrcDesc* descs, int n, const int64_t* chunk_first,
                                                            const uint32_t* chunk_crc, uint32_t* out) {
  const int i = blockIdx.x;
  if (i >= n) return;
  const int lane = threadIdx.x;
  const int64_t c0 = chunk_first[i], nc = chunk_first[i + 1] - c0;
  if (nc <= 0) {  // no bytes: crc32(b"") == 0, and a zero state stays zero
    if (lane == 0) out[i] = 0;
    return;
  }
  uint32_t f = 0;
  const int64_t n1 = nc - 1;  // chunks ahead of the last one: each ends a whole chunk before the next does
  if (n1 > 0) {
    const int64_t z = (kLanes - (n1 & (kLanes - 1))) & (kLanes - 1);
    const int64_t groups = (z + n1) >> 6;
    const uint32_t mine = g_fold.chunk[kLanes - 1 - lane], group = g_fold.chunk[kLanes];
    for (int64_t g = 0; g < groups; ++g) {
      const int64_t idx = g * kLanes + lane - z;
      const uint32_t v = idx >= 0 ? chunk_crc[c0 + idx] : 0u;
      f = gf_mul(f, group) ^ wave_xor(gf_mul(v, mine));
    }
    const CrcDesc d = descs[i];
    const int64_t last_len = (int64_t)((uintptr_t)d.p & 15) + d.len - n1 * kChunkBytes;
    f = gf_mul(f, gf_xpow8((uint64_t)last_len));
  }
  const uint32_t st = f ^ chunk_crc[c0 + nc - 1];
  if (lane == 0) out[i] = kState ? st : ~st;
}

__global__ void crc32_trailers_kernel(const CrcDesc* descs, int n, uint32_t* stored) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t* t = descs[i].p + descs[i].len;
  stored[i] = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3];
}
}  // namespace

int64_t crc32_chunk_bytes() { return kChunkBytes; }

size_t crc32_ws_bytes(int64_t total_chunks) { return (size_t)(total_chunks > 0 ? total_chunks : 1) * sizeof(uint32_t); }

int64_t crc32_chunk_plan(const CrcDesc* descs, int n, int64_t* chunk_first) {
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    chunk_first[i] = total;
    if (descs[i].len < 0) throw std::invalid_argument("crc32_chunk_plan: negative length");
    if (descs[i].len > 0)
      total += ((int64_t)((uintptr_t)descs[i].p & 15) + descs[i].len + kChunkBytes - 1) / kChunkBytes;
  }
  chunk_first[n] = total;
  return total;
}

namespace {
template <bool kState>
void launch_crc32_mode(const CrcDesc* descs, int n, const int64_t* chunk_first, int64_t total_chunks, void* ws,
                       uint32_t* out, hipStream_t s) {
  if (n <= 0) return;
  if (total_chunks > 0) {
    // enough workgroups to fill the device a few waves deep; a wave strides over the chunks beyond that
    const int64_t want = (total_chunks + kCrcWaves - 1) / kCrcWaves;
    const unsigned blocks = (unsigned)(want < 2048 ? want : 2048);
    hipLaunchKernelGGL(crc32_chunks_kernel<kState>, dim3(blocks), dim3(kCrcThreads), 0, s, descs, n, chunk_first,
                       total_chunks, static_cast<uint32_t*>(ws));
  }
  hipLaunchKernelGGL(crc32_fold_kernel<kState>, dim3((unsigned)n), dim3(kLanes), 0, s, descs, n, chunk_first,
                     static_cast<const uint32_t*>(ws), out);
}
}  // namespace

void launch_crc32(const CrcDesc* descs, int n, const int64_t* chunk_first, int64_t total_chunks, void* ws,
                  uint32_t* out, hipStream_t s) {
  launch_crc32_mode<false>(descs, n, chunk_first, total_chunks, ws, out, s);
}

void launch_crc32_states(const CrcDesc* descs, int n, const int64_t* chunk_first, int64_t total_chunks, void* ws,
                         uint32_t* out, hipStream_t s) {
  launch_crc32_mode<true>(descs, n, chunk_first, total_chunks, ws, out, s);
}

void launch_crc32_trailers(const CrcDesc* descs, int n, uint32_t* stored, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(crc32_trailers_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, descs, n, stored);
}

}  // namespace gpu
}  // namespace uda
