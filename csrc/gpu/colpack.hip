// colpack on the device: column-range bit-packing of a round's merged output ahead of its D2H
// (format and host reference: codec/colpack.h). Three launches per round over a fixed list of pieces:
//   colpack_stats_kernel  per piece, per column min / max (LDS reduction, one atomic pair per column
//                         per workgroup into the piece's table)
//   colpack_plan_kernel   per piece: widths -> masks, bases, group sizes, stride, packed-or-raw, length;
//                         writes the piece header and the zero padding after the rows
//   colpack_pack_kernel   tiles of records packed into LDS (shift + or, no hardware pext) and written
//                         out with coalesced vector stores; raw pieces are skipped
// A work item is one (record, 8-column group): consecutive lanes read consecutive 8-byte words of the
// record stream when L % 8 == 0 (104-byte TeraSort records: 13 groups).
#include "codec/colpack.h"
#include "kernels.h"

#include <algorithm>

namespace uda {
namespace gpu {

namespace {
constexpr int kCpThreads = 256;
constexpr int kCpTileRows = 128;                      // rows per pack tile: tile starts stay 16-byte aligned
constexpr int kCpTileBytes = kCpTileRows * (9 * kColpackMaxRecordBytes / 10);  // LDS bytes of a packed tile
constexpr int kCpTableStride = 2 * kColpackMaxRecordBytes;  // per piece: min[256] | min of (255 - v)[256]

// The n (<= 8) column bytes at p as a little-endian word.
__device__ __forceinline__ uint64_t load_cols(const uint8_t* p, int n) {
  if (n == 8 && (reinterpret_cast<uintptr_t>(p) & 7) == 0) return *reinterpret_cast<const uint64_t*>(p);
  uint64_t x = 0;
  for (int k = 0; k < n; ++k) x |= (uint64_t)p[k] << (8 * k);
  return x;
}

__global__ void __launch_bounds__(kCpThreads) colpack_stats_kernel(const ColpackPieceDesc* pieces, int L,
                                                                   uint32_t* table) {
  const ColpackPieceDesc pc = pieces[blockIdx.y];
  const int G = (L + 7) / 8;
  const int rows_per_iter = kCpThreads / G;  // threads past rows_per_iter * G idle: a thread keeps its group
  if ((int64_t)blockIdx.x * rows_per_iter >= pc.nrec) return;
  __shared__ uint32_t s_mn[kColpackMaxRecordBytes], s_mx[kColpackMaxRecordBytes];
  const int t = threadIdx.x;
  s_mn[t] = 255;
  s_mx[t] = 0;
  __syncthreads();
  const int g = t % G, rl = t / G;
  if (rl < rows_per_iter) {
    const int ncol = min(8, L - 8 * g);
    uint32_t mn[8], mx[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      mn[c] = 255;
      mx[c] = 0;
    }
    const uint8_t* p = pc.src + 8 * g;
    const int64_t step = (int64_t)gridDim.x * rows_per_iter;
#pragma unroll 4
    for (int64_t r = (int64_t)blockIdx.x * rows_per_iter + rl; r < pc.nrec; r += step) {
      const uint64_t x = load_cols(p + r * L, ncol);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint32_t v = (uint32_t)(x >> (8 * c)) & 0xFF;
        mn[c] = min(mn[c], v);
        mx[c] = max(mx[c], v);
      }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (c < ncol) {
        atomicMin(&s_mn[8 * g + c], mn[c]);
        atomicMax(&s_mx[8 * g + c], mx[c]);
      }
  }
  __syncthreads();
  if (t < L) {
    uint32_t* tb = table + (size_t)blockIdx.y * kCpTableStride;
    atomicMin(&tb[t], s_mn[t]);
    atomicMin(&tb[kColpackMaxRecordBytes + t], 255u - s_mx[t]);
  }
}

__global__ void __launch_bounds__(64) colpack_plan_kernel(const ColpackPieceDesc* pieces, int L, uint32_t buf_records,
                                                          const uint32_t* table, ColpackResult* results) {
  const ColpackPieceDesc pc = pieces[blockIdx.x];
  const uint32_t* tb = table + (size_t)blockIdx.x * kCpTableStride;
  const int G = (L + 7) / 8;
  const int t = threadIdx.x;
  ColpackHeader* h = reinterpret_cast<ColpackHeader*>(pc.dst);
  __shared__ uint32_t s_gb[kColpackMaxGroups];
  if (t < kColpackMaxGroups) {
    uint64_t mask = 0, base = 0;
    int bits = 0;
    if (t < G)
      for (int c = 0; c < 8 && 8 * t + c < L; ++c) {
        const uint32_t mn = tb[8 * t + c], mx = 255u - tb[kColpackMaxRecordBytes + 8 * t + c];
        const uint32_t range = mx > mn ? mx - mn : 0;
        const int w = range ? 32 - __clz((int)range) : 0;
        bits += w;
        mask |= (uint64_t)((1u << w) - 1) << (8 * c);
        base |= (uint64_t)(mn & 0xFF) << (8 * c);
      }
    h->mask[t] = mask;
    h->base[t] = base;
    h->gb[t] = (uint8_t)((bits + 7) / 8);
    h->pad[t] = 0;
    s_gb[t] = (uint32_t)((bits + 7) / 8);
  }
  __syncthreads();
  int64_t S = 0;
  for (int g = 0; g < G; ++g) S += s_gb[g];
  const bool raw = colpack_is_raw(S, L);
  const int64_t total = raw ? (int64_t)kColpackHeaderBytes : colpack_packed_bytes(S, pc.nrec);
  if (t == 0) {
    h->magic = kColpackMagic;
    h->version = kColpackVersion;
    h->record_bytes = (uint32_t)L;
    h->flags = raw ? 0 : kColpackFlagPacked;
    h->records = (uint64_t)pc.nrec;
    h->buf_records = buf_records;
    h->stride = (uint32_t)S;
    h->groups = (uint32_t)G;
    for (int k = 0; k < 7; ++k) h->reserved[k] = 0;
    ColpackResult r;
    r.bytes = total;
    r.packed = raw ? 0 : 1;
    r.stride = (uint32_t)S;
    results[blockIdx.x] = r;
  }
  if (!raw)
    for (int64_t i = (int64_t)kColpackHeaderBytes + S * pc.nrec + t; i < total; i += 64) pc.dst[i] = 0;
}

// kG: groups per record known at compile time (13: TeraSort records), 0: from L.
template <int kG>
__global__ void __launch_bounds__(kCpThreads) colpack_pack_kernel(const ColpackPieceDesc* pieces, int L) {
  const ColpackPieceDesc pc = pieces[blockIdx.y];
  const ColpackHeader* h = reinterpret_cast<const ColpackHeader*>(pc.dst);
  if (!(h->flags & kColpackFlagPacked)) return;
  const int S = (int)h->stride;
  if (S == 0) return;
  const int64_t ntiles = (pc.nrec + kCpTileRows - 1) / kCpTileRows;
  if ((int64_t)blockIdx.x >= ntiles) return;
  const int G = kG ? kG : (L + 7) / 8;
  const int t = threadIdx.x;
  __shared__ uint64_t s_base[kColpackMaxGroups];
  __shared__ uint64_t s_shift[kColpackMaxGroups];  // byte c: bit offset of column c in the group's word
  __shared__ int s_gb[kColpackMaxGroups], s_off[kColpackMaxGroups];
  __shared__ __attribute__((aligned(16))) uint8_t s_tile[kCpTileBytes];
  if (t < G) {
    const uint64_t mask = h->mask[t];
    uint64_t sh = 0;
    int bits = 0;
    for (int c = 0; c < 8; ++c) {
      sh |= (uint64_t)bits << (8 * c);
      bits += __popc((uint32_t)(mask >> (8 * c)) & 0xFF);
    }
    s_shift[t] = sh;
    s_base[t] = h->base[t];
    s_gb[t] = h->gb[t];
  }
  __syncthreads();
  if (t == 0) {
    int off = 0;
    for (int g = 0; g < G; ++g) {
      s_off[g] = off;
      off += s_gb[g];
    }
  }
  __syncthreads();
  uint8_t* rows = pc.dst + kColpackHeaderBytes;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * kCpTileRows;
    const int nrows = (int)min((int64_t)kCpTileRows, pc.nrec - r0);
    const uint8_t* src = pc.src + r0 * L;
    for (int i = t; i < nrows * G; i += kCpThreads) {
      const int r = i / G, g = i - r * G;
      const int gb = s_gb[g];
      if (gb == 0) continue;
      const int ncol = min(8, L - 8 * g);
      // bytewise value - min: no byte borrows (value >= min in every column)
      const uint64_t x = load_cols(src + (int64_t)r * L + 8 * g, ncol) - s_base[g];
      const uint64_t sh = s_shift[g];
      uint64_t word = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) word |= ((x >> (8 * c)) & 0xFF) << ((uint32_t)(sh >> (8 * c)) & 0xFF);
      uint8_t* o = s_tile + r * S + s_off[g];
      for (int k = 0; k < gb; ++k) o[k] = (uint8_t)(word >> (8 * k));
    }
    __syncthreads();
    // tile start r0 * S is a multiple of 16 (kCpTileRows is) past the 64-byte aligned rows
    const int nbytes = nrows * S;
    uint8_t* out = rows + r0 * S;
    const int n16 = nbytes >> 4;
    for (int i = t; i < n16; i += kCpThreads)
      reinterpret_cast<uint4*>(out)[i] = reinterpret_cast<const uint4*>(s_tile)[i];
    for (int i = (n16 << 4) + t; i < nbytes; i += kCpThreads) out[i] = s_tile[i];
    __syncthreads();
  }
}
}  // namespace

size_t colpack_table_bytes(int npieces) { return (size_t)npieces * kCpTableStride * sizeof(uint32_t); }

void launch_colpack(const ColpackPieceDesc* pieces, int npieces, int64_t max_nrec, int L, int64_t buf_records,
                    uint32_t* table, ColpackResult* results, hipStream_t s) {
  if (npieces <= 0) return;
  (void)hipMemsetAsync(table, 0xFF, colpack_table_bytes(npieces), s);
  const int G = (L + 7) / 8;
  const int rows_per_iter = kCpThreads / G;
  // ~32 rows per thread before the grid stride; pieces of one launch share the grid's x extent
  int64_t sb = (max_nrec + (int64_t)rows_per_iter * 32 - 1) / ((int64_t)rows_per_iter * 32);
  sb = std::max<int64_t>(1, std::min<int64_t>(sb, 256));
  hipLaunchKernelGGL(colpack_stats_kernel, dim3((unsigned)sb, (unsigned)npieces), dim3(kCpThreads), 0, s, pieces, L,
                     table);
  hipLaunchKernelGGL(colpack_plan_kernel, dim3((unsigned)npieces), dim3(64), 0, s, pieces, L, (uint32_t)buf_records,
                     table, results);
  int64_t pb = (max_nrec + kCpTileRows - 1) / kCpTileRows;
  pb = std::max<int64_t>(1, std::min<int64_t>(pb, 1024));
  if (G == 13)
    hipLaunchKernelGGL(colpack_pack_kernel<13>, dim3((unsigned)pb, (unsigned)npieces), dim3(kCpThreads), 0, s, pieces, L);
  else
    hipLaunchKernelGGL(colpack_pack_kernel<0>, dim3((unsigned)pb, (unsigned)npieces), dim3(kCpThreads), 0, s, pieces, L);
}

}  // namespace gpu
}  // namespace uda
