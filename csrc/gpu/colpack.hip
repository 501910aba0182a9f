// colpack on the device: column-range bit-packing of a round's merged output ahead of its D2H
// (format and host reference: codec/colpack.h). Three launches per round over a fixed list of pieces:
//   colpack_stats_kernel  per piece, per column min / max (LDS reduction, one atomic pair per column
//                         per workgroup into the piece's table); with a key field also min / max of the
//                         key columns' difference bytes (T(r) of codec/colpack.h)
//   colpack_plan_kernel   per piece: plain or delta, widths -> masks, bases, row layout, stride,
//                         packed-or-raw, length; writes the piece header, the restart table of a delta
//                         piece and the zero padding after the rows
//   colpack_pack_kernel   tiles of records packed into LDS (shift + or, no hardware pext) and written
//                         out with coalesced vector stores; raw pieces are skipped
// A work item is one (record, 8-column group): consecutive lanes read consecutive 8-byte words of the
// record stream when L % 8 == 0 (104-byte TeraSort records: 13 groups). An item whose group overlaps
// the key field also loads the key of the record before it. Both format versions run through the same
// kernels: version 1 is byte-aligned groups and no key.
#include "codec/colpack.h"
#include "kernels.h"

#include <algorithm>

namespace uda {
namespace gpu {

namespace {
constexpr int kCpThreads = 256;
constexpr int kCpTileRows = 128;                      // rows per pack tile: tile starts stay 16-byte aligned
constexpr int kCpTileBytes = kCpTileRows * (9 * kColpackMaxRecordBytes / 10);  // LDS bytes of a packed tile
// per piece: min[256] | min of (255 - v)[256] | the same two of the key's difference bytes [16] [16]
constexpr int kCpTableDelta = 2 * kColpackMaxRecordBytes;
constexpr int kCpTableStride = kCpTableDelta + 2 * kColpackMaxKeyBytes;

// The n (<= 8) column bytes at p as a little-endian word.
__device__ __forceinline__ uint64_t load_cols(const uint8_t* p, int n) {
  if (n == 8 && (reinterpret_cast<uintptr_t>(p) & 7) == 0) return *reinterpret_cast<const uint64_t*>(p);
  uint64_t x = 0;
  for (int k = 0; k < n; ++k) x |= (uint64_t)p[k] << (8 * k);
  return x;
}

// A key field (<= 16 bytes) as a big-endian integer.
struct Key128 {
  uint64_t hi, lo;
};

__device__ __forceinline__ Key128 load_key(const uint8_t* rec, int L, int ko, int kl) {
  Key128 k{0, 0};
  const int g1 = (ko + kl - 1) >> 3;
  for (int g = ko >> 3; g <= g1; ++g) {
    const uint64_t x = load_cols(rec + 8 * g, min(8, L - 8 * g));
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int col = 8 * g + c;
      if (col >= ko && col < ko + kl) {
        k.hi = (k.hi << 8) | (k.lo >> 56);
        k.lo = (k.lo << 8) | ((x >> (8 * c)) & 0xFF);
      }
    }
  }
  return k;
}

__device__ __forceinline__ bool is_restart(int64_t row, uint32_t buf_records) {
  return (row >> 32) == 0 ? (uint32_t)row % buf_records == 0 : row % (int64_t)buf_records == 0;
}

// T(row): 0 on a restart row, else key(row) - key(row - 1); only its low kl bytes are ever used.
__device__ __forceinline__ Key128 key_delta(const uint8_t* rec, int64_t row, int L, uint32_t buf_records, int ko, int kl) {
  if (is_restart(row, buf_records)) return Key128{0, 0};
  const Key128 a = load_key(rec, L, ko, kl), b = load_key(rec - L, L, ko, kl);
  return Key128{a.hi - b.hi - (a.lo < b.lo ? 1 : 0), a.lo - b.lo};
}

// Group g's word x with its key columns replaced by T's bytes (column ko is the most significant).
__device__ __forceinline__ uint64_t with_key_delta(uint64_t x, int g, Key128 t, int ko, int kl) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int col = 8 * g + c;
    if (col >= ko && col < ko + kl) {
      const int j = ko + kl - 1 - col;  // byte of T, 0: least significant
      const uint64_t b = (j < 8 ? t.lo >> (8 * j) : t.hi >> (8 * (j - 8))) & 0xFF;
      x = (x & ~(0xFFull << (8 * c))) | (b << (8 * c));
    }
  }
  return x;
}

__device__ __forceinline__ bool group_has_key(int g, int ko, int kl) { return kl > 0 && 8 * g < ko + kl && 8 * g + 8 > ko; }

__global__ void __launch_bounds__(kCpThreads) colpack_stats_kernel(const ColpackPieceDesc* pieces, int L,
                                                                   uint32_t buf_records, int ko, int kl,
                                                                   uint32_t* table) {
  const ColpackPieceDesc pc = pieces[blockIdx.y];
  const int G = (L + 7) / 8;
  const int rows_per_iter = kCpThreads / G;  // threads past rows_per_iter * G idle: a thread keeps its group
  if ((int64_t)blockIdx.x * rows_per_iter >= pc.nrec) return;
  __shared__ uint32_t s_mn[kColpackMaxRecordBytes], s_mx[kColpackMaxRecordBytes];
  __shared__ uint32_t s_dmn[kColpackMaxKeyBytes], s_dmx[kColpackMaxKeyBytes];
  const int t = threadIdx.x;
  s_mn[t] = 255;
  s_mx[t] = 0;
  if (t < kColpackMaxKeyBytes) {
    s_dmn[t] = 255;
    s_dmx[t] = 0;
  }
  __syncthreads();
  const int g = t % G, rl = t / G;
  if (rl < rows_per_iter) {
    const int ncol = min(8, L - 8 * g);
    const bool keyed = group_has_key(g, ko, kl);
    uint32_t mn[8], mx[8], dmn[8], dmx[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      mn[c] = dmn[c] = 255;
      mx[c] = dmx[c] = 0;
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
      if (keyed) {
        const uint64_t xd = with_key_delta(x, g, key_delta(pc.src + r * L, r, L, buf_records, ko, kl), ko, kl);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const uint32_t v = (uint32_t)(xd >> (8 * c)) & 0xFF;
          dmn[c] = min(dmn[c], v);
          dmx[c] = max(dmx[c], v);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (c < ncol) {
        atomicMin(&s_mn[8 * g + c], mn[c]);
        atomicMax(&s_mx[8 * g + c], mx[c]);
        const int kc = 8 * g + c - ko;
        if (keyed && kc >= 0 && kc < kl) {
          atomicMin(&s_dmn[kc], dmn[c]);
          atomicMax(&s_dmx[kc], dmx[c]);
        }
      }
  }
  __syncthreads();
  uint32_t* tb = table + (size_t)blockIdx.y * kCpTableStride;
  if (t < L) {
    atomicMin(&tb[t], s_mn[t]);
    atomicMin(&tb[kColpackMaxRecordBytes + t], 255u - s_mx[t]);
  }
  if (t < kl) {
    atomicMin(&tb[kCpTableDelta + t], s_dmn[t]);
    atomicMin(&tb[kCpTableDelta + kColpackMaxKeyBytes + t], 255u - s_dmx[t]);
  }
}

__device__ __forceinline__ int width_of(uint32_t mn, uint32_t mx) {
  const uint32_t range = mx > mn ? mx - mn : 0;
  return range ? 32 - __clz((int)range) : 0;
}

__global__ void __launch_bounds__(64) colpack_plan_kernel(const ColpackPieceDesc* pieces, int L, uint32_t buf_records,
                                                          uint32_t version, int ko, int kl, const uint32_t* table,
                                                          ColpackResult* results) {
  const ColpackPieceDesc pc = pieces[blockIdx.x];
  const uint32_t* tb = table + (size_t)blockIdx.x * kCpTableStride;
  const int G = (L + 7) / 8;
  const int t = threadIdx.x;
  const bool v1 = version == kColpackVersion;
  ColpackHeader* h = reinterpret_cast<ColpackHeader*>(pc.dst);
  __shared__ int s_bits[kColpackMaxGroups];
  __shared__ uint16_t s_bo[kColpackMaxGroups];
  __shared__ int s_stride;
  // plain or delta: every thread takes the same decision from the same table
  int64_t plain_bits = 0, delta_bits = 0;
  for (int c = 0; c < kl; ++c) {
    plain_bits += width_of(tb[ko + c], 255u - tb[kColpackMaxRecordBytes + ko + c]);
    delta_bits += width_of(tb[kCpTableDelta + c], 255u - tb[kCpTableDelta + kColpackMaxKeyBytes + c]);
  }
  const bool delta = colpack2_choose_delta(plain_bits, delta_bits, pc.nrec, buf_records, kl);
  if (t < kColpackMaxGroups) {
    uint64_t mask = 0, base = 0;
    int bits = 0;
    if (t < G)
      for (int c = 0; c < 8 && 8 * t + c < L; ++c) {
        const int col = 8 * t + c, kc = col - ko;
        uint32_t mn = tb[col], mx = 255u - tb[kColpackMaxRecordBytes + col];
        if (delta && kc >= 0 && kc < kl) {
          mn = tb[kCpTableDelta + kc];
          mx = 255u - tb[kCpTableDelta + kColpackMaxKeyBytes + kc];
        }
        const int w = width_of(mn, mx);
        bits += w;
        mask |= (uint64_t)((1u << w) - 1) << (8 * c);
        base |= (uint64_t)(mn & 0xFF) << (8 * c);
      }
    h->mask[t] = mask;
    h->base[t] = base;
    s_bits[t] = bits;
  }
  __syncthreads();
  if (t == 0) s_stride = colpack_layout(s_bits, G, v1, s_bo);
  __syncthreads();
  if (t < kColpackMaxGroups) {
    if (v1) {
      h->gb[t] = (uint8_t)((s_bits[t] + 7) / 8);
      h->pad[t] = 0;
    } else {
      h->bo[t] = t < G ? s_bo[t] : (uint16_t)0;
    }
  }
  const int64_t S = s_stride;
  const bool raw = colpack_is_raw(S, L);
  const int64_t table_bytes = delta ? colpack2_table_bytes(pc.nrec, buf_records) : 0;
  const int64_t total = raw  ? (int64_t)kColpackHeaderBytes
                        : v1 ? colpack_packed_bytes(S, pc.nrec)
                             : colpack2_packed_bytes(S, pc.nrec, table_bytes);
  if (t == 0) {
    h->magic = kColpackMagic;
    h->version = version;
    h->record_bytes = (uint32_t)L;
    h->flags = (raw ? 0 : kColpackFlagPacked) | (delta ? kColpackFlagDelta : 0);
    h->records = (uint64_t)pc.nrec;
    h->buf_records = buf_records;
    h->stride = (uint32_t)S;
    h->groups = (uint32_t)G;
    h->key_off = (uint32_t)ko;
    h->key_len = (uint32_t)kl;
    for (int k = 0; k < 5; ++k) h->reserved[k] = 0;
    ColpackResult r;
    r.bytes = total;
    r.packed = raw ? 0 : 1;
    r.stride = (uint32_t)S;
    r.delta = delta ? 1 : 0;
    r.reserved = 0;
    results[blockIdx.x] = r;
  }
  if (raw) return;
  if (delta) {  // restart table: the key of every buffer's first row, zero-filled to 16 bytes, then to 64
    uint8_t* tab = pc.dst + kColpackHeaderBytes;
    const int64_t entries = (pc.nrec + buf_records - 1) / buf_records;
    for (int64_t b = t; b < entries; b += 64) {
      const uint8_t* key = pc.src + b * buf_records * L + ko;
      for (int k = 0; k < kColpackRestartBytes; ++k) tab[b * kColpackRestartBytes + k] = k < kl ? key[k] : (uint8_t)0;
    }
    for (int64_t i = entries * kColpackRestartBytes + t; i < table_bytes; i += 64) tab[i] = 0;
  }
  for (int64_t i = (int64_t)kColpackHeaderBytes + table_bytes + S * pc.nrec + t; i < total; i += 64) pc.dst[i] = 0;
}

// kG: groups per record known at compile time (13: TeraSort records), 0: from L.
// Group words share bytes in version 2, so a tile is zeroed in LDS and every item ORs its shifted
// word into the tile's 32-bit words (at most three) with LDS atomics.
template <int kG>
__global__ void __launch_bounds__(kCpThreads) colpack_pack_kernel(const ColpackPieceDesc* pieces, int L) {
  const ColpackPieceDesc pc = pieces[blockIdx.y];
  const ColpackHeader* h = reinterpret_cast<const ColpackHeader*>(pc.dst);
  const uint32_t flags = h->flags;
  if (!(flags & kColpackFlagPacked)) return;
  const int S = (int)h->stride;
  if (S == 0) return;
  const int64_t ntiles = (pc.nrec + kCpTileRows - 1) / kCpTileRows;
  if ((int64_t)blockIdx.x >= ntiles) return;
  const int G = kG ? kG : (L + 7) / 8;
  const int t = threadIdx.x;
  const bool delta = (flags & kColpackFlagDelta) != 0;
  const uint32_t buf_records = h->buf_records;
  const int ko = (int)h->key_off, kl = delta ? (int)h->key_len : 0;
  __shared__ uint64_t s_base[kColpackMaxGroups];
  __shared__ uint64_t s_shift[kColpackMaxGroups];  // byte c: bit offset of column c in the group's word
  __shared__ int s_bits[kColpackMaxGroups];
  __shared__ uint16_t s_bo[kColpackMaxGroups];
  __shared__ __attribute__((aligned(16))) uint32_t s_tile[kCpTileBytes / 4 + 4];
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
    s_bits[t] = bits;
  }
  __syncthreads();
  if (t == 0) colpack_layout(s_bits, G, h->version == kColpackVersion, s_bo);
  __syncthreads();
  uint8_t* rows = pc.dst + kColpackHeaderBytes + (delta ? colpack2_table_bytes(pc.nrec, buf_records) : 0);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * kCpTileRows;
    const int nrows = (int)min((int64_t)kCpTileRows, pc.nrec - r0);
    const int nbytes = nrows * S;
    for (int i = t; i < (nbytes + 15) >> 4; i += kCpThreads) reinterpret_cast<uint4*>(s_tile)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const uint8_t* src = pc.src + r0 * L;
    for (int i = t; i < nrows * G; i += kCpThreads) {
      const int r = i / G, g = i - r * G;
      if (s_bits[g] == 0) continue;
      const int ncol = min(8, L - 8 * g);
      const uint8_t* rec = src + (int64_t)r * L;
      uint64_t x = load_cols(rec + 8 * g, ncol);
      if (group_has_key(g, ko, kl)) x = with_key_delta(x, g, key_delta(rec, r0 + r, L, buf_records, ko, kl), ko, kl);
      // bytewise value - min: no byte borrows (value >= min in every column)
      x -= s_base[g];
      const uint64_t sh = s_shift[g];
      uint64_t word = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) word |= ((x >> (8 * c)) & 0xFF) << ((uint32_t)(sh >> (8 * c)) & 0xFF);
      // the word's set bits lie inside the row: a 32-bit part past the tile is zero and is skipped
      const int bit = r * S * 8 + s_bo[g];
      const int wi = bit >> 5, ws = bit & 31;
      const uint64_t lo = word << ws;
      const uint32_t w0 = (uint32_t)lo, w1 = (uint32_t)(lo >> 32), w2 = ws ? (uint32_t)(word >> (64 - ws)) : 0u;
      if (w0) atomicOr(&s_tile[wi], w0);
      if (w1) atomicOr(&s_tile[wi + 1], w1);
      if (w2) atomicOr(&s_tile[wi + 2], w2);
    }
    __syncthreads();
    // tile start r0 * S is a multiple of 16 (kCpTileRows is) past the 64-byte aligned rows
    uint8_t* out = rows + r0 * S;
    const int n16 = nbytes >> 4;
    for (int i = t; i < n16; i += kCpThreads)
      reinterpret_cast<uint4*>(out)[i] = reinterpret_cast<const uint4*>(s_tile)[i];
    for (int i = (n16 << 4) + t; i < nbytes; i += kCpThreads) out[i] = reinterpret_cast<const uint8_t*>(s_tile)[i];
    __syncthreads();
  }
}
}  // namespace

size_t colpack_table_bytes(int npieces) { return (size_t)npieces * kCpTableStride * sizeof(uint32_t); }

void launch_colpack(const ColpackPieceDesc* pieces, int npieces, int64_t max_nrec, int L, int64_t buf_records,
                    uint32_t* table, ColpackResult* results, hipStream_t s, int version, int key_off, int key_len) {
  if (npieces <= 0) return;
  if (version != (int)kColpackVersion2) version = (int)kColpackVersion, key_len = 0;
  if (key_len <= 0 || key_len > kColpackMaxKeyBytes || key_off < 0 || key_off + key_len > L || buf_records < 1 ||
      buf_records > 0xFFFFFFFFll)
    key_len = 0;  // no key: nothing is read outside a record
  if (key_len == 0) key_off = 0;
  (void)hipMemsetAsync(table, 0xFF, colpack_table_bytes(npieces), s);
  const int G = (L + 7) / 8;
  const int rows_per_iter = kCpThreads / G;
  // ~32 rows per thread before the grid stride; pieces of one launch share the grid's x extent
  int64_t sb = (max_nrec + (int64_t)rows_per_iter * 32 - 1) / ((int64_t)rows_per_iter * 32);
  sb = std::max<int64_t>(1, std::min<int64_t>(sb, 256));
  hipLaunchKernelGGL(colpack_stats_kernel, dim3((unsigned)sb, (unsigned)npieces), dim3(kCpThreads), 0, s, pieces, L,
                     (uint32_t)buf_records, key_off, key_len, table);
  hipLaunchKernelGGL(colpack_plan_kernel, dim3((unsigned)npieces), dim3(64), 0, s, pieces, L, (uint32_t)buf_records,
                     (uint32_t)version, key_off, key_len, table, results);
  int64_t pb = (max_nrec + kCpTileRows - 1) / kCpTileRows;
  pb = std::max<int64_t>(1, std::min<int64_t>(pb, 1024));
  if (G == 13)
    hipLaunchKernelGGL(colpack_pack_kernel<13>, dim3((unsigned)pb, (unsigned)npieces), dim3(kCpThreads), 0, s, pieces, L);
  else
    hipLaunchKernelGGL(colpack_pack_kernel<0>, dim3((unsigned)pb, (unsigned)npieces), dim3(kCpThreads), 0, s, pieces, L);
}

}  // namespace gpu
}  // namespace uda
