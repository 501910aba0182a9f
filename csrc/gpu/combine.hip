// Reduce-side combiner on the merged order (uda/combine.h: sums, min / max, VInt / VLong sums): equal keys
// are adjacent after F3, so what remains is a head flag per merged element, a segmented fold of the values
// and a compaction in F4. Everything reads the side tables F2 left behind (keyptr / keylen / recptr /
// reclen); record headers are never parsed again.
//
//   combine_heads_kernel    head[i] = first record of its group, and the value check of the op
//   (exclusive scan of head: gidx[i] = groups begun before i, so group(i) = gidx[i + 1] - 1)
//   combine_sums_kernel     sums[group] = fold of the group's values; fixed-width ops: sizes[i] = head ? reclen : 0
//   combine_vsizes_kernel   v ops only: sizes[i] = head ? reclen - value bytes + vint_size(sum) : 0
//   (exclusive scan of sizes: output offsets; a non-head shares the offset of the next head)
//   gather_combine_kernel   copies the head records with the folded value in place of theirs
//
// Streamed key-range rounds (a merge of more than round_bytes) run the same on the subrange a round
// delivers; two more kernels serve them:
//   combine_check_values_kernel  any value the op cannot read, over all records, before F3
//   combine_round_heads_kernel   head flags of the elements a round added, and the round close: the
//                                highest head position, where the still open last group begins
//
// Folds are on unsigned 64-bit integers. Sums (the low 32 bits serve sum.int and sum.vint): wrapping adds
// are associative, so the result is the same bits in any reduction order, atomics included. Min / max: the
// signed value is mapped to an unsigned one of the same order (v ^ sign bit for max, the complement of that
// for min), so both folds are one unsigned max whose identity is 0. That keeps the zero memset of sums[]
// and one atomic per tile-straddling segment, as the sums have them, where a signed min would need a fill
// kernel for its identity; the gather maps the result back with one xor.
#include "generic_cmp.h"
#include "kernels.h"
#include "uda/combine.h"
#include "uda/vint.h"

namespace uda {
namespace gpu {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 __attribute__((aligned(1))) u32x4_u;  // unaligned 16-byte access (legal for global memory)

static_assert(kCombineTile == 256, "combine_sums_kernel: one element per lane, four waves per tile");

constexpr unsigned long long kSignBit = 1ull << 63;

constexpr bool op_is_max(CombineOp op) { return op == CombineOp::kMaxInt || op == CombineOp::kMaxLong; }
constexpr bool op_is_min(CombineOp op) { return op == CombineOp::kMinInt || op == CombineOp::kMinLong; }
// stored fold value = signed value ^ op_bias(op), and back (0 for the sums)
constexpr unsigned long long op_bias(CombineOp op) { return op_is_max(op) ? kSignBit : op_is_min(op) ? ~kSignBit : 0; }

// Equal under key_compare: the same content bytes and the same content length. Elem.hi holds content
// bytes 0..7 zero padded, so the length has to match too ("a" and "a\0" share hi); the 16-bit length
// field clamps at 0xFFFF, so contents longer than 8 bytes compare their real lengths in keylen.
__device__ __forceinline__ bool same_key(const GenericKeyCtx& ctx, const Elem& a, const Elem& b) {
  if (a.hi != b.hi || (a.lo >> 48) != (b.lo >> 48)) return false;
  if ((a.lo >> 48) <= 8) return true;
  const uint64_t ga = a.lo & kGenOrdMask, gb = b.lo & kGenOrdMask;
  const int la = ctx.keylen[ga];
  if (la != ctx.keylen[gb]) return false;
  const uint8_t* pa = ctx.keyptr[ga];
  const uint8_t* pb = ctx.keyptr[gb];
  for (int i = 8; i < la; i += 8)
    if (load_be8(pa + i, la - i) != load_be8(pb + i, la - i)) return false;
  return true;
}

// Value bytes of record g from the side tables: record size less the headers, the key's class prefix
// (both lie between recptr and keyptr) and the key content.
// Numeric kinds: keyptr points at the normalized key, outside the record, so the value length is read from
// the record's second header (ctx.normkey is a kernel argument: the branch is uniform).
__device__ __forceinline__ int64_t value_bytes(const GenericKeyCtx& ctx, uint64_t g) {
  if (ctx.normkey) {
    const uint8_t* rec = ctx.recptr[g];
    int64_t vl = 0;
    vint_decode(rec + vint_decode_size((int8_t)rec[0]), 9, &vl);
    return vl;
  }
  return (int64_t)ctx.reclen[g] - (int64_t)(ctx.keyptr[g] - ctx.recptr[g]) - (int64_t)ctx.keylen[g];
}

// combine_value_ok (uda/combine.h) from the side tables: W value bytes, or for the v ops one VLong that
// fills the value exactly (then at most 9 bytes, all inside the record), in int32 range under sum.vint.
__device__ __forceinline__ bool value_ok(const GenericKeyCtx& ctx, uint64_t g, CombineOp op) {
  const int64_t vb = value_bytes(ctx, g);
  if (!combine_variable_width(op)) return vb == combine_value_bytes(op);
  if (vb < 1) return false;
  const uint8_t* p = ctx.recptr[g] + ctx.reclen[g] - vb;
  if (vb != vint_decode_size((int8_t)p[0])) return false;
  if (op == CombineOp::kSumVLong) return true;
  int64_t v = 0;
  vint_decode(p, (size_t)vb, &v);
  return v >= INT32_MIN && v <= INT32_MAX;
}

__global__ void __launch_bounds__(256) combine_heads_kernel(GenericKeyCtx ctx, const Elem* order, int64_t n,
                                                            CombineOp op, int64_t* heads, unsigned long long* bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Elem e = order[i];
  heads[i] = (i == 0 || !same_key(ctx, order[i - 1], e)) ? 1 : 0;
  // error path only: the lowest merged position with a value the op cannot read
  if (!value_ok(ctx, e.lo & kGenOrdMask, op)) atomicMin(bad, (unsigned long long)i);
}

// Streamed rounds (generic_merger.cc): the value check over every record of the side tables, in record
// order. It runs before F3 and says only whether any value is one the op cannot read; the whole path then
// finds the lowest merged position for the error.
__global__ void __launch_bounds__(256) combine_check_values_kernel(GenericKeyCtx ctx, int64_t n, CombineOp op,
                                                                   int* any_bad) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool bad = g < n && !value_ok(ctx, (uint64_t)g, op);
  if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(any_bad, 1);
}

// Streamed rounds: the head flags of the merged elements [i0, i1) a round added (element i0 compares with
// i0 - 1, which an earlier round merged), and the round close: *last_head = 1 + the highest head position
// in the range (0 stays for none), a max over each wave, then over the workgroup's waves in LDS, then one
// atomicMax per workgroup that saw a head.
__global__ void __launch_bounds__(256) combine_round_heads_kernel(GenericKeyCtx ctx, const Elem* order, int64_t i0,
                                                                  int64_t i1, int64_t* heads,
                                                                  unsigned long long* last_head) {
  __shared__ unsigned long long wmax[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t i = i0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long m = 0;
  if (i < i1) {
    const bool h = i == 0 || !same_key(ctx, order[i - 1], order[i]);
    heads[i] = h ? 1 : 0;
    if (h) m = (unsigned long long)i + 1;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = max(m, (unsigned long long)__shfl_xor(m, off, 64));
  if (lane == 0) wmax[wid] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
    if (m != 0) atomicMax(last_head, m);
  }
}

// The fold of two partial results of OP (see the head of the file): a wrapping add, or an unsigned max of
// the order-preserving images. 0 is the identity of both.
template <CombineOp OP>
__device__ __forceinline__ unsigned long long fold(unsigned long long a, unsigned long long b) {
  if (op_is_max(OP) || op_is_min(OP)) return a > b ? a : b;
  return a + b;
}

// The value of record g (L bytes long) as OP folds it; a value the op cannot read counts as the identity.
template <CombineOp OP>
__device__ __forceinline__ unsigned long long load_value(const GenericKeyCtx& ctx, uint64_t g, int L) {
  if (!value_ok(ctx, g, OP)) return 0;  // flagged by combine_heads_kernel, nothing is delivered
  if (combine_variable_width(OP)) {
    const int vb = (int)value_bytes(ctx, g);
    int64_t v = 0;
    vint_decode(ctx.recptr[g] + L - vb, (size_t)vb, &v);
    return (unsigned long long)v;
  }
  constexpr int W = combine_value_bytes(OP);
  const uint8_t* p = ctx.recptr[g] + L - W;
  if (W == 8) {
    uint64_t w;
    __builtin_memcpy(&w, p, 8);
    return __builtin_bswap64(w) ^ op_bias(OP);
  }
  uint32_t w;
  __builtin_memcpy(&w, p, 4);
  w = __builtin_bswap32(w);
  if (OP == CombineOp::kSumInt) return w;
  return (unsigned long long)(int64_t)(int32_t)w ^ op_bias(OP);  // min / max compare the signed value
}

// One merged element per lane, kCombineTile per workgroup. A wave's values are folded by a segmented
// inclusive scan under the wave's head mask, the waves' open ends are joined through LDS, and the last
// lane of every segment that ends in the workgroup writes it. A group that lies inside the tile is written
// with a plain store; the tile's leading segment (its head is in an earlier tile) and its trailing one
// (it goes on in the next tile) are folded into the zeroed sums[] with one atomic each (64-bit, device
// scope: the other tiles of the group are other workgroups).
template <CombineOp OP>
__global__ void __launch_bounds__(kCombineTile) combine_sums_kernel(GenericKeyCtx ctx, const Elem* order,
                                                                    const int64_t* gidx, int64_t n,
                                                                    unsigned long long* sums, int64_t* sizes) {
  constexpr int kWaves = kCombineTile / 64;
  __shared__ unsigned long long tail[kWaves];
  __shared__ int has_head[kWaves], first_head[kWaves];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * kCombineTile + threadIdx.x;
  const bool valid = i < n;
  bool h = true;  // lanes past the end close the last segment and write nothing
  int64_t group = 0;
  unsigned long long v = 0;
  if (valid) {
    const int64_t g0 = gidx[i], g1 = gidx[i + 1];
    h = g1 != g0;
    group = g1 - 1;
    const uint64_t g = order[i].lo & kGenOrdMask;
    const int L = ctx.reclen[g];
    // a v op's record size needs the group's final sum: combine_vsizes_kernel writes the sizes
    if (!combine_variable_width(OP)) sizes[i] = h ? L : 0;
    v = load_value<OP>(ctx, g, L);
  }
  const unsigned long long mask = __ballot(h);
  const unsigned long long below = mask & ((2ull << lane) - 1);  // heads at or before this lane
  const bool open = below == 0;                                  // the segment began in an earlier wave
  const int seg_lo = open ? 0 : 63 - __builtin_clzll(below);
  unsigned long long x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long y = __shfl_up(x, off, 64);
    if (lane - off >= seg_lo) x = fold<OP>(x, y);
  }
  if (lane == 63) tail[wid] = x;
  if (lane == 0) {
    has_head[wid] = mask != 0;
    first_head[wid] = (int)(mask & 1);
  }
  __syncthreads();
  if (!valid) return;
  const bool seg_end = lane == 63 || ((mask >> (lane + 1)) & 1);
  if (!seg_end) return;
  if (lane == 63 && wid + 1 < kWaves && !first_head[wid + 1]) return;  // goes on in the next wave
  bool head_in_tile = !open;
  if (open) {  // the earlier waves' open ends, back to the nearest head
    for (int w = wid - 1; w >= 0; --w) {
      x = fold<OP>(x, tail[w]);
      if (has_head[w]) {
        head_in_tile = true;
        break;
      }
    }
  }
  bool ends_in_tile = true;
  if (lane == 63 && wid + 1 == kWaves && i + 1 < n) ends_in_tile = gidx[i + 2] != gidx[i + 1];
  if (head_in_tile && ends_in_tile)
    sums[group] = x;
  else if (op_is_max(OP) || op_is_min(OP))
    atomicMax(&sums[group], x);
  else
    atomicAdd(&sums[group], x);
}

// The signed value a v op delivers for a group's sum: sum.vint wraps to 32 bits (Java's int add).
__device__ __forceinline__ int64_t vsum_value(CombineOp op, unsigned long long sum) {
  return op == CombineOp::kSumVInt ? (int64_t)(int32_t)(uint32_t)sum : (int64_t)sum;
}

// The v ops' F4 sizes, after combine_sums_kernel has finished every group (a segment that straddles tiles
// has its sum only then): a head's record with its value re-encoded, 0 for any other element. The
// value-length header stays one byte (lengths 1..9). A record whose value cannot be read keeps a size that
// is never used: nothing is delivered.
__global__ void __launch_bounds__(256) combine_vsizes_kernel(GenericKeyCtx ctx, const Elem* order, const int64_t* gidx,
                                                             int64_t n, CombineOp op, const unsigned long long* sums,
                                                             int64_t* sizes) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t g1 = gidx[i + 1];
  int64_t size = 0;
  if (g1 != gidx[i]) {
    const uint64_t g = order[i].lo & kGenOrdMask;
    size = (int64_t)ctx.reclen[g] - value_bytes(ctx, g) + vint_size(vsum_value(op, sums[g1 - 1]));
  }
  sizes[i] = size;
}

// Bytes [t, t + W) of the 8 bytes in w (as loaded: byte k in bits 8k..8k+7) replaced by the value's
// big-endian bytes `be` (in the same layout; bm covers its W bytes). t may lie outside the word.
__device__ __forceinline__ uint64_t patch8(uint64_t w, int t, uint64_t be, uint64_t bm) {
  if (t >= 8 || t <= -8) return w;
  const uint64_t v = t >= 0 ? be << (8 * t) : be >> (8 * -t);
  const uint64_t m = t >= 0 ? bm << (8 * t) : bm >> (8 * -t);
  return (w & ~m) | (v & m);
}

__device__ __forceinline__ u32x4 patch16(u32x4 v, int t, uint64_t be, uint64_t bm) {
  if (t >= 16) return v;
  const uint64_t lo = patch8((uint64_t)v[0] | ((uint64_t)v[1] << 32), t, be, bm);
  const uint64_t hi = patch8((uint64_t)v[2] | ((uint64_t)v[3] << 32), t - 8, be, bm);
  u32x4 r;
  r[0] = (uint32_t)lo;
  r[1] = (uint32_t)(lo >> 32);
  r[2] = (uint32_t)hi;
  r[3] = (uint32_t)(hi >> 32);
  return r;
}

// F4 under the fixed-width ops: gather_var_grp_kernel's copy (kGatherLanes lanes per record, 16-byte
// pieces, the last one shifted back to end at L) for the head records only. The folded value (sums[] ^
// unbias, see the head of the file) replaces the record's last W bytes in the registers of whichever
// pieces cover them, before the store: overlapping pieces then still store identical bytes, and no second
// store has to be ordered after the copy.
template <int kGatherLanes>
__global__ void __launch_bounds__(256) gather_combine_kernel(GenericKeyCtx ctx, const Elem* elems, int64_t n,
                                                             const int64_t* gidx, const int64_t* out_off,
                                                             const unsigned long long* sums,
                                                             unsigned long long unbias, int W, uint8_t* out) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGatherLanes;
  const int sub = (int)(threadIdx.x % kGatherLanes);
  if (i >= n) return;
  const int64_t g1 = gidx[i + 1];
  if (g1 == gidx[i]) return;  // not the head of its group
  const uint64_t g = elems[i].lo & kGenOrdMask;
  const uint8_t* src = ctx.recptr[g];
  const int L = ctx.reclen[g];
  uint8_t* dst = out + out_off[i];
  const unsigned long long sum = sums[g1 - 1] ^ unbias;
  const uint64_t be = W == 8 ? __builtin_bswap64(sum) : (uint64_t)__builtin_bswap32((uint32_t)sum);
  const uint64_t bm = W == 8 ? ~0ull : 0xFFFFFFFFull;
  const int vt = L - W;  // the value's offset in the record
  if (L < 16) {
    if (sub != 0) return;
    if (L >= 8) {
      uint64_t a, b;
      __builtin_memcpy(&a, src, 8);
      __builtin_memcpy(&b, src + L - 8, 8);
      a = patch8(a, vt, be, bm);
      b = patch8(b, 8 - W, be, bm);
      __builtin_memcpy(dst, &a, 8);
      __builtin_memcpy(dst + L - 8, &b, 8);
    } else {
      for (int k = 0; k < L; ++k) dst[k] = k >= vt ? (uint8_t)(be >> (8 * (k - vt))) : src[k];
    }
    return;
  }
  constexpr int kStep = kGatherLanes * 16;
  for (int base = sub * 16; base < L; base += 2 * kStep) {
    const int o0 = min(base, L - 16);
    const int o1 = min(base + kStep, L - 16);
    const u32x4 v0 = patch16(*reinterpret_cast<const u32x4_u*>(src + o0), vt - o0, be, bm);
    const u32x4 v1 = patch16(*reinterpret_cast<const u32x4_u*>(src + o1), vt - o1, be, bm);
    *reinterpret_cast<u32x4_u*>(dst + o0) = v0;
    if (base + kStep < L) *reinterpret_cast<u32x4_u*>(dst + o1) = v1;
  }
}

// A delivered record of the v ops, as a function of the output byte position: the head record's first P
// bytes (its headers and key; P = L - value bytes) with the one-byte value-length header at `hoff` set to
// nv, then the nv bytes of the canonical VLong (byte k of it in bits 8k.. of elo, byte 8 in e8).
struct VRecord {
  const uint8_t* src;
  int P, hoff, nv;
  uint64_t elo;
  uint32_t e8;

  __device__ __forceinline__ uint32_t byte(int pos) const {
    if (pos < P) return pos == hoff ? (uint32_t)nv : src[pos];
    const int j = pos - P;
    return j < 8 ? (uint32_t)(elo >> (8 * j)) & 0xFFu : e8;
  }
  // Output bytes [pos, pos + 8), byte k in bits 8k..; the caller keeps pos + 8 <= P + nv. Source bytes are
  // loaded only below P, which is inside the source record however long the output record is.
  __device__ __forceinline__ uint64_t word(int pos) const {
    uint64_t w = 0;
    if (pos + 8 <= P) {
      __builtin_memcpy(&w, src + pos, 8);
      const int t = hoff - pos;
      if (t >= 0 && t < 8) w = (w & ~(0xFFull << (8 * t))) | ((uint64_t)nv << (8 * t));
      return w;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) w |= (uint64_t)byte(pos + k) << (8 * k);
    return w;
  }
  __device__ __forceinline__ u32x4 piece(int pos) const {  // output bytes [pos, pos + 16)
    const uint64_t lo = word(pos), hi = word(pos + 8);
    u32x4 r;
    r[0] = (uint32_t)lo;
    r[1] = (uint32_t)(lo >> 32);
    r[2] = (uint32_t)hi;
    r[3] = (uint32_t)(hi >> 32);
    return r;
  }
};

// F4 under the v ops (sum.vint, sum.vlong): the same lanes and 16-byte pieces over the output record,
// which is P + nv bytes long: shorter or longer than the head record. Every piece is built whole in
// registers (VRecord) before it is stored, so overlapping pieces store identical bytes, and nothing is
// loaded at or past the head's value: the head can be the last record of its buffer.
template <int kGatherLanes>
__global__ void __launch_bounds__(256) gather_combine_var_kernel(GenericKeyCtx ctx, const Elem* elems, int64_t n,
                                                                 const int64_t* gidx, const int64_t* out_off,
                                                                 const unsigned long long* sums, CombineOp op,
                                                                 uint8_t* out) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGatherLanes;
  const int sub = (int)(threadIdx.x % kGatherLanes);
  if (i >= n) return;
  const int64_t g1 = gidx[i + 1];
  if (g1 == gidx[i]) return;  // not the head of its group
  const uint64_t g = elems[i].lo & kGenOrdMask;
  VRecord r;
  r.src = ctx.recptr[g];
  r.P = ctx.reclen[g] - (int)value_bytes(ctx, g);
  r.hoff = vint_decode_size((int8_t)r.src[0]);  // after the key-length VInt
  // vint_encode (uda/vint.h) in registers
  const int64_t v = vsum_value(op, sums[g1 - 1]);
  if (v >= -112 && v <= 127) {
    r.nv = 1;
    r.elo = (uint8_t)(int8_t)v;
    r.e8 = 0;
  } else {
    const uint64_t m = v < 0 ? ~(uint64_t)v : (uint64_t)v;  // != 0
    const int nb = (64 - __builtin_clzll(m) + 7) / 8;       // magnitude bytes, 1..8
    const uint64_t be = __builtin_bswap64(m) >> (8 * (8 - nb));  // most significant of the nb bytes first
    r.nv = nb + 1;
    r.elo = (uint64_t)(uint8_t)(int8_t)((v < 0 ? -120 : -112) - nb) | (be << 8);
    r.e8 = (uint32_t)(be >> 56);
  }
  const int Lo = r.P + r.nv;
  uint8_t* dst = out + out_off[i];
  if (Lo < 16) {
    if (sub != 0) return;
    if (Lo >= 8) {
      const uint64_t a = r.word(0), b = r.word(Lo - 8);
      __builtin_memcpy(dst, &a, 8);
      __builtin_memcpy(dst + Lo - 8, &b, 8);
    } else {
      for (int k = 0; k < Lo; ++k) dst[k] = (uint8_t)r.byte(k);
    }
    return;
  }
  constexpr int kStep = kGatherLanes * 16;
  for (int base = sub * 16; base < Lo; base += 2 * kStep) {
    const int o0 = min(base, Lo - 16);
    *reinterpret_cast<u32x4_u*>(dst + o0) = r.piece(o0);
    if (base + kStep < Lo) {
      const int o1 = min(base + kStep, Lo - 16);
      *reinterpret_cast<u32x4_u*>(dst + o1) = r.piece(o1);
    }
  }
}

template <CombineOp OP>
void launch_sums_of(GenericKeyCtx ctx, const Elem* order, const int64_t* gidx, int64_t n, unsigned long long* sums,
                    int64_t* sizes, hipStream_t s) {
  hipLaunchKernelGGL(combine_sums_kernel<OP>, dim3((unsigned)((n + kCombineTile - 1) / kCombineTile)),
                     dim3(kCombineTile), 0, s, ctx, order, gidx, n, sums, sizes);
}

}  // namespace

void launch_combine_heads(GenericKeyCtx ctx, const Elem* order, int64_t n, CombineOp op, int64_t* heads,
                          unsigned long long* bad, hipStream_t s) {
  (void)hipMemsetAsync(bad, 0xFF, sizeof(unsigned long long), s);
  if (n <= 0) return;
  hipLaunchKernelGGL(combine_heads_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ctx, order, n, op,
                     heads, bad);
}

void launch_combine_check_values(GenericKeyCtx ctx, int64_t n, CombineOp op, int* any_bad, hipStream_t s) {
  (void)hipMemsetAsync(any_bad, 0, sizeof(int), s);
  if (n <= 0) return;
  hipLaunchKernelGGL(combine_check_values_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ctx, n, op,
                     any_bad);
}

void launch_combine_round_heads(GenericKeyCtx ctx, const Elem* order, int64_t i0, int64_t i1, int64_t* heads,
                                unsigned long long* last_head, hipStream_t s) {
  if (i1 <= i0) return;
  hipLaunchKernelGGL(combine_round_heads_kernel, dim3((unsigned)((i1 - i0 + 255) / 256)), dim3(256), 0, s, ctx, order,
                     i0, i1, heads, last_head);
}

void launch_combine_sums(GenericKeyCtx ctx, const Elem* order, const int64_t* gidx, int64_t n, CombineOp op,
                         unsigned long long* sums, int64_t* sizes, hipStream_t s) {
  if (n <= 0) return;
  (void)hipMemsetAsync(sums, 0, (size_t)n * sizeof(unsigned long long), s);
  switch (op) {
    case CombineOp::kSumInt: launch_sums_of<CombineOp::kSumInt>(ctx, order, gidx, n, sums, sizes, s); break;
    case CombineOp::kSumLong: launch_sums_of<CombineOp::kSumLong>(ctx, order, gidx, n, sums, sizes, s); break;
    case CombineOp::kMinInt: launch_sums_of<CombineOp::kMinInt>(ctx, order, gidx, n, sums, sizes, s); break;
    case CombineOp::kMaxInt: launch_sums_of<CombineOp::kMaxInt>(ctx, order, gidx, n, sums, sizes, s); break;
    case CombineOp::kMinLong: launch_sums_of<CombineOp::kMinLong>(ctx, order, gidx, n, sums, sizes, s); break;
    case CombineOp::kMaxLong: launch_sums_of<CombineOp::kMaxLong>(ctx, order, gidx, n, sums, sizes, s); break;
    case CombineOp::kSumVInt: launch_sums_of<CombineOp::kSumVInt>(ctx, order, gidx, n, sums, sizes, s); break;
    case CombineOp::kSumVLong: launch_sums_of<CombineOp::kSumVLong>(ctx, order, gidx, n, sums, sizes, s); break;
    case CombineOp::kNone: break;
  }
  if (combine_variable_width(op))
    hipLaunchKernelGGL(combine_vsizes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ctx, order, gidx, n,
                       op, sums, sizes);
}

void launch_gather_combine(GenericKeyCtx ctx, const Elem* elems, int64_t n, const int64_t* gidx,
                           const int64_t* out_off, const unsigned long long* sums, CombineOp op, uint8_t* out,
                           hipStream_t s) {
  if (n <= 0) return;
  const dim3 grid((unsigned)((n * 8 + 255) / 256));
  if (combine_variable_width(op))
    hipLaunchKernelGGL(gather_combine_var_kernel<8>, grid, dim3(256), 0, s, ctx, elems, n, gidx, out_off, sums, op,
                       out);
  else
    hipLaunchKernelGGL(gather_combine_kernel<8>, grid, dim3(256), 0, s, ctx, elems, n, gidx, out_off, sums,
                       op_bias(op), combine_value_bytes(op), out);
}

}  // namespace gpu
}  // namespace uda
