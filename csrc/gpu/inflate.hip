// zlib inflate on the device: DefaultCodec map outputs, one RFC 1950 stream per partition, decoded in HBM.
// GzipCodec map outputs too: one RFC 1952 member per partition around the same deflate data. The container is
// uniform for a launch and is looked at twice per stream, ahead of the first block and behind the last one;
// the block and symbol loops between do not know it.
//
// A zlib stream has no framing and nothing indexed inside it, so the unit of parallelism is the stream:
// one wave64 per stream, four waves per workgroup, all streams of a reduce task in one launch (a lane per
// stream would leave the device empty: a task has as many streams as maps, not hundreds of thousands).
//   * The parse is wave-uniform: every lane decodes the same symbol and the values are scalar. The bit
//     buffer (64 bits) is refilled four bytes at a time from a 256-byte register window of the input (the
//     LeanWin idea of decode.hip: two v_readlane per peek, one coalesced load per 252 bytes).
//   * The decode tables live in the wave's LDS slice (WaveLds, under 4 KiB of the 8 KiB a wave may take):
//     a first-level table with sub-tables, built by the code of csrc/codec/inflate_tables.h, the same code
//     the host inflater and its sanitizer program run. Every lane builds the same table into the same slice
//     (same values to the same addresses), so each lane reads only what it wrote itself and no barrier is
//     needed.
//   * Literals are not stored one at a time: lane k keeps the k-th pending literal in a register and the run
//     goes out as one coalesced store when 64 are pending, before a match, before a stored block and at the
//     end of a block. A match therefore always finds its source bytes in memory.
//   * Matches use decode.hip's overlap rule (out[op+i] = out[op-d + i % d] when d < len, the 64-lane vector
//     copy otherwise) behind the same workgroup-scope release / vmcnt(0) / acquire when the source lies above
//     the wave's flushed mark. Stored blocks are a 64-lane vector copy from the input.
// Safety: every table index is masked into tables whose construction checked their capacity; no byte at or
// past dst + raw_len is written and none at or past src + src_len is read (each copy is checked ahead of its
// access); every loop iteration consumes at least one input bit or ends with a status, and bits past the
// input's end are zeros that are never acted on (a field is checked against the bits really there first), so
// a corrupt or truncated stream ends with status != 0: it never spins and never faults.
// The gzip header is walked bytewise ahead of the bit reader under the same contract: every step checks
// ip < ip_end before its read and takes at least one byte or ends with a status, so a header field that never
// terminates cannot spin and no byte at or past src + src_len is read; its optional FHCRC is verified in the
// same walk by a bitwise CRC-32 without a table. Only one member is decoded: what lies behind its trailer is
// the host's to judge (stream_decoder.cc).
// The stream's own check (zlib: Adler-32; gzip: CRC-32, with ISIZE) is read, not verified, here: adler32.hip /
// crc32.hip sum the decoded bytes right behind this launch and the host compares (block_decoder's sibling
// stream_decoder.cc).
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "codec/inflate_tables.h"
#include "kernels.h"

namespace uda {
namespace gpu {

namespace {

using namespace uda::inflate;

constexpr int kWavesPerBlock = 4;
constexpr int kRegWin = 256;   // input bytes held in the register window, 4 per lane
constexpr int kRegAlign = 4;   // its base is ip & ~(kRegAlign - 1)
constexpr int kStage = 64;     // pending literals, one per lane
constexpr int kShortCopy = 64; // a match of up to one byte per lane is a single masked move
constexpr int kVecBytes = 16;
constexpr int kWaveStep = 64 * kVecBytes;

struct WaveLds {
  uint16_t lit[kLitCap];
  uint16_t dist[kDistCap];
  uint16_t cl[kClCap];
  uint16_t work[kWork];
  uint8_t lens[kMaxLit + kMaxDist];
  uint8_t cl_lens[32];
};
static_assert(sizeof(WaveLds) <= 8192, "a wave's decode tables take at most 8 KiB of LDS");

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

struct __attribute__((packed, aligned(1))) U32p {
  uint32_t v;
};
struct __attribute__((packed, aligned(1))) U128 {
  uint32_t a, b, c, d;
};

// ---- own copies of decode.hip's helpers (that file stays as it is)
struct LeanWin {
  uint32_t rw = 0;    // this lane's 4 bytes of the 256-byte window at base
  uint32_t base = 0;  // stream offset of window byte 0
  uint32_t lim = 0;   // bytes [ip, ip + n) are in the window while ip + n <= lim (0: empty)
};

__device__ __forceinline__ void lean_fill(LeanWin& w, const uint8_t* ib, uint32_t ip, uint32_t ip_end, int lane) {
  const uint32_t base = ip & ~(uint32_t)(kRegAlign - 1);
  const uint32_t end = min(base + (uint32_t)kRegWin, ip_end);
  const uint32_t p = base + 4 * (uint32_t)lane;
  uint32_t v = 0;
  if (p + 4 <= end) {
    v = reinterpret_cast<const U32p*>(ib + p)->v;
  } else {
    for (uint32_t k = 0; k < 4; ++k)
      if (p + k < end) v |= (uint32_t)ib[p + k] << (8 * k);
  }
  w.rw = v;
  w.base = base;
  w.lim = end == ip_end ? 0xFFFFFFFFu : end;  // the stream's last window is never refilled
}

// Bytes ip .. ip+3, little-endian; only those below ip_end mean anything (the caller masks the rest).
__device__ __forceinline__ uint32_t lean_peek4(LeanWin& w, const uint8_t* ib, uint32_t ip, uint32_t ip_end, int lane) {
  if (ip + 4 > w.lim) lean_fill(w, ib, ip, ip_end, lane);
  const uint32_t d = ip - w.base;
  const uint32_t i = (d >> 2) & 63;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)w.rw, (int)i);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)w.rw, (int)((i + 1) & 63));
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (d & 3)));
}

// Non-overlapping copy dst[0, len) = src[0, len) by the 64 lanes, 16 bytes per lane and step at any alignment.
__device__ __forceinline__ void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t len, int lane) {
  const uint32_t nv = len & ~(uint32_t)(kVecBytes - 1);
  for (uint32_t i = (uint32_t)lane * kVecBytes; i < nv; i += kWaveStep)
    *reinterpret_cast<U128*>(dst + i) = *reinterpret_cast<const U128*>(src + i);
  for (uint32_t i = nv + lane; i < len; i += 64) dst[i] = src[i];
}

// out[op, op + len) = out[op - d ...] with LZ77 overlap semantics; the caller checked d <= op and the end.
__device__ __forceinline__ void copy_match(uint8_t* ob, uint32_t op, uint32_t d, uint32_t len, uint32_t& flushed, int lane) {
  const uint32_t src = op - d;
  if (src + min(d, len) > flushed) {  // reads bytes this wave stored since its last fence
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's stores completed
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    flushed = op;
  }
  if (len <= (uint32_t)kShortCopy) {
    if ((uint32_t)lane < len) ob[op + lane] = ob[src + (d >= len ? (uint32_t)lane : (uint32_t)lane % d)];
  } else if (d >= len) {
    wave_copy(ob + op, ob + src, len, lane);
  } else {
    for (uint32_t i = lane; i < len; i += 64) ob[op + i] = ob[src + i % d];
  }
}

// The wave's view of one stream. Everything but `lit` is wave-uniform.
struct Stream {
  const uint8_t* ib;
  uint8_t* ob;
  uint32_t ip, ip_end;   // next input byte to enter the bit buffer, end of the stream's bytes
  uint32_t op, op_end;   // next output byte (behind the pending literals), raw_len
  uint64_t bb;           // bit buffer, next bit lowest; bits at and above bc are zero
  uint32_t bc;
  uint32_t npend;        // pending literals: lane k < npend holds the k-th in lit
  uint32_t lit;
  uint32_t flushed;
  LeanWin win;
  int lane;
};

// At least 32 bits in the buffer unless the input ends first.
__device__ __forceinline__ void refill(Stream& s) {
  if (s.bc >= 32) return;
  const uint32_t left = s.ip_end - s.ip;
  if (left == 0) return;
  uint32_t v = lean_peek4(s.win, s.ib, s.ip, s.ip_end, s.lane);
  const uint32_t take = min(left, 4u);
  if (take < 4) v &= (1u << (8 * take)) - 1;
  s.bb |= (uint64_t)v << s.bc;
  s.bc += 8 * take;
  s.ip += take;
}
__device__ __forceinline__ void consume(Stream& s, uint32_t n) {
  s.bb >>= n;
  s.bc -= n;
}
// Drop the bits up to the next byte boundary and hand the whole bytes left in the buffer back to the input.
__device__ __forceinline__ void to_bytes(Stream& s) {
  consume(s, s.bc & 7);
  s.ip -= s.bc >> 3;
  s.bb = 0;
  s.bc = 0;
  // ip stays inside the register window after a stored block's header: the window is based at or below the ip
  // of the refill that filled it and ip only grows between fills, and fewer bytes are handed back than the
  // last refill took (it ran with under 32 bits buffered and LEN / NLEN then took 32). The stream's end may
  // hand back more, up to 7 bytes, but nothing is peeked after it: the Adler-32 is read from memory.
}
__device__ __forceinline__ void flush_literals(Stream& s) {
  if (s.npend == 0) return;
  if ((uint32_t)s.lane < s.npend) s.ob[s.op + s.lane] = (uint8_t)s.lit;  // (op + npend <= op_end: checked per literal)
  s.op += s.npend;
  s.npend = 0;
}
__device__ __forceinline__ uint32_t low_bits(uint32_t n) { return (1u << n) - 1; }

// BTYPE 2 header: the code lengths into L.lens, *nlit / *ndist of them. Returns a status.
__device__ __forceinline__ int dynamic_lengths(Stream& s, WaveLds& L, int* nlit_out, int* ndist_out) {
  refill(s);
  if (s.bc < 14) return kInflateTruncated;
  const int nlit = (int)(s.bb & 31) + 257, ndist = (int)((s.bb >> 5) & 31) + 1, ncl = (int)((s.bb >> 10) & 15) + 4;
  consume(s, 14);
  if (nlit > 286 || ndist > 30) return kInflateCorrupt;
  for (int i = 0; i < kClSyms; ++i) L.cl_lens[i] = 0;
  for (int i = 0; i < ncl; ++i) {
    refill(s);
    if (s.bc < 3) return kInflateTruncated;
    L.cl_lens[cl_order(i) & 31] = (uint8_t)(s.bb & 7);
    consume(s, 3);
  }
  if (!build_table(L.cl_lens, kClSyms, kClRoot, false, L.cl, kClCap, L.work)) return kInflateCorrupt;
  const int total = nlit + ndist;  // <= 316 < sizeof L.lens
  int have = 0;
  while (have < total) {
    refill(s);
    const uint32_t e = uni(lookup(L.cl, kClRoot, (uint32_t)s.bb));
    const uint32_t bits = e & 15, sym = e >> 4;
    if (bits == 0) return s.bc < (uint32_t)kClRoot ? kInflateTruncated : kInflateCorrupt;
    if (bits > s.bc) return kInflateTruncated;
    if (sym < 16) {
      L.lens[have++] = (uint8_t)sym;
      consume(s, bits);
      continue;
    }
    const uint32_t eb = sym == 16 ? 2 : sym == 17 ? 3 : 7;
    if (bits + eb > s.bc) return kInflateTruncated;
    uint32_t rep = (uint32_t)(s.bb >> bits) & low_bits(eb);
    uint32_t v = 0;
    if (sym == 16) {
      if (have == 0) return kInflateCorrupt;  // no previous length
      v = L.lens[have - 1];
      rep += 3;
    } else {
      rep += sym == 17 ? 3 : 11;
    }
    if (have + (int)rep > total) return kInflateCorrupt;  // a repeat past the last length
    for (uint32_t k = 0; k < rep; ++k) L.lens[have++] = (uint8_t)v;
    consume(s, bits + eb);
  }
  if (L.lens[kEndOfBlock] == 0) return kInflateCorrupt;  // no code for end-of-block
  *nlit_out = nlit;
  *ndist_out = ndist;
  return kInflateOk;
}

// The symbols of one Huffman block, tables in L. Returns a status.
__device__ __forceinline__ int huffman_block(Stream& s, const WaveLds& L) {
  for (;;) {
    refill(s);
    uint32_t e = uni(lookup(L.lit, kLitRoot, (uint32_t)s.bb));
    uint32_t used = e & 15;
    const uint32_t sym = e >> 4;
    if (used == 0) return s.bc < (uint32_t)kMaxBits ? kInflateTruncated : kInflateCorrupt;
    if (used > s.bc) return kInflateTruncated;
    if (sym < 256) {
      if (s.op + s.npend >= s.op_end) return kInflateOverflow;
      if ((uint32_t)s.lane == s.npend) s.lit = sym;
      consume(s, used);
      if (++s.npend == (uint32_t)kStage) flush_literals(s);
      continue;
    }
    if (sym == (uint32_t)kEndOfBlock) {
      consume(s, used);
      flush_literals(s);
      return kInflateOk;
    }
    if (sym >= 286) return kInflateCorrupt;
    uint32_t base, eb;
    length_code((int)sym, &base, &eb);
    if (used + eb > s.bc) return kInflateTruncated;
    const uint32_t len = base + ((uint32_t)(s.bb >> used) & low_bits(eb));
    consume(s, used + eb);
    refill(s);
    e = uni(lookup(L.dist, kDistRoot, (uint32_t)s.bb));
    used = e & 15;
    const uint32_t dsym = e >> 4;
    if (used == 0) return s.bc < (uint32_t)kMaxBits ? kInflateTruncated : kInflateCorrupt;
    if (used > s.bc) return kInflateTruncated;
    if (dsym >= 30) return kInflateCorrupt;
    dist_code((int)dsym, &base, &eb);
    if (used + eb > s.bc) return kInflateTruncated;
    const uint32_t d = base + ((uint32_t)(s.bb >> used) & low_bits(eb));
    consume(s, used + eb);
    flush_literals(s);  // a match that reads pending literals must see them
    if (d > s.op) return kInflateCorrupt;  // a distance beyond the bytes produced
    if (len > s.op_end - s.op) return kInflateOverflow;
    copy_match(s.ob, s.op, d, len, s.flushed, s.lane);
    s.op += len;
  }
}

// One header byte at s.ip into *b and into the header's CRC-32 (bitwise, no table); false at the input's end.
__device__ __forceinline__ bool header_byte(Stream& s, uint32_t* b, uint32_t& crc) {
  if (s.ip >= s.ip_end) return false;
  const uint32_t v = uni(s.ib[s.ip]);
  ++s.ip;
  crc ^= v;
  for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1)));
  *b = v;
  return true;
}

// The gzip member header (RFC 1952) from s.ip = 0, bytewise and before the bit reader starts: on kInflateOk
// s.ip is the first deflate byte. Every step checks s.ip < s.ip_end ahead of its read and takes at least one
// byte or returns, so a field that never ends (an FNAME without its zero, an XLEN past the input) ends with
// kInflateTruncated at the input's end. MTIME, XFL, OS and FTEXT are ignored, as zlib ignores them.
__device__ __forceinline__ int gzip_header(Stream& s) {
  uint32_t crc = 0xFFFFFFFFu, b = 0, flg = 0;
  for (int i = 0; i < 10; ++i) {
    if (!header_byte(s, &b, crc)) return kInflateTruncated;
    if ((i == 0 && b != 0x1f) || (i == 1 && b != 0x8b) || (i == 2 && b != 8)) return kInflateCorrupt;
    if (i == 3) {
      flg = b;
      if (flg & 0xE0) return kInflateCorrupt;  // reserved bits
    }
  }
  if (flg & 4) {  // FEXTRA: u16 XLEN, little-endian, and that many bytes
    uint32_t lo, hi;
    if (!header_byte(s, &lo, crc) || !header_byte(s, &hi, crc)) return kInflateTruncated;
    const uint32_t xlen = lo | (hi << 8);
    if (xlen > s.ip_end - s.ip) return kInflateTruncated;
    if (flg & 2) {  // only a header CRC needs the bytes themselves
      for (uint32_t k = 0; k < xlen; ++k)
        if (!header_byte(s, &b, crc)) return kInflateTruncated;
    } else {
      s.ip += xlen;
    }
  }
  for (uint32_t bit = 8; bit <= 16; bit <<= 1) {  // FNAME, FCOMMENT: zero-terminated
    if (!(flg & bit)) continue;
    do {
      if (!header_byte(s, &b, crc)) return kInflateTruncated;
    } while (b != 0);
  }
  if (flg & 2) {  // FHCRC: the low 16 bits of the CRC-32 of the header bytes before it
    const uint32_t want = ~crc & 0xFFFF;
    uint32_t lo, hi;
    if (!header_byte(s, &lo, crc) || !header_byte(s, &hi, crc)) return kInflateTruncated;
    if ((lo | (hi << 8)) != want) return kInflateCorrupt;
  }
  return kInflateOk;
}

__device__ __forceinline__ int inflate_stream(Stream& s, WaveLds& L, int container, uint32_t* check, uint32_t* isize) {
  if (container == kContainerGzip) {
    const int st = gzip_header(s);
    if (st) return st;
  } else {
    refill(s);
    if (s.bc < 16) return kInflateTruncated;
    if (!zlib_header_ok((uint32_t)(s.bb & 0xFF), (uint32_t)((s.bb >> 8) & 0xFF))) return kInflateCorrupt;
    consume(s, 16);
  }
  for (;;) {
    refill(s);
    if (s.bc < 3) return kInflateTruncated;
    const bool last = s.bb & 1;
    const uint32_t type = (uint32_t)(s.bb >> 1) & 3;
    consume(s, 3);
    if (type == 3) return kInflateCorrupt;
    if (type == 0) {
      consume(s, s.bc & 7);
      refill(s);
      if (s.bc < 32) return kInflateTruncated;
      const uint32_t len = (uint32_t)s.bb & 0xFFFF, nlen = (uint32_t)(s.bb >> 16) & 0xFFFF;
      if (len != (nlen ^ 0xFFFF)) return kInflateCorrupt;
      consume(s, 32);
      to_bytes(s);
      if (len > s.ip_end - s.ip) return kInflateTruncated;
      if (len > s.op_end - s.op) return kInflateOverflow;
      wave_copy(s.ob + s.op, s.ib + s.ip, len, s.lane);
      s.ip += len;
      s.op += len;
    } else {
      int nlit = kMaxLit, ndist = kMaxDist;
      if (type == 1) {
        fixed_lengths(L.lens);
      } else {
        const int st = dynamic_lengths(s, L, &nlit, &ndist);
        if (st) return st;
      }
      if (!build_table(L.lens, nlit, kLitRoot, true, L.lit, kLitCap, L.work)) return kInflateCorrupt;
      if (!build_table(L.lens + nlit, ndist, kDistRoot, true, L.dist, kDistCap, L.work)) return kInflateCorrupt;
      const int st = huffman_block(s, L);
      if (st) return st;
    }
    if (last) break;
  }
  to_bytes(s);
  const uint8_t* p = s.ib + s.ip;
  if (container == kContainerGzip) {  // CRC-32 and ISIZE, little-endian
    if (s.ip_end - s.ip < 8) return kInflateTruncated;
    *check = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    *isize = (uint32_t)p[4] | ((uint32_t)p[5] << 8) | ((uint32_t)p[6] << 16) | ((uint32_t)p[7] << 24);
    s.ip += 8;
    return kInflateOk;
  }
  if (s.ip_end - s.ip < 4) return kInflateTruncated;
  *check = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
  s.ip += 4;
  return kInflateOk;
}

__global__ void __launch_bounds__(64 * kWavesPerBlock)
inflate_kernel(const uint8_t* in, uint8_t* out, const InflateDesc* descs, int n, InflateResult* results, int container) {
  __shared__ WaveLds lds[kWavesPerBlock];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const int idx = (int)blockIdx.x * kWavesPerBlock + wave;
  if (idx >= n) return;  // (whole waves: the kernel has no workgroup barrier)
  const InflateDesc d = descs[idx];
  Stream s;
  s.ib = in ? in + d.src : reinterpret_cast<const uint8_t*>((uintptr_t)d.src);
  s.ob = out + d.dst;
  s.ip = 0;
  s.op = 0;
  s.bb = 0;
  s.bc = 0;
  s.npend = 0;
  s.lit = 0;
  s.flushed = 0;
  s.lane = lane;
  uint32_t check = 0, isize = 0;
  int status;
  constexpr int64_t kLimit = 1ll << 31;
  if (d.src_len < 0 || d.src_len >= kLimit || d.raw_len < 0 || d.raw_len >= kLimit) {
    s.ip_end = s.op_end = 0;
    status = kInflateTooBig;
  } else {
    s.ip_end = (uint32_t)d.src_len;
    s.op_end = (uint32_t)d.raw_len;
    status = inflate_stream(s, lds[wave], container, &check, &isize);
  }
  if (lane == 0) {
    InflateResult r;
    r.consumed = (int64_t)s.ip;
    r.produced = (int64_t)s.op;
    r.check_stored = check;
    r.status = status;
    r.isize = isize;
    results[idx] = r;
  }
}

}  // namespace

void launch_inflate_streams(const uint8_t* in, uint8_t* out, const InflateDesc* d, int n, InflateResult* r, hipStream_t s,
                            int container) {
  if (n <= 0) return;
  if (container != kContainerZlib && container != kContainerGzip)
    throw std::invalid_argument("launch_inflate_streams: unknown container " + std::to_string(container));
  const int blocks = (n + kWavesPerBlock - 1) / kWavesPerBlock;
  hipLaunchKernelGGL(inflate_kernel, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0, s, in, out, d, n, r, container);
}

InflateGeometry inflate_geometry() {
  return InflateGeometry{kRegWin, kRegAlign, kStage, kWavesPerBlock, (int)sizeof(WaveLds)};
}

}  // namespace gpu
}  // namespace uda
