// zstd on the device: ZStandardCodec map outputs, one RFC 8878 frame per partition, decoded in HBM.
//
// As in inflate.hip the unit of parallelism is the stream: one wave64 per frame, four waves per workgroup, all
// frames of a reduce task in one launch, and the output written in place, so any Window_Size is servable.
//   * The parse is wave-uniform: every lane reads the same headers, builds the same tables and decodes the same
//     sequences; the values are scalar. Backward bitstreams are read through a 64-bit container that is
//     reloaded from memory about twice per sequence (Back).
//   * The tables live in the wave's LDS slice (WaveLds: Huffman 2^11 x 2 B, literal lengths and match lengths
//     2^9 x 4 B, offsets 2^8 x 4 B, and the builders' work area; under 16 KiB) and stay across the blocks of a
//     frame, since Repeat mode and Treeless literals use the previous block's. They are built by the code of
//     csrc/codec/zstd_tables.h, the same code the host decoder and its sanitizer program run. Every lane builds
//     the same table into the same slice (same values to the same addresses), so each lane reads only what it
//     wrote itself and no barrier is needed.
//   * A block's Huffman literals are decoded first, into the frame's 128 KiB literal scratch in HBM: the four
//     streams of a 4-stream section by four lanes, one each, from the shared LDS table; a single stream by one
//     lane. Raw literals are read from the input and RLE literals are splatted: neither needs the scratch.
//   * Each sequence copies its literal run with the 64-lane vector copy and its match with inflate.hip's overlap
//     rule (out[op+i] = out[op-d + i % d] when d < len) behind the same workgroup-scope release / vmcnt(0) /
//     acquire when the source lies above the wave's flushed mark. (Own copies of those helpers.)
// Safety: every table index is masked into tables whose construction checked their capacity; no byte at or past
// dst + raw_len is written and none at or past src + src_len is read (each copy and each field is checked ahead
// of its access; a backward stream's container never loads outside its stream); literal scratch writes stay
// below the section's regenerated size, which is checked against the scratch. Every loop is bounded by a count
// read from the input and checked (symbols of a section, sequences of a block, bytes of a block) and each turn
// takes input or produces output or ends with a status, so a corrupt or truncated frame ends with status != 0
// and a reason: it never spins and never faults.
// The content checksum is read, not verified, here: xxh64.hip sums the decoded bytes behind this launch when a
// frame carries one, and the host compares (stream_decoder.cc).
#include <hip/hip_runtime.h>

#include "codec/zstd_tables.h"
#include "kernels.h"

namespace uda {
namespace gpu {

namespace {

using namespace uda::zstd;

constexpr int kWavesPerBlock = 4;
constexpr int kShortCopy = 64;
constexpr int kVecBytes = 16;
constexpr int kWaveStep = 64 * kVecBytes;
constexpr uint32_t kLitScratch = 128 * 1024;
static_assert(kLitScratch == kBlockMax, "a literals section is at most one block");

struct WaveLds {
  uint16_t huf[kHufCap];
  uint32_t ll[kLlCap];
  uint32_t ml[kMlCap];
  uint32_t of[kOfCap];
  HufScratch hw;
  int16_t norm[kMaxSyms + 1];
  uint16_t work[kMaxSyms + 1];
};
static_assert(sizeof(WaveLds) <= 16384, "a wave's tables take at most 16 KiB of LDS: four waves stay within 64 KiB");

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

struct __attribute__((packed, aligned(1))) U64p {
  uint64_t v;
};
struct __attribute__((packed, aligned(1))) U128 {
  uint32_t a, b, c, d;
};

// ---- own copies of inflate.hip's helpers (that file stays as it is)
__device__ __forceinline__ void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t len, int lane) {
  const uint32_t nv = len & ~(uint32_t)(kVecBytes - 1);
  for (uint32_t i = (uint32_t)lane * kVecBytes; i < nv; i += kWaveStep)
    *reinterpret_cast<U128*>(dst + i) = *reinterpret_cast<const U128*>(src + i);
  for (uint32_t i = nv + lane; i < len; i += 64) dst[i] = src[i];
}

__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's stores completed
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// out[op, op + len) = out[op - d ...] with LZ77 overlap semantics; the caller checked d <= op and the end.
__device__ __forceinline__ void copy_match(uint8_t* ob, uint32_t op, uint32_t d, uint32_t len, uint32_t& flushed, int lane) {
  const uint32_t src = op - d;
  if (src + min(d, len) > flushed) {  // reads bytes this wave stored since its last fence
    wave_fence();
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

// ---- a backward bitstream p[0, n): the next bit to read lies below `bit`; bits below 0 read as zero
struct Back {
  const uint8_t* p;
  uint32_t n;
  int32_t bit;
  int32_t cb;     // stream bit of the container's bit 0 (a multiple of 8)
  uint64_t cont;  // the stream's bytes [cb / 8, cb / 8 + 8), those at or past n as zero
};
__device__ __forceinline__ uint64_t load64(const uint8_t* p, uint32_t n, uint32_t off) {
  if (off + 8 <= n) return reinterpret_cast<const U64p*>(p + off)->v;
  uint64_t v = 0;
  for (uint32_t k = 0; k < 8; ++k)
    if (off + k < n) v |= (uint64_t)p[off + k] << (8 * k);
  return v;
}
__device__ __forceinline__ void back_reload(Back& b) {
  const int32_t top = (b.bit + 7) >> 3;
  const int32_t off = top > 8 ? top - 8 : 0;
  b.cb = off * 8;
  b.cont = load64(b.p, b.n, (uint32_t)off);
}
__device__ __forceinline__ bool back_init(Back& b, const uint8_t* p, uint32_t n) {
  b.p = p;
  b.n = n;
  b.bit = 0;
  b.cb = 0;
  b.cont = 0;
  if (n == 0) return false;
  const uint32_t last = p[n - 1];
  if (last == 0) return false;
  b.bit = (int32_t)(n - 1) * 8 + highbit(last);
  back_reload(b);
  return true;
}
// The nb <= 32 bits below b.bit; does not move.
__device__ __forceinline__ uint32_t back_peek(Back& b, uint32_t nb) {
  if (nb == 0) return 0;
  const uint32_t mask = nb >= 32 ? 0xFFFFFFFFu : (1u << nb) - 1;
  const int32_t lo = b.bit - (int32_t)nb;
  if (lo < b.cb && b.cb > 0) back_reload(b);  // afterwards b.bit - b.cb >= 57, or b.cb == 0
  if (lo >= b.cb) return (uint32_t)(b.cont >> (uint32_t)(lo - b.cb)) & mask;
  if (b.bit <= 0) return 0;  // (b.cb == 0 and lo < 0: the stream's first bits, zeros below them)
  return ((uint32_t)b.cont & ((1u << b.bit) - 1)) << (uint32_t)(-lo);  // b.bit < nb <= 32
}
__device__ __forceinline__ uint32_t back_take(Back& b, uint32_t nb) {
  const uint32_t v = back_peek(b, nb);
  b.bit -= (int32_t)nb;
  return v;
}

// The wave's view of one frame; everything is wave-uniform.
struct Frame {
  const uint8_t* ib;
  uint8_t* ob;
  uint8_t* scratch;
  uint32_t ip, ip_end;
  uint32_t op, op_end;
  uint32_t flushed;
  int huf_bits, ll_log, of_log, ml_log;  // 0 / -1: no table yet
  uint32_t rep[3];
  int reason;
  int lane;
};

__device__ __forceinline__ int bad(Frame& f, int status, int reason) {
  f.reason = reason;
  return status;
}
__device__ __forceinline__ uint32_t byte_at(const Frame& f, uint32_t at) { return uni(f.ib[at]); }  // the caller checked at < ip_end
__device__ __forceinline__ uint32_t le_at(const Frame& f, uint32_t at, int n) {
  uint32_t v = 0;
  for (int k = 0; k < n; ++k) v |= byte_at(f, at + k) << (8 * k);
  return v;
}

// One stream of a Huffman literals section, by one lane: count symbols into dst. false: the stream is bad.
__device__ __forceinline__ bool huf_lane(const uint16_t* table, int bits, const uint8_t* p, uint32_t n, uint8_t* dst, uint32_t count) {
  Back b;
  if (!back_init(b, p, n)) return false;
  const uint32_t mask = (1u << bits) - 1;
  for (uint32_t i = 0; i < count; ++i) {  // every symbol takes at least one bit
    if (b.bit <= 0) return false;
    const uint32_t e = table[back_peek(b, (uint32_t)bits) & mask];
    dst[i] = (uint8_t)e;
    b.bit -= (int32_t)(e >> 8);
  }
  return b.bit == 0;
}

// One of the three sequence tables by its mode, from f.ib[at, end); *used = the bytes it took.
__device__ __forceinline__ int seq_table(Frame& f, WaveLds& L, int mode, uint32_t* table, int cap, int* log, int max_log,
                                         int max_sym, int which, uint32_t at, uint32_t end, uint32_t* used) {
  int nsym = 0, alog = 0;
  *used = 0;
  if (mode == 0) {
    nsym = which == 0 ? predefined_ll(L.norm, &alog) : which == 1 ? predefined_of(L.norm, &alog) : predefined_ml(L.norm, &alog);
    if (!fse_build(L.norm, nsym, alog, table, cap, L.work)) return bad(f, kInflateCorrupt, kZstdFseTable);
    *log = alog;
  } else if (mode == 1) {
    if (at >= end) return bad(f, kInflateTruncated, kZstdInputEnds);
    const uint32_t sym = byte_at(f, at);
    if (sym > (uint32_t)max_sym) return bad(f, kInflateCorrupt, kZstdFseTable);
    fse_build_rle(sym, table);
    *log = 0;
    *used = 1;
  } else if (mode == 2) {
    size_t took = 0;
    if (!fse_read_description(f.ib + at, end - at, max_log, max_sym, L.norm, &nsym, &alog, &took))
      return bad(f, kInflateCorrupt, kZstdFseTable);
    if (!fse_build(L.norm, nsym, alog, table, cap, L.work)) return bad(f, kInflateCorrupt, kZstdFseTable);
    *log = alog;
    *used = (uint32_t)took;
  } else if (*log < 0) {
    return bad(f, kInflateCorrupt, kZstdRepeatMode);
  }
  return kInflateOk;
}

// len literals of the block, from its literal source (kind 0: bytes at lit; 1: the byte `rle`), to ob + op.
__device__ __forceinline__ void put_literals(Frame& f, int kind, const uint8_t* lit, uint32_t rle, uint32_t len) {
  uint8_t* const to = f.ob + f.op;
  if (kind == 1) {
    for (uint32_t i = f.lane; i < len; i += 64) to[i] = (uint8_t)rle;
  } else if (len <= (uint32_t)kShortCopy) {
    if ((uint32_t)f.lane < len) to[f.lane] = lit[f.lane];
  } else {
    wave_copy(to, lit, len, f.lane);
  }
}

// A compressed block f.ib[at, at + n): output at f.op, at most block_max bytes and never past op_end.
__device__ __forceinline__ int compressed_block(Frame& f, WaveLds& L, uint32_t at, uint32_t n, uint32_t block_max) {
  const uint32_t end = at + n;
  // ---- literals section
  if (n < 1) return bad(f, kInflateTruncated, kZstdLiterals);
  const uint32_t b0 = byte_at(f, at);
  const uint32_t type = b0 & 3, sf = (b0 >> 2) & 3;
  uint32_t hdr, regen, comp = 0, streams = 1;
  if (type < 2) {
    hdr = sf == 1 ? 2 : sf == 3 ? 3 : 1;
    if (n < hdr) return bad(f, kInflateTruncated, kZstdLiterals);
    regen = hdr == 1 ? b0 >> 3 : le_at(f, at, (int)hdr) >> 4;
  } else {
    hdr = sf < 2 ? 3 : sf == 2 ? 4 : 5;
    if (n < hdr) return bad(f, kInflateTruncated, kZstdLiterals);
    const uint32_t bits = sf < 2 ? 10 : sf == 2 ? 14 : 18;
    const uint64_t v = ((uint64_t)le_at(f, at, hdr < 4 ? (int)hdr : 4) | (hdr == 5 ? (uint64_t)byte_at(f, at + 4) << 32 : 0)) >> 4;
    regen = (uint32_t)(v & ((1u << bits) - 1));
    comp = (uint32_t)((v >> bits) & ((1u << bits) - 1));
    streams = sf == 0 ? 1 : 4;
  }
  if (regen > kLitScratch) return bad(f, kInflateCorrupt, kZstdLiterals);
  uint32_t pos = at + hdr;
  int kind = 0;
  const uint8_t* lit = f.scratch;
  uint32_t rle = 0;
  if (type == 0) {
    if (end - pos < regen) return bad(f, kInflateTruncated, kZstdLiterals);
    lit = f.ib + pos;
    pos += regen;
  } else if (type == 1) {
    if (end - pos < 1) return bad(f, kInflateTruncated, kZstdLiterals);
    kind = 1;
    rle = byte_at(f, pos);
    pos += 1;
  } else {
    if (end - pos < comp) return bad(f, kInflateTruncated, kZstdLiterals);
    uint32_t p = pos, left = comp;
    if (type == 2) {
      size_t used = 0;
      bool fse_coded = false;
      int bits = 0;
      const int hs = huf_read_description(f.ib + p, left, L.huf, kHufCap, &bits, &used, &fse_coded, &L.hw);
      if (hs != kHufOk) return bad(f, hs == kHufTruncated ? kInflateTruncated : kInflateCorrupt, kZstdHuffmanTree);
      f.huf_bits = (int)uni((uint32_t)bits);
      p += (uint32_t)used;
      left -= (uint32_t)used;
    } else if (f.huf_bits == 0) {
      return bad(f, kInflateCorrupt, kZstdTreeless);
    }
    // the streams' extents, wave-uniform; then lane j < streams decodes stream j into the scratch
    uint32_t my_at = p, my_len = left, to_at = 0, to_len = regen;  // this lane's stream and where its symbols go
    if (streams == 4) {
      if (left < 6) return bad(f, kInflateTruncated, kZstdLiterals);
      const uint32_t s1 = le_at(f, p, 2), s2 = le_at(f, p + 2, 2), s3 = le_at(f, p + 4, 2);
      if (6 + s1 + s2 + s3 > left) return bad(f, kInflateCorrupt, kZstdLiterals);
      const uint32_t seg = (regen + 3) / 4;
      if (3 * seg > regen) return bad(f, kInflateCorrupt, kZstdLiterals);
      const uint32_t j = (uint32_t)f.lane & 3;
      my_at = p + 6 + (j > 0 ? s1 : 0) + (j > 1 ? s2 : 0) + (j > 2 ? s3 : 0);
      my_len = j == 0 ? s1 : j == 1 ? s2 : j == 2 ? s3 : left - 6 - s1 - s2 - s3;
      to_at = j * seg;
      to_len = j < 3 ? seg : regen - 3 * seg;
    }
    bool ok = true;
    if ((uint32_t)f.lane < streams) ok = huf_lane(L.huf, f.huf_bits, f.ib + my_at, my_len, f.scratch + to_at, to_len);
    if (__any(!ok)) return bad(f, kInflateCorrupt, kZstdHuffmanStream);
    wave_fence();  // the literal copies below read what those lanes stored
    pos += comp;
  }
  // ---- sequences section
  if (end - pos < 1) return bad(f, kInflateTruncated, kZstdSequences);
  uint32_t nseq = byte_at(f, pos++);
  if (nseq >= 128) {
    if (nseq == 255) {
      if (end - pos < 2) return bad(f, kInflateTruncated, kZstdSequences);
      nseq = le_at(f, pos, 2) + 0x7F00;
      pos += 2;
    } else {
      if (end - pos < 1) return bad(f, kInflateTruncated, kZstdSequences);
      nseq = ((nseq - 128) << 8) + byte_at(f, pos++);
    }
  }
  const uint32_t start = f.op;
  uint32_t lp = 0;
  if (nseq > 0) {
    if (end - pos < 1) return bad(f, kInflateTruncated, kZstdSequences);
    const uint32_t modes = byte_at(f, pos++);
    uint32_t used = 0;
    int st = seq_table(f, L, (int)(modes >> 6), L.ll, kLlCap, &f.ll_log, kLlMaxLog, kLlMaxSym, 0, pos, end, &used);
    if (st) return st;
    pos += used;
    st = seq_table(f, L, (int)((modes >> 4) & 3), L.of, kOfCap, &f.of_log, kOfMaxLog, kOfMaxSym, 1, pos, end, &used);
    if (st) return st;
    pos += used;
    st = seq_table(f, L, (int)((modes >> 2) & 3), L.ml, kMlCap, &f.ml_log, kMlMaxLog, kMlMaxSym, 2, pos, end, &used);
    if (st) return st;
    pos += used;
    if (pos > end) return bad(f, kInflateTruncated, kZstdSequences);
    Back b;
    if (!back_init(b, f.ib + pos, end - pos)) return bad(f, kInflateCorrupt, kZstdBitstream);
    const uint32_t llm = (1u << f.ll_log) - 1, ofm = (1u << f.of_log) - 1, mlm = (1u << f.ml_log) - 1;
    uint32_t sl = uni(back_take(b, (uint32_t)f.ll_log));
    uint32_t so = uni(back_take(b, (uint32_t)f.of_log));
    uint32_t sm = uni(back_take(b, (uint32_t)f.ml_log));
    if (b.bit < 0) return bad(f, kInflateCorrupt, kZstdBitstream);
    for (uint32_t i = 0; i < nseq; ++i) {  // every sequence produces at least its match's three bytes
      const uint32_t el = uni(L.ll[sl & llm]), eo = uni(L.of[so & ofm]), em = uni(L.ml[sm & mlm]);
      const uint32_t oc = fse_sym(eo), lc = fse_sym(el), mc = fse_sym(em);
      if (oc > (uint32_t)kOfMaxSym || lc > (uint32_t)kLlMaxSym || mc > (uint32_t)kMlMaxSym)
        return bad(f, kInflateCorrupt, kZstdSequenceCode);
      const uint32_t ov = (1u << oc) + uni(back_take(b, oc));
      const uint32_t mlen = ml_base(mc) + uni(back_take(b, ml_bits(mc)));
      const uint32_t llen = ll_base(lc) + uni(back_take(b, ll_bits(lc)));
      if (i + 1 < nseq) {
        sl = fse_base(el) + uni(back_take(b, fse_nbits(el)));
        sm = fse_base(em) + uni(back_take(b, fse_nbits(em)));
        so = fse_base(eo) + uni(back_take(b, fse_nbits(eo)));
      }
      if (b.bit < 0) return bad(f, kInflateCorrupt, kZstdBitstream);
      if (llen > regen - lp) return bad(f, kInflateCorrupt, kZstdLiteralsShort);
      if (llen + mlen > block_max - (f.op - start)) return bad(f, kInflateCorrupt, kZstdBlockSize);
      if (llen + mlen > f.op_end - f.op) return bad(f, kInflateOverflow, kZstdOutputFull);
      put_literals(f, kind, lit + lp, rle, llen);
      f.op += llen;
      lp += llen;
      const uint32_t off = apply_offset(ov, llen, f.rep);
      if (off > f.op) return bad(f, kInflateCorrupt, kZstdOffset);  // reaches before the frame's first byte
      copy_match(f.ob, f.op, off, mlen, f.flushed, f.lane);
      f.op += mlen;
    }
    if (b.bit != 0) return bad(f, kInflateCorrupt, kZstdBitstreamLeft);
  } else if (pos != end) {
    return bad(f, kInflateCorrupt, kZstdSequences);
  }
  const uint32_t rest = regen - lp;
  if (rest > block_max - (f.op - start)) return bad(f, kInflateCorrupt, kZstdBlockSize);
  if (rest > f.op_end - f.op) return bad(f, kInflateOverflow, kZstdOutputFull);
  put_literals(f, kind, lit + lp, rle, rest);
  f.op += rest;
  if (type >= 2) wave_fence();  // the next block's literals overwrite the scratch these copies read
  return kInflateOk;
}

__device__ __forceinline__ int decode_frame(Frame& f, WaveLds& L, uint32_t* check, uint32_t* has_sum) {
  if (f.ip_end < 5) return bad(f, kInflateTruncated, kZstdInputEnds);
  if (le_at(f, 0, 4) != 0xFD2FB528u) return bad(f, kInflateCorrupt, kZstdMagic);
  const uint32_t d = byte_at(f, 4);
  if (d & 0x08) return bad(f, kInflateCorrupt, kZstdReservedBit);
  const bool single = d & 0x20;
  const uint32_t did = d & 3, fcsf = d >> 6;
  const uint32_t did_n = did == 3 ? 4 : did, fcs_n = fcsf == 0 ? (single ? 1u : 0u) : 1u << fcsf;
  const uint32_t hl = 5 + (single ? 0 : 1) + did_n + fcs_n;
  if (f.ip_end < hl) return bad(f, kInflateTruncated, kZstdInputEnds);
  uint32_t at = 5;
  uint64_t window = 0;
  if (!single) {
    const uint32_t w = byte_at(f, at++);
    const uint64_t base = 1ull << (10 + (w >> 3));
    window = base + (base >> 3) * (w & 7);
  }
  if (did_n && le_at(f, at, (int)did_n) != 0) return bad(f, kInflateCorrupt, kZstdDictionary);
  at += did_n;
  uint64_t fcs = 0;
  for (uint32_t k = 0; k < fcs_n; ++k) fcs |= (uint64_t)byte_at(f, at + k) << (8 * k);
  if (fcs_n == 2) fcs += 256;
  at += fcs_n;
  if (single) window = fcs;
  const uint32_t block_max = (uint32_t)(window < kBlockMax ? window : kBlockMax);
  *has_sum = (d >> 2) & 1;
  f.ip = at;
  for (bool last = false; !last;) {  // every block takes its three header bytes
    if (f.ip_end - f.ip < 3) return bad(f, kInflateTruncated, kZstdInputEnds);
    const uint32_t bh = le_at(f, f.ip, 3);
    f.ip += 3;
    last = bh & 1;
    const uint32_t type = (bh >> 1) & 3, size = bh >> 3;
    if (type == 3) return bad(f, kInflateCorrupt, kZstdBlockType);
    if (size > block_max) return bad(f, kInflateCorrupt, kZstdBlockSize);
    if (type == 0) {
      if (size > f.ip_end - f.ip) return bad(f, kInflateTruncated, kZstdInputEnds);
      if (size > f.op_end - f.op) return bad(f, kInflateOverflow, kZstdOutputFull);
      wave_copy(f.ob + f.op, f.ib + f.ip, size, f.lane);
      f.ip += size;
      f.op += size;
    } else if (type == 1) {
      if (f.ip_end - f.ip < 1) return bad(f, kInflateTruncated, kZstdInputEnds);
      if (size > f.op_end - f.op) return bad(f, kInflateOverflow, kZstdOutputFull);
      const uint32_t v = byte_at(f, f.ip);
      for (uint32_t i = f.lane; i < size; i += 64) f.ob[f.op + i] = (uint8_t)v;
      f.ip += 1;
      f.op += size;
    } else {
      if (size > f.ip_end - f.ip) return bad(f, kInflateTruncated, kZstdInputEnds);
      const int st = compressed_block(f, L, f.ip, size, block_max);
      if (st) return st;
      f.ip += size;
    }
  }
  if (fcs_n && fcs != (uint64_t)f.op) return bad(f, kInflateCorrupt, kZstdContentSize);
  if (*has_sum) {
    if (f.ip_end - f.ip < 4) return bad(f, kInflateTruncated, kZstdInputEnds);
    *check = le_at(f, f.ip, 4);
    f.ip += 4;
  }
  return kInflateOk;
}

__global__ void __launch_bounds__(64 * kWavesPerBlock)
zstd_kernel(const uint8_t* in, uint8_t* out, const InflateDesc* descs, int n, ZstdResult* results, uint8_t* lit_scratch) {
  __shared__ WaveLds lds[kWavesPerBlock];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const int idx = (int)blockIdx.x * kWavesPerBlock + wave;
  if (idx >= n) return;  // (whole waves: the kernel has no workgroup barrier)
  const InflateDesc d = descs[idx];
  Frame f;
  f.ib = in ? in + d.src : reinterpret_cast<const uint8_t*>((uintptr_t)d.src);
  f.ob = out + d.dst;
  f.scratch = lit_scratch + (size_t)idx * kLitScratch;
  f.ip = 0;
  f.op = 0;
  f.flushed = 0;
  f.huf_bits = 0;
  f.ll_log = f.of_log = f.ml_log = -1;
  f.rep[0] = 1;
  f.rep[1] = 4;
  f.rep[2] = 8;
  f.reason = kZstdFine;
  f.lane = lane;
  uint32_t check = 0, has_sum = 0;
  int status;
  constexpr int64_t kLimit = 1ll << 31;
  if (d.src_len < 0 || d.src_len >= kLimit || d.raw_len < 0 || d.raw_len >= kLimit) {
    f.ip_end = f.op_end = 0;
    status = kInflateTooBig;
  } else {
    f.ip_end = (uint32_t)d.src_len;
    f.op_end = (uint32_t)d.raw_len;
    status = decode_frame(f, lds[wave], &check, &has_sum);
  }
  if (lane == 0) {
    ZstdResult r;
    r.consumed = (int64_t)f.ip;
    r.produced = (int64_t)f.op;
    r.check_stored = check;
    r.status = status;
    r.reason = f.reason;
    r.has_checksum = has_sum;
    results[idx] = r;
  }
}

}  // namespace

void launch_zstd_frames(const uint8_t* in, uint8_t* out, const InflateDesc* d, int n, ZstdResult* r, uint8_t* lit_scratch,
                        hipStream_t s) {
  if (n <= 0) return;
  const int blocks = (n + kWavesPerBlock - 1) / kWavesPerBlock;
  hipLaunchKernelGGL(zstd_kernel, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0, s, in, out, d, n, r, lit_scratch);
}

ZstdGeometry zstd_geometry() { return ZstdGeometry{kWavesPerBlock, (int)sizeof(WaveLds), (int)kLitScratch}; }

const char* zstd_reason_text(int reason) {
  switch (reason) {
    case kZstdMagic: return "wrong magic";
    case kZstdReservedBit: return "reserved descriptor bit";
    case kZstdDictionary: return "needs a dictionary";
    case kZstdBlockType: return "reserved block type";
    case kZstdBlockSize: return "block larger than min(window, 128 KiB)";
    case kZstdLiterals: return "bad literals section";
    case kZstdHuffmanTree: return "bad Huffman tree";
    case kZstdHuffmanStream: return "bad Huffman stream";
    case kZstdTreeless: return "Treeless literals with no earlier table";
    case kZstdSequences: return "bad sequences section";
    case kZstdFseTable: return "bad FSE table";
    case kZstdRepeatMode: return "Repeat mode with no earlier table";
    case kZstdBitstream: return "sequence bitstream ends early";
    case kZstdBitstreamLeft: return "sequence bitstream not used up";
    case kZstdSequenceCode: return "sequence code out of range";
    case kZstdLiteralsShort: return "sequence takes more literals than the block has";
    case kZstdOffset: return "offset reaches before the frame's first byte";
    case kZstdContentSize: return "content size does not match";
    case kZstdInputEnds: return "truncated";
    case kZstdOutputFull: return "more output than its index says";
    default: return "refused";
  }
}

}  // namespace gpu
}  // namespace uda
