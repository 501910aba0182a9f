// Zstandard (RFC 8878): one-shot and incremental decoders and a small encoder. See uda/codec.h.
//
// One block decoder serves both entry points: decode_block writes a block's bytes at out[op..) with the frame's
// earlier output [hist, op) behind it. The one-shot call hands it the caller's buffer; ZstdDecoder hands it its
// sliding history buffer. The entropy tables are built by zstd_tables.h and live in an Entropy per frame, since
// Repeat mode and Treeless literals use the previous block's tables.
#include <algorithm>
#include <cstring>

#include "uda/codec.h"
#include "uda/error.h"
#include "zstd_tables.h"

namespace uda {
namespace {
using namespace zstd;

constexpr uint32_t kMagic = 0xFD2FB528u, kSkipMagic = 0x184D2A50u;
constexpr uint64_t kWindowMax = 128ull << 20;  // libzstd's default windowLogMax of 27

[[noreturn]] void fail(const char* what) { throw UdaError(std::string("corrupt zstd frame: ") + what); }

// (memcpy / memset with a null pointer are undefined even for no bytes: an empty vector's data() is one)
inline void copy(uint8_t* dst, const uint8_t* src, size_t n) {
  if (n) std::memcpy(dst, src, n);
}
inline void fill(uint8_t* dst, uint8_t v, size_t n) {
  if (n) std::memset(dst, v, n);
}
inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le24(const uint8_t* p) { return le16(p) | ((uint32_t)p[2] << 16); }
inline uint32_t le32(const uint8_t* p) { return le24(p) | ((uint32_t)p[3] << 24); }
inline uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }

// ---- XXH64 (the content checksum is its low 32 bits, seed 0)
constexpr uint64_t kP1 = 0x9E3779B185EBCA87ull, kP2 = 0xC2B2AE3D27D4EB4Full, kP3 = 0x165667B19E3779F9ull,
                   kP4 = 0x85EBCA77C2B2AE63ull, kP5 = 0x27D4EB2F165667C5ull;
inline uint64_t rotl(uint64_t v, int r) { return (v << r) | (v >> (64 - r)); }
inline uint64_t xround(uint64_t acc, uint64_t in) { return rotl(acc + in * kP2, 31) * kP1; }
inline uint64_t xmerge(uint64_t h, uint64_t v) { return (h ^ xround(0, v)) * kP1 + kP4; }

struct Xxh64 {
  uint64_t v[4] = {kP1 + kP2, kP2, 0, 0 - kP1};
  uint64_t total = 0;
  uint8_t buf[32];
  size_t n = 0;
  void update(const uint8_t* p, size_t len) {
    total += len;
    if (n) {
      const size_t k = std::min(len, 32 - n);
      std::memcpy(buf + n, p, k);
      n += k;
      p += k;
      len -= k;
      if (n < 32) return;
      for (int j = 0; j < 4; ++j) v[j] = xround(v[j], le64(buf + 8 * j));
      n = 0;
    }
    for (; len >= 32; p += 32, len -= 32)
      for (int j = 0; j < 4; ++j) v[j] = xround(v[j], le64(p + 8 * j));
    if (len) std::memcpy(buf, p, len);
    n = len;
  }
  uint64_t digest() const {
    uint64_t h;
    if (total >= 32) {
      h = rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18);
      for (int j = 0; j < 4; ++j) h = xmerge(h, v[j]);
    } else {
      h = kP5;  // (seed 0)
    }
    h += total;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) h = rotl(h ^ xround(0, le64(buf + i)), 27) * kP1 + kP4;
    if (i + 4 <= n) {
      h = rotl(h ^ ((uint64_t)le32(buf + i) * kP1), 23) * kP2 + kP3;
      i += 4;
    }
    for (; i < n; ++i) h = rotl(h ^ (buf[i] * kP5), 11) * kP1;
    h ^= h >> 33;
    h *= kP2;
    h ^= h >> 29;
    h *= kP3;
    h ^= h >> 32;
    return h;
  }
};

// ---- a frame's entropy state
struct Entropy {
  uint16_t huf[kHufCap];
  int huf_bits = 0;  // 0: no literal table yet
  uint32_t ll[kLlCap], of[kOfCap], ml[kMlCap];
  int ll_log = -1, of_log = -1, ml_log = -1;  // -1: no table yet
  uint32_t rep[3] = {1, 4, 8};
  std::vector<uint8_t> lit;  // decoded literals of the current block
  void reset() {
    huf_bits = 0;
    ll_log = of_log = ml_log = -1;
    rep[0] = 1;
    rep[1] = 4;
    rep[2] = 8;
  }
};

// Decodes the Huffman tree description at p[0, n); returns its length.
size_t read_huf_table(Entropy* e, const uint8_t* p, size_t n, ZstdStats* st) {
  HufScratch w;
  size_t used = 0;
  bool fse_coded = false;
  int bits = 0;
  switch (huf_read_description(p, n, e->huf, kHufCap, &bits, &used, &fse_coded, &w)) {
    case kHufOk: break;
    case kHufTruncated: fail("truncated Huffman tree");
    case kHufBadWeights: fail("bad Huffman weights");
    default: fail("Huffman weights do not complete a tree");
  }
  e->huf_bits = bits;
  if (st) ++st->weights[fse_coded];
  return used;
}

void huf_stream(const Entropy& e, const uint8_t* p, size_t n, uint8_t* dst, size_t count) {
  int64_t bit = back_start(p, n);
  if (bit < 0) fail("bad Huffman stream");
  const uint32_t mask = (1u << e.huf_bits) - 1;
  for (size_t i = 0; i < count; ++i) {
    if (bit <= 0) fail("Huffman stream ends early");
    const uint32_t ent = e.huf[back_bits(p, n, bit, e.huf_bits) & mask];
    dst[i] = (uint8_t)ent;
    bit -= ent >> 8;
  }
  if (bit != 0) fail("Huffman stream not used up");
}

// One of the three sequence tables, by its mode; returns the bytes of the section it took.
size_t seq_table(int mode, uint32_t* table, int cap, int* log, int max_log, int max_sym, int which, const uint8_t* p, size_t n) {
  int16_t norm[kMaxSyms];
  uint16_t work[kMaxSyms];
  int nsym = 0, alog = 0;
  switch (mode) {
    case 0:
      nsym = which == 0 ? predefined_ll(norm, &alog) : which == 1 ? predefined_of(norm, &alog) : predefined_ml(norm, &alog);
      if (!fse_build(norm, nsym, alog, table, cap, work)) fail("predefined table");
      *log = alog;
      return 0;
    case 1:
      if (n < 1) fail("truncated RLE table");
      if (p[0] > max_sym) fail("RLE symbol out of range");
      fse_build_rle(p[0], table);
      *log = 0;
      return 1;
    case 2: {
      size_t used = 0;
      if (!fse_read_description(p, n, max_log, max_sym, norm, &nsym, &alog, &used)) fail("bad FSE table description");
      if (!fse_build(norm, nsym, alog, table, cap, work)) fail("bad FSE table");
      *log = alog;
      return used;
    }
    default:
      if (*log < 0) fail("Repeat mode with no earlier table");
      return 0;
  }
}

// A compressed block src[0, n): writes at out[op..), never past out[cap); the frame's output so far is
// out[hist, op). max_off: the largest offset taken (the incremental decoder keeps Window_Size bytes of history and
// no more, so it refuses what reaches further; the one-shot decoder has the whole output and passes no limit).
// Returns the new op.
size_t decode_compressed(Entropy* e, const uint8_t* src, size_t n, uint8_t* out, size_t op, size_t cap, size_t hist,
                         size_t block_max, size_t max_off, ZstdStats* st) {
  // ---- literals section
  if (n < 1) fail("truncated literals header");
  const uint32_t type = src[0] & 3, sf = (src[0] >> 2) & 3;
  size_t hdr, regen, comp = 0;
  int streams = 1;
  if (type < 2) {
    hdr = sf == 1 ? 2 : sf == 3 ? 3 : 1;
    if (n < hdr) fail("truncated literals header");
    regen = hdr == 1 ? src[0] >> 3 : hdr == 2 ? le16(src) >> 4 : le24(src) >> 4;
  } else {
    hdr = sf < 2 ? 3 : sf == 2 ? 4 : 5;
    if (n < hdr) fail("truncated literals header");
    const int b = sf < 2 ? 10 : sf == 2 ? 14 : 18;
    const uint64_t v = (hdr == 3 ? le24(src) : hdr == 4 ? le32(src) : (uint64_t)le32(src) | ((uint64_t)src[4] << 32)) >> 4;
    regen = (size_t)(v & ((1u << b) - 1));
    comp = (size_t)((v >> b) & ((1u << b) - 1));
    streams = sf == 0 ? 1 : 4;
  }
  if (regen > kBlockMax) fail("literals section larger than a block");
  if (st) ++st->literals[type];
  const uint8_t* lit;
  size_t pos = hdr;
  if (type == 0) {
    if (n - pos < regen) fail("truncated raw literals");
    lit = src + pos;
    pos += regen;
  } else if (type == 1) {
    if (n - pos < 1) fail("truncated RLE literals");
    e->lit.assign(regen, src[pos]);
    lit = e->lit.data();
    pos += 1;
  } else {
    if (n - pos < comp) fail("truncated compressed literals");
    const uint8_t* p = src + pos;
    size_t left = comp;
    if (type == 2) {
      const size_t used = read_huf_table(e, p, left, st);
      p += used;
      left -= used;
    } else if (e->huf_bits == 0) {
      fail("Treeless literals with no earlier table");
    }
    e->lit.resize(regen);
    if (st) ++st->huf_streams[streams == 4];
    if (streams == 1) {
      huf_stream(*e, p, left, e->lit.data(), regen);
    } else {
      if (left < 6) fail("truncated literals jump table");
      const size_t s1 = le16(p), s2 = le16(p + 2), s3 = le16(p + 4);
      if (6 + s1 + s2 + s3 > left) fail("literal streams longer than their section");
      const size_t s4 = left - 6 - s1 - s2 - s3, seg = (regen + 3) / 4;
      if (3 * seg > regen) fail("literal streams larger than the section's size");
      uint8_t* d = e->lit.data();
      huf_stream(*e, p + 6, s1, d, seg);
      huf_stream(*e, p + 6 + s1, s2, d + seg, seg);
      huf_stream(*e, p + 6 + s1 + s2, s3, d + 2 * seg, seg);
      huf_stream(*e, p + 6 + s1 + s2 + s3, s4, d + 3 * seg, regen - 3 * seg);
    }
    lit = e->lit.data();
    pos += comp;
  }
  // ---- sequences section
  if (n - pos < 1) fail("truncated sequences header");
  size_t nseq = src[pos++];
  if (nseq >= 128) {
    if (nseq == 255) {
      if (n - pos < 2) fail("truncated sequences header");
      nseq = le16(src + pos) + 0x7F00;
      pos += 2;
    } else {
      if (n - pos < 1) fail("truncated sequences header");
      nseq = ((nseq - 128) << 8) + src[pos++];
    }
  }
  const size_t limit = std::min(cap, op + block_max);  // a block regenerates at most Block_Maximum_Size bytes
  size_t lp = 0;
  if (nseq > 0) {
    if (n - pos < 1) fail("truncated sequences header");
    const uint32_t modes = src[pos++];
    if (st) {
      ++st->modes[0][modes >> 6];
      ++st->modes[1][(modes >> 4) & 3];
      ++st->modes[2][(modes >> 2) & 3];
      st->sequences += (int64_t)nseq;
    }
    pos += seq_table((int)(modes >> 6), e->ll, kLlCap, &e->ll_log, kLlMaxLog, kLlMaxSym, 0, src + pos, n - pos);
    pos += seq_table((int)((modes >> 4) & 3), e->of, kOfCap, &e->of_log, kOfMaxLog, kOfMaxSym, 1, src + pos, n - pos);
    pos += seq_table((int)((modes >> 2) & 3), e->ml, kMlCap, &e->ml_log, kMlMaxLog, kMlMaxSym, 2, src + pos, n - pos);
    const uint8_t* b = src + pos;
    const size_t bn = n - pos;
    int64_t bit = back_start(b, bn);
    if (bit < 0) fail("bad sequence bitstream");
    const uint32_t llm = (1u << e->ll_log) - 1, ofm = (1u << e->of_log) - 1, mlm = (1u << e->ml_log) - 1;
    uint32_t sl = (uint32_t)back_bits(b, bn, bit, e->ll_log);
    bit -= e->ll_log;
    uint32_t so = (uint32_t)back_bits(b, bn, bit, e->of_log);
    bit -= e->of_log;
    uint32_t sm = (uint32_t)back_bits(b, bn, bit, e->ml_log);
    bit -= e->ml_log;
    if (bit < 0) fail("sequence bitstream ends early");
    for (size_t i = 0; i < nseq; ++i) {
      const uint32_t el = e->ll[sl & llm], eo = e->of[so & ofm], em = e->ml[sm & mlm];
      const uint32_t oc = fse_sym(eo), lc = fse_sym(el), mc = fse_sym(em);
      if (oc > (uint32_t)kOfMaxSym || lc > (uint32_t)kLlMaxSym || mc > (uint32_t)kMlMaxSym) fail("sequence code out of range");
      const uint32_t ov = (1u << oc) + (uint32_t)back_bits(b, bn, bit, (int)oc);
      bit -= oc;
      const uint32_t mlen = ml_base(mc) + (uint32_t)back_bits(b, bn, bit, (int)ml_bits(mc));
      bit -= ml_bits(mc);
      const uint32_t llen = ll_base(lc) + (uint32_t)back_bits(b, bn, bit, (int)ll_bits(lc));
      bit -= ll_bits(lc);
      if (i + 1 < nseq) {
        sl = fse_base(el) + (uint32_t)back_bits(b, bn, bit, (int)fse_nbits(el));
        bit -= fse_nbits(el);
        sm = fse_base(em) + (uint32_t)back_bits(b, bn, bit, (int)fse_nbits(em));
        bit -= fse_nbits(em);
        so = fse_base(eo) + (uint32_t)back_bits(b, bn, bit, (int)fse_nbits(eo));
        bit -= fse_nbits(eo);
      }
      if (bit < 0) fail("sequence bitstream ends early");
      if (llen > regen - lp) fail("sequence takes more literals than the block has");
      if ((size_t)llen + mlen > limit - op) fail("block regenerates more than its limit");
      copy(out + op, lit + lp, llen);
      op += llen;
      lp += llen;
      const uint32_t off = apply_offset(ov, llen, e->rep);
      if (off > max_off) fail("offset beyond Window_Size");  // (first: what lies further back may be slid away)
      if (off > op - hist) fail("offset reaches before the frame's first byte");
      if (st && off > st->max_offset) st->max_offset = off;
      const uint8_t* from = out + op - off;
      if (off >= mlen) {
        std::memcpy(out + op, from, mlen);
      } else {
        for (uint32_t k = 0; k < mlen; ++k) out[op + k] = from[k];
      }
      op += mlen;
    }
    if (bit != 0) fail("sequence bitstream not used up");
  } else if (pos != n) {
    fail("bytes behind an empty sequences section");
  }
  if (regen - lp > limit - op) fail("block regenerates more than its limit");
  copy(out + op, lit + lp, regen - lp);
  return op + (regen - lp);
}

struct FrameHeader {
  uint64_t window = 0, fcs = 0;
  bool has_fcs = false, has_sum = false;
};
// 0: the header at p[0, n) (behind the magic) is not whole yet; otherwise its length.
size_t parse_frame_header(const uint8_t* p, size_t n, FrameHeader* h) {
  if (n < 1) return 0;
  const uint32_t d = p[0];
  if (d & 0x08) fail("reserved descriptor bit");
  const bool single = d & 0x20;
  const int did = (int)(d & 3), fcsf = (int)(d >> 6);
  const size_t did_n = did == 3 ? 4 : (size_t)did, fcs_n = fcsf == 0 ? (single ? 1 : 0) : (size_t)1 << fcsf;
  const size_t len = 1 + (single ? 0 : 1) + did_n + fcs_n;
  if (n < len) return 0;
  size_t at = 1;
  if (!single) {
    const uint32_t w = p[at++];
    const uint64_t base = 1ull << (10 + (w >> 3));
    h->window = base + (base >> 3) * (w & 7);
  }
  uint32_t dict = 0;
  for (size_t i = 0; i < did_n; ++i) dict |= (uint32_t)p[at + i] << (8 * i);
  at += did_n;
  if (dict != 0) fail("needs a dictionary");
  h->has_fcs = fcs_n > 0;
  h->fcs = 0;
  for (size_t i = 0; i < fcs_n; ++i) h->fcs |= (uint64_t)p[at + i] << (8 * i);
  if (fcs_n == 2) h->fcs += 256;
  if (single) h->window = h->fcs;
  h->has_sum = d & 0x04;
  return len;
}
}  // namespace

bool zstd_decompress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len, size_t* consumed,
                     ZstdStats* st, std::string* why) {
  *out_len = 0;
  if (consumed) *consumed = 0;
  try {
    auto e = std::make_unique<Entropy>();
    size_t pos = 0, op = 0;
    int64_t seen = 0;
    for (;;) {
      if (n - pos < 4) {
        if (!seen) fail("truncated");
        break;
      }
      const uint32_t magic = le32(src + pos);
      if ((magic & 0xFFFFFFF0u) == kSkipMagic) {
        if (n - pos < 8) fail("truncated skippable frame");
        const uint64_t len = le32(src + pos + 4);
        if (len > n - pos - 8) fail("truncated skippable frame");
        pos += 8 + (size_t)len;
        ++seen;
        if (st) ++st->skippable;
        continue;
      }
      if (magic != kMagic) {
        if (!seen) fail("wrong magic");
        break;
      }
      FrameHeader h;
      const size_t hl = parse_frame_header(src + pos + 4, n - pos - 4, &h);
      if (!hl) fail("truncated frame header");
      pos += 4 + hl;
      ++seen;
      e->reset();
      const size_t fstart = op;
      const size_t block_max = (size_t)std::min<uint64_t>(h.window, kBlockMax);
      int64_t blocks = 0;
      for (bool last = false; !last;) {
        if (n - pos < 3) fail("truncated block header");
        const uint32_t bh = le24(src + pos);
        pos += 3;
        last = bh & 1;
        const uint32_t type = (bh >> 1) & 3, size = bh >> 3;
        if (type == 3) fail("reserved block type");
        if (size > block_max) fail("block larger than min(window, 128 KiB)");
        ++blocks;
        if (st) ++st->blocks[type];
        if (type == 0) {
          if (n - pos < size) fail("truncated raw block");
          if (size > cap - op) fail("more output than expected");
          copy(dst + op, src + pos, size);
          op += size;
          pos += size;
        } else if (type == 1) {
          if (n - pos < 1) fail("truncated RLE block");
          if (size > cap - op) fail("more output than expected");
          fill(dst + op, src[pos], size);
          op += size;
          pos += 1;
        } else {
          if (n - pos < size) fail("truncated compressed block");
          op = decode_compressed(e.get(), src + pos, size, dst, op, cap, fstart, block_max, SIZE_MAX, st);
          pos += size;
        }
      }
      if (st) {
        ++st->frames;
        st->max_frame_blocks = std::max(st->max_frame_blocks, blocks);
      }
      if (h.has_fcs && h.fcs != op - fstart) fail("content size does not match");
      if (h.has_sum) {
        if (n - pos < 4) fail("truncated content checksum");
        Xxh64 x;
        x.update(dst + fstart, op - fstart);
        if ((uint32_t)x.digest() != le32(src + pos)) fail("content checksum mismatch");
        pos += 4;
        if (st) ++st->checksums;
      }
    }
    *out_len = op;
    if (consumed) *consumed = pos;
    return true;
  } catch (const UdaError& err) {
    if (why) *why = err.what();
    return false;
  }
}

// ---- incremental
struct ZstdDecoder::Tables {
  Entropy e;
  Xxh64 sum;
};

ZstdDecoder::ZstdDecoder() : t_(std::make_unique<Tables>()) {}
ZstdDecoder::~ZstdDecoder() = default;

// What is consumed is dropped at every feed and the vector grows in 4 KiB steps, not by doubling: with a caller
// that reads between feeds it holds one block's input, its header and the piece fed, and no more.
void ZstdDecoder::feed(const uint8_t* p, size_t n) {
  if (ipos_ > 0) {
    in_.erase(in_.begin(), in_.begin() + (long)ipos_);
    dropped_ += ipos_;
    ipos_ = 0;
  }
  if (in_.size() + n > in_.capacity()) in_.reserve((in_.size() + n + 4095) & ~(size_t)4095);
  in_.insert(in_.end(), p, p + n);
}

size_t ZstdDecoder::read(uint8_t* dst, size_t cap) {
  size_t got = 0;
  for (;;) {
    const size_t n = std::min(cap - got, wpos_ - rpos_);
    copy(dst + got, buf_.data() + rpos_, n);
    rpos_ += n;
    got += n;
    if (rpos_ < wpos_) return got;
    // all read: decode ahead, so finished() is current when the last bytes are handed out
    if (!run()) return got;  // needs input (or just ended)
    if (got == cap) return got;
  }
}

// Decodes units until a block has produced output (true), the input runs out or the last frame ends.
bool ZstdDecoder::run() {
  for (;;) {
    const uint8_t* p = in_.data() + ipos_;
    const size_t avail = in_.size() - ipos_;
    if (skip_) {
      const size_t k = (size_t)std::min<uint64_t>(skip_, avail);
      ipos_ += k;
      skip_ -= k;
      if (skip_) return false;
      continue;
    }
    switch (state_) {
      case kDone:  // another frame begins only if its magic is there
        if (avail < 4 || (le32(p) != kMagic && (le32(p) & 0xFFFFFFF0u) != kSkipMagic)) return false;
        state_ = kFrame;
        break;
      case kFrame: {
        if (avail < 4) return false;
        const uint32_t magic = le32(p);
        if ((magic & 0xFFFFFFF0u) == kSkipMagic) {
          if (avail < 8) return false;
          skip_ = le32(p + 4);
          ipos_ += 8;
          if (any_frame_) state_ = kDone;  // (behind a frame: finished again once it is skipped)
          break;
        }
        if (magic != kMagic) fail("wrong magic");
        FrameHeader h;
        const size_t hl = parse_frame_header(p + 4, avail - 4, &h);
        if (!hl) return false;
        if (h.window > kWindowMax) fail("Window_Size above 128 MiB");
        ipos_ += 4 + hl;
        window_ = h.window;
        fcs_ = h.fcs;
        has_fcs_ = h.has_fcs;
        has_sum_ = h.has_sum;
        frame_out_ = 0;
        fstart_ = wpos_;
        t_->e.reset();
        t_->sum = Xxh64();
        any_frame_ = true;
        state_ = kBlock;
        break;
      }
      case kBlock: {
        if (avail < 3) return false;
        const uint32_t bh = le24(p), type = (bh >> 1) & 3, size = bh >> 3;
        if (type == 3) fail("reserved block type");
        const size_t block_max = (size_t)std::min<uint64_t>(window_, kBlockMax);
        if (size > block_max) fail("block larger than min(window, 128 KiB)");
        const size_t csize = type == 1 ? 1 : size;
        if (avail < 3 + csize) return false;
        // room for one block's output (everything decoded was read: this runs only then)
        if (wpos_ + block_max > buf_.size()) {
          const size_t most = (size_t)window_ + block_max;  // Window_Size of history and one block
          if (wpos_ + block_max <= most) {
            const size_t to = std::min(most, std::max(2 * buf_.size(), wpos_ + block_max));
            buf_.reserve(to);  // (exactly: resize alone may double the capacity past `most`)
            buf_.resize(to);
          } else {  // keep the last Window_Size bytes as history at the buffer's start
            const size_t keep = std::min<size_t>((size_t)window_, wpos_), shift = wpos_ - keep;
            if (keep) std::memmove(buf_.data(), buf_.data() + shift, keep);
            fstart_ = fstart_ > shift ? fstart_ - shift : 0;
            wpos_ = rpos_ = keep;
            if (wpos_ + block_max > buf_.size()) {
              buf_.reserve(wpos_ + block_max);
              buf_.resize(wpos_ + block_max);
            }
          }
        }
        const size_t was = wpos_;
        if (type == 0) {
          copy(buf_.data() + wpos_, p + 3, size);
          wpos_ += size;
        } else if (type == 1) {
          fill(buf_.data() + wpos_, p[3], size);
          wpos_ += size;
        } else {
          wpos_ = decode_compressed(&t_->e, p + 3, size, buf_.data(), wpos_, buf_.size(), fstart_, block_max, (size_t)window_, nullptr);
        }
        ipos_ += 3 + csize;
        frame_out_ += wpos_ - was;
        if (has_sum_) t_->sum.update(buf_.data() + was, wpos_ - was);
        if (bh & 1) {
          if (has_fcs_ && fcs_ != frame_out_) fail("content size does not match");
          state_ = has_sum_ ? kChecksum : kDone;
        }
        if (wpos_ > was) return true;
        break;  // an empty block: nothing for read() to hand out, so go on
      }
      case kChecksum:
        if (avail < 4) return false;
        if ((uint32_t)t_->sum.digest() != le32(p)) fail("content checksum mismatch");
        ipos_ += 4;
        state_ = kDone;
        break;
    }
  }
}

// ---- encoder
namespace {
struct BitWriter {
  uint8_t* p;
  size_t n = 0;
  uint64_t acc = 0;
  int cnt = 0;
  void put(uint32_t v, int nb) {  // nb <= 32
    if (!nb) return;
    acc |= (uint64_t)(v & (nb == 32 ? 0xFFFFFFFFu : (1u << nb) - 1)) << cnt;
    cnt += nb;
    while (cnt >= 8) {
      p[n++] = (uint8_t)acc;
      acc >>= 8;
      cnt -= 8;
    }
  }
  size_t finish() {  // the closing 1 bit and padding
    put(1, 1);
    if (cnt) {
      p[n++] = (uint8_t)acc;
      acc = 0;
      cnt = 0;
    }
    return n;
  }
};

// The predefined tables with, for every symbol and every next state, the state to come from.
struct PredefEnc {
  uint32_t ll[64], of[32], ml[64];
  uint8_t ll_from[36][64], of_from[29][32], ml_from[53][64];
  uint8_t ll_any[36], of_any[29], ml_any[53];
  PredefEnc() {
    int16_t norm[kMaxSyms];
    uint16_t work[kMaxSyms];
    int alog;
    int ns = predefined_ll(norm, &alog);
    fse_build(norm, ns, alog, ll, 64, work);
    fill(ll, 64, &ll_from[0][0], 64, ll_any);
    ns = predefined_of(norm, &alog);
    fse_build(norm, ns, alog, of, 32, work);
    fill(of, 32, &of_from[0][0], 32, of_any);
    ns = predefined_ml(norm, &alog);
    fse_build(norm, ns, alog, ml, 64, work);
    fill(ml, 64, &ml_from[0][0], 64, ml_any);
  }
  static void fill(const uint32_t* t, int size, uint8_t* from, int stride, uint8_t* any) {
    for (int s = 0; s < size; ++s) {
      const uint32_t sym = fse_sym(t[s]), base = fse_base(t[s]), span = 1u << fse_nbits(t[s]);
      any[sym] = (uint8_t)s;
      for (uint32_t k = 0; k < span; ++k) from[sym * stride + base + k] = (uint8_t)s;
    }
  }
};
const PredefEnc& predef() {
  static const PredefEnc p;
  return p;
}

struct Seq {
  uint32_t ll, ml, ov;  // literal length, match length, Offset_Value
};
inline uint32_t ll_code(uint32_t v) {
  uint32_t c = v < 16 ? v : 16;
  while (c < 35 && ll_base(c + 1) <= v) ++c;
  return c;
}
inline uint32_t ml_code(uint32_t v) {
  uint32_t c = v < 35 ? v - 3 : 32;
  while (c < 52 && ml_base(c + 1) <= v) ++c;
  return c;
}
inline void put_le24(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
  p[2] = (uint8_t)(v >> 16);
}

// The compressed form of a block (literals, sequences) in *buf; returns its length.
size_t write_compressed(const std::vector<uint8_t>& lits, const std::vector<Seq>& seqs, std::vector<uint8_t>* buf) {
  const size_t nl = lits.size(), ns = seqs.size();
  // worst case: header 3, literals, count 3, modes 1, 3 states + per sequence at most 16+16+28 extra and 6+6+5 state bits
  buf->resize(3 + nl + 4 + (ns * 80 + 32) / 8 + 1);
  uint8_t* const dst = buf->data();
  size_t at = 0;
  if (nl < 32) {
    dst[at++] = (uint8_t)(nl << 3);
  } else if (nl < 4096) {
    dst[at++] = (uint8_t)(0x04 | (nl << 4));
    dst[at++] = (uint8_t)(nl >> 4);
  } else {
    put_le24(dst + at, (uint32_t)(0x0C | (nl << 4)));
    at += 3;
  }
  if (nl) std::memcpy(dst + at, lits.data(), nl);
  at += nl;
  if (ns < 128) {
    dst[at++] = (uint8_t)ns;
  } else if (ns < 0x7F00) {
    dst[at++] = (uint8_t)(128 + (ns >> 8));
    dst[at++] = (uint8_t)ns;
  } else {
    dst[at++] = 255;
    dst[at++] = (uint8_t)(ns - 0x7F00);
    dst[at++] = (uint8_t)((ns - 0x7F00) >> 8);
  }
  if (ns == 0) return at;
  dst[at++] = 0;  // Predefined, Predefined, Predefined
  const PredefEnc& t = predef();
  BitWriter w{dst + at};
  uint32_t sl = 0, so = 0, sm = 0;
  for (size_t i = ns; i-- > 0;) {
    const Seq& q = seqs[i];
    const uint32_t lc = ll_code(q.ll), mc = ml_code(q.ml), oc = (uint32_t)highbit(q.ov);
    if (i + 1 == ns) {
      sl = t.ll_any[lc];
      so = t.of_any[oc];
      sm = t.ml_any[mc];
    } else {  // the decoder goes from this sequence's states to the next one's: LL, ML, OF, so written OF, ML, LL
      const uint32_t pl = t.ll_from[lc][sl], po = t.of_from[oc][so], pm = t.ml_from[mc][sm];
      w.put(so - fse_base(t.of[po]), (int)fse_nbits(t.of[po]));
      w.put(sm - fse_base(t.ml[pm]), (int)fse_nbits(t.ml[pm]));
      w.put(sl - fse_base(t.ll[pl]), (int)fse_nbits(t.ll[pl]));
      sl = pl;
      so = po;
      sm = pm;
    }
    w.put(q.ll - ll_base(lc), (int)ll_bits(lc));
    w.put(q.ml - ml_base(mc), (int)ml_bits(mc));
    w.put(q.ov - (1u << oc), (int)oc);
  }
  w.put(sm, 6);
  w.put(so, 5);
  w.put(sl, 6);
  return at + w.finish();
}
}  // namespace

size_t zstd_max_compressed_length(size_t n) { return n + 3 * (n / kBlockMax + 1) + 16; }

size_t zstd_compress(const uint8_t* src, size_t n, uint8_t* dst) {
  size_t at = 0;
  dst[at++] = 0x28;
  dst[at++] = 0xB5;
  dst[at++] = 0x2F;
  dst[at++] = 0xFD;
  dst[at++] = 0;  // no content size, no checksum, no dictionary: a Window_Descriptor follows
  int wlog = 10;
  while (wlog < 22 && ((size_t)1 << wlog) < n) ++wlog;
  dst[at++] = (uint8_t)((wlog - 10) << 3);
  const size_t window = (size_t)1 << wlog;
  constexpr int kHashLog = 16, kDepth = 16;
  constexpr uint32_t kMinMatch = 4, kMaxMatch = 65535 + 3;
  std::vector<int32_t> head((size_t)1 << kHashLog, -1), prev(n < (1u << 31) ? n : 0, -1);
  auto hash = [&](size_t i) {
    uint32_t v;
    std::memcpy(&v, src + i, 4);
    return (v * 2654435761u) >> (32 - kHashLog);
  };
  const bool match_ok = n < (1u << 31);  // (positions are 32-bit; beyond that the blocks go out Raw)
  std::vector<uint8_t> lits, tmp;
  std::vector<Seq> seqs;
  uint32_t rep[3] = {1, 4, 8};
  size_t inserted = 0;
  auto insert_to = [&](size_t end) {  // positions [inserted, end) enter the chains
    for (; inserted < end && inserted + 4 <= n; ++inserted) {
      const uint32_t h = hash(inserted);
      prev[inserted] = head[h];
      head[h] = (int32_t)inserted;
    }
  };
  size_t off = 0;
  do {
    const size_t len = std::min<size_t>(kBlockMax, n - off), end = off + len;
    const bool last = end == n;
    bool rle = len > 0;
    for (size_t i = 1; i < len && rle; ++i) rle = src[off + i] == src[off];
    if (rle && len > 1) {
      put_le24(dst + at, (uint32_t)((len << 3) | 2 | (last ? 1 : 0)));
      dst[at + 3] = src[off];
      at += 4;
      off = end;
      continue;
    }
    lits.clear();
    seqs.clear();
    uint32_t brep[3] = {rep[0], rep[1], rep[2]};
    size_t i = off, anchor = off;
    while (match_ok && i + kMinMatch <= end) {
      insert_to(i);
      size_t best = 0, best_from = 0;
      int depth = kDepth;
      // the most recent offset first: it costs no offset bits
      if (i - anchor > 0 && brep[0] <= i && std::memcmp(src + i, src + i - brep[0], 4) == 0) {
        size_t m = 4;
        while (i + m < end && src[i + m] == src[i - brep[0] + m]) ++m;
        best = m;
        best_from = i - brep[0];
      }
      for (int32_t c = head[hash(i)]; c >= 0 && depth-- > 0 && i - (size_t)c <= window; c = prev[(size_t)c]) {
        size_t m = 0;
        while (i + m < end && src[(size_t)c + m] == src[i + m]) ++m;
        if (m > best && m >= kMinMatch) {
          best = m;
          best_from = (size_t)c;
        }
      }
      if (best < kMinMatch) {
        ++i;
        continue;
      }
      best = std::min<size_t>(best, kMaxMatch);
      const uint32_t ll = (uint32_t)(i - anchor), d = (uint32_t)(i - best_from);
      uint32_t ov = d + 3;
      if (ll > 0 && d == brep[0]) ov = 1;
      else if (ll == 0 && d == brep[1]) ov = 1;
      else if (ll > 0 && d == brep[1]) ov = 2;
      (void)apply_offset(ov, ll, brep);
      lits.insert(lits.end(), src + anchor, src + i);
      seqs.push_back(Seq{ll, (uint32_t)best, ov});
      i += best;
      anchor = i;
    }
    lits.insert(lits.end(), src + anchor, src + end);
    const size_t c = seqs.empty() ? 0 : write_compressed(lits, seqs, &tmp);
    if (c > 0 && c < len) {
      put_le24(dst + at, (uint32_t)((c << 3) | 4 | (last ? 1 : 0)));
      std::memcpy(dst + at + 3, tmp.data(), c);
      at += 3 + c;
      rep[0] = brep[0];
      rep[1] = brep[1];
      rep[2] = brep[2];
    } else {  // a Raw block leaves the repeat offsets as they were
      put_le24(dst + at, (uint32_t)((len << 3) | (last ? 1 : 0)));
      copy(dst + at + 3, src + off, len);
      at += 3 + len;
    }
    off = end;
  } while (off < n);
  return at;
}

}  // namespace uda
