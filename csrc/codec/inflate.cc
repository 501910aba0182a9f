// Host zlib / deflate decoder (RFC 1950 / 1951) for DefaultCodec map outputs, and in its gzip mode (RFC 1952
// members around the same deflate data) for GzipCodec ones. See uda/codec.h.
//
// One state machine serves the one-shot call and the incremental Inflater. A unit (block header, symbol
// with its extra bits, stored chunk, trailer) is parsed from a local bit position and committed only when
// all of its bits were there; otherwise run() returns and the unit is parsed again after the next feed.
// Bits past the input's end read as zeros and are never acted on: every field is checked against the bits
// that are really there before it is used, so "needs input" always wins over "corrupt".
// A gzip member's header (with its optional fields) and its 8-byte trailer are units of the same kind: parsed
// from the bytes that are there, committed only when whole.
#include <algorithm>
#include <cstring>

#include "inflate_tables.h"
#include "uda/codec.h"
#include "uda/error.h"

namespace uda {

namespace {
constexpr size_t kHistory = 32768;
constexpr size_t kOutBuf = 65536;
constexpr size_t kMaxMatch = 258;

// 57 or more bits at bit position pos of p[0, n), zeros past the end.
inline uint64_t peek_bits(const uint8_t* p, size_t n, uint64_t pos) {
  const size_t byte = (size_t)(pos >> 3);
  uint64_t w = 0;
  if (byte + 8 <= n) {
    std::memcpy(&w, p + byte, 8);  // little-endian hosts only, as the rest of the tree
  } else {
    for (size_t k = 0; byte + k < n && k < 8; ++k) w |= (uint64_t)p[byte + k] << (8 * k);
  }
  return w >> (pos & 7);
}
inline uint32_t mask(uint32_t n) { return (1u << n) - 1; }

// CRC-32 (IEEE, reflected) with a table of this file's own: the stand-alone sanitizer programs build this file alone.
struct CrcTable {
  uint32_t t[256];
  constexpr CrcTable() : t() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1)));
      t[i] = c;
    }
  }
};
constexpr CrcTable kCrc;
inline uint32_t crc32_update(uint32_t crc, const uint8_t* p, size_t n) {
  uint32_t c = ~crc;
  for (size_t i = 0; i < n; ++i) c = kCrc.t[(c ^ p[i]) & 0xFF] ^ (c >> 8);
  return ~c;
}
inline uint32_t le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

constexpr size_t kGzipMinMember = 18;  // a 10-byte header and the 8-byte trailer: no member is shorter
// FLG bits (RFC 1952)
constexpr uint32_t kFhcrc = 2, kFextra = 4, kFname = 8, kFcomment = 16, kFlgReserved = 0xE0;

// Another member starts at p[0, n): enough bytes for the smallest header and trailer, and the magic with CM.
inline bool gzip_member_starts(const uint8_t* p, size_t n) {
  return n >= kGzipMinMember && p[0] == 0x1f && p[1] == 0x8b && p[2] == 8;
}
}  // namespace

Inflater::Inflater(Container c)
    : buf_(kHistory + kOutBuf), gzip_(c == Container::kGzip), lit_(inflate::kLitCap), dist_(inflate::kDistCap) {}

void Inflater::fail(const char* what) const {
  throw UdaError(std::string(gzip_ ? "corrupt gzip stream: " : "corrupt zlib stream: ") + what);
}

// gzip, behind a member's trailer: go on into the next member if one starts in the input that is there.
bool Inflater::next_member() {
  const size_t byte = (size_t)((bitpos_ + 7) >> 3);
  if (byte > in_.size() || !gzip_member_starts(in_.data() + byte, in_.size() - byte)) return false;
  crc_ = 0;
  member_out_ = total_out_;
  state_ = kHeader;
  return true;
}

// 0 = the gzip header at p[0, n) is not whole yet; otherwise its length. Fails on what zlib refuses.
size_t Inflater::gzip_header(const uint8_t* p, size_t n) const {
  if (n < 10) return 0;
  if (p[0] != 0x1f || p[1] != 0x8b) fail("incorrect header check");
  if (p[2] != 8) fail("unknown compression method");
  const uint32_t flg = p[3];
  if (flg & kFlgReserved) fail("unknown header flags set");
  size_t at = 10;  // MTIME, XFL and OS are ignored (and FTEXT)
  if (flg & kFextra) {
    if (n - at < 2) return 0;
    const size_t xlen = (size_t)p[at] | ((size_t)p[at + 1] << 8);
    at += 2;
    if (n - at < xlen) return 0;
    at += xlen;
  }
  for (const uint32_t bit : {kFname, kFcomment}) {
    if (!(flg & bit)) continue;
    const void* z = std::memchr(p + at, 0, n - at);
    if (!z) return 0;
    at = (size_t)((const uint8_t*)z - p) + 1;
  }
  if (flg & kFhcrc) {
    if (n - at < 2) return 0;
    const uint32_t stored = (uint32_t)p[at] | ((uint32_t)p[at + 1] << 8);
    if (stored != (crc32_update(0, p, at) & 0xFFFF)) fail("header crc mismatch");
    at += 2;
  }
  return at;
}

void Inflater::feed(const uint8_t* p, size_t n) {
  const size_t done = (size_t)(bitpos_ >> 3);
  if (done > 0 && (done == in_.size() || done > (1u << 16))) {
    in_.erase(in_.begin(), in_.begin() + (long)done);
    dropped_ += done;
    bitpos_ -= (uint64_t)done * 8;
  }
  in_.insert(in_.end(), p, p + n);
}

void Inflater::sum() {
  if (gzip_) {  // its check over the same bytes is a CRC-32
    crc_ = crc32_update(crc_, buf_.data() + spos_, wpos_ - spos_);
    spos_ = wpos_;
    return;
  }
  uint32_t a = adler_a_, b = adler_b_;
  while (spos_ < wpos_) {
    const size_t n = std::min<size_t>(5552, wpos_ - spos_);  // the most bytes before b can overflow 32 bits
    for (size_t i = 0; i < n; ++i) {
      a += buf_[spos_ + i];
      b += a;
    }
    a %= inflate::kAdlerMod;
    b %= inflate::kAdlerMod;
    spos_ += n;
  }
  adler_a_ = a;
  adler_b_ = b;
}

// Everything was read: keep the last 32 KiB as history at the buffer's start.
void Inflater::slide() {
  sum();
  if (wpos_ <= kHistory) return;
  std::memmove(buf_.data(), buf_.data() + (wpos_ - kHistory), kHistory);
  wpos_ = rpos_ = spos_ = kHistory;
}

size_t Inflater::read(uint8_t* dst, size_t cap) {
  size_t got = 0;
  for (;;) {
    const size_t n = std::min(cap - got, wpos_ - rpos_);
    if (n) std::memcpy(dst + got, buf_.data() + rpos_, n);
    rpos_ += n;
    got += n;
    if (rpos_ < wpos_) return got;  // cap reached with output left
    // all read: decode ahead, so finished() is current when the last bytes are handed out
    if (state_ == kDone && !(gzip_ && next_member())) return got;
    if (wpos_ + kMaxMatch > buf_.size()) slide();
    const size_t before = wpos_;
    run();
    if (wpos_ == before) return got;  // needs input (or just ended)
    if (got == cap) return got;
  }
}

void Inflater::run() {
  using namespace inflate;
  const uint8_t* const in = in_.data();
  const size_t n = in_.size();
  const uint64_t nbits = (uint64_t)n * 8;
  uint8_t* const out = buf_.data();
  const size_t out_cap = buf_.size();
  for (;;) {
    uint64_t pos = bitpos_;
    switch (state_) {
      case kHeader: {
        if (gzip_) {  // (pos is a byte boundary: the stream's start, or the end of a member's trailer)
          const size_t byte = (size_t)(pos >> 3);
          const size_t len = gzip_header(in + byte, n - byte);
          if (len == 0) return;
          bitpos_ = pos + (uint64_t)len * 8;
          state_ = kBlockHeader;
          break;
        }
        if (nbits - pos < 16) return;
        const uint64_t w = peek_bits(in, n, pos);
        if (!zlib_header_ok((uint32_t)(w & 0xFF), (uint32_t)((w >> 8) & 0xFF))) fail("bad header");
        bitpos_ = pos + 16;
        state_ = kBlockHeader;
        break;
      }
      case kBlockHeader: {
        if (nbits - pos < 3) return;
        uint64_t w = peek_bits(in, n, pos);
        const bool last = w & 1;
        const uint32_t type = (uint32_t)((w >> 1) & 3);
        pos += 3;
        if (type == 3) fail("invalid block type");
        if (type == 0) {
          pos = (pos + 7) & ~(uint64_t)7;
          if (nbits < pos || nbits - pos < 32) return;
          w = peek_bits(in, n, pos);
          const uint32_t len = (uint32_t)(w & 0xFFFF), nlen = (uint32_t)((w >> 16) & 0xFFFF);
          if (len != (nlen ^ 0xFFFF)) fail("invalid stored block lengths");
          stored_left_ = len;
          last_ = last;
          bitpos_ = pos + 32;
          state_ = kStored;
          break;
        }
        uint8_t lens[kMaxLit + kMaxDist];
        uint16_t work[kWork];
        int nlit = kMaxLit, ndist = kMaxDist;
        if (type == 1) {
          fixed_lengths(lens);
        } else {
          if (nbits - pos < 14) return;
          w = peek_bits(in, n, pos);
          nlit = (int)(w & 31) + 257;
          ndist = (int)((w >> 5) & 31) + 1;
          const int ncl = (int)((w >> 10) & 15) + 4;
          pos += 14;
          if (nlit > 286 || ndist > 30) fail("too many length or distance symbols");
          if (nbits - pos < (uint64_t)ncl * 3) return;
          uint8_t cl[kClSyms] = {0};
          for (int i = 0; i < ncl; ++i) {
            cl[cl_order(i)] = (uint8_t)(peek_bits(in, n, pos) & 7);
            pos += 3;
          }
          uint16_t clt[kClCap];
          if (!build_table(cl, kClSyms, kClRoot, false, clt, kClCap, work)) fail("invalid code lengths set");
          int have = 0;
          while (have < nlit + ndist) {
            const uint64_t avail = nbits - pos;
            w = peek_bits(in, n, pos);
            const uint32_t e = lookup(clt, kClRoot, (uint32_t)w);
            const uint32_t bits = e & 15, sym = e >> 4;
            if (bits == 0) {
              if (avail < 7) return;
              fail("invalid code lengths set");  // (no code-length code at all)
            }
            if (bits > avail) return;
            if (sym < 16) {
              lens[have++] = (uint8_t)sym;
              pos += bits;
              continue;
            }
            const uint32_t eb = sym == 16 ? 2 : sym == 17 ? 3 : 7;
            if (bits + eb > avail) return;
            uint32_t rep = (uint32_t)((w >> bits) & mask(eb));
            uint8_t v = 0;
            if (sym == 16) {
              if (have == 0) fail("invalid bit length repeat");
              v = lens[have - 1];
              rep += 3;
            } else {
              rep += sym == 17 ? 3 : 11;
            }
            if (have + (int)rep > nlit + ndist) fail("invalid bit length repeat");
            while (rep--) lens[have++] = v;
            pos += bits + eb;
          }
          if (lens[kEndOfBlock] == 0) fail("invalid code -- missing end-of-block");
          // the distance lengths lie right behind the literal/length ones
        }
        if (!build_table(lens, nlit, kLitRoot, true, lit_.data(), kLitCap, work)) fail("invalid literal/lengths set");
        if (!build_table(lens + nlit, ndist, kDistRoot, true, dist_.data(), kDistCap, work)) fail("invalid distances set");
        last_ = last;
        bitpos_ = pos;
        state_ = kSymbols;
        break;
      }
      case kStored: {
        if (stored_left_ == 0) {
          state_ = last_ ? kAdler : kBlockHeader;
          break;
        }
        const size_t byte = (size_t)(pos >> 3);
        const size_t k = std::min<size_t>({(size_t)stored_left_, n - byte, out_cap - wpos_});
        if (k == 0) return;  // no input, or no room
        std::memcpy(out + wpos_, in + byte, k);
        wpos_ += k;
        total_out_ += k;
        stored_left_ -= (uint32_t)k;
        bitpos_ = pos + (uint64_t)k * 8;
        break;
      }
      case kSymbols: {
        const uint16_t* const lit = lit_.data();
        const uint16_t* const dist = dist_.data();
        for (;;) {
          if (wpos_ + kMaxMatch > out_cap) {
            bitpos_ = pos;
            return;  // output buffer full
          }
          const uint64_t avail = nbits - pos;
          const uint64_t w = peek_bits(in, n, pos);
          uint32_t e = lookup(lit, kLitRoot, (uint32_t)w);
          uint32_t used = e & 15;
          const uint32_t sym = e >> 4;
          if (used == 0) {
            if (avail >= (uint64_t)kMaxBits) fail("invalid literal/length code");
            bitpos_ = pos;
            return;
          }
          if (used > avail) {
            bitpos_ = pos;
            return;
          }
          if (sym < 256) {
            out[wpos_++] = (uint8_t)sym;
            ++total_out_;
            pos += used;
            continue;
          }
          if (sym == (uint32_t)kEndOfBlock) {
            pos += used;
            state_ = last_ ? kAdler : kBlockHeader;
            break;
          }
          if (sym >= 286) fail("invalid literal/length code");
          uint32_t base, eb;
          length_code((int)sym, &base, &eb);
          if (used + eb > avail) {
            bitpos_ = pos;
            return;
          }
          const uint32_t len = base + (uint32_t)((w >> used) & mask(eb));
          used += eb;
          e = lookup(dist, kDistRoot, (uint32_t)(w >> used));
          const uint32_t dbits = e & 15, dsym = e >> 4;
          if (dbits == 0) {
            if (avail - used >= (uint64_t)kMaxBits) fail("invalid distance code");
            bitpos_ = pos;
            return;
          }
          if (used + dbits > avail) {
            bitpos_ = pos;
            return;
          }
          if (dsym >= 30) fail("invalid distance code");
          used += dbits;
          dist_code((int)dsym, &base, &eb);
          if (used + eb > avail) {
            bitpos_ = pos;
            return;
          }
          const uint32_t d = base + (uint32_t)((w >> used) & mask(eb));
          used += eb;
          if ((uint64_t)d > total_out_ - member_out_) fail("invalid distance too far back");
          // (the buffer holds min(total_out_, 32 KiB or more) bytes below wpos_)
          for (uint32_t i = 0; i < len; ++i) out[wpos_ + i] = out[wpos_ + i - d];
          wpos_ += len;
          total_out_ += len;
          pos += used;
        }
        bitpos_ = pos;
        break;
      }
      case kAdler: {
        pos = (pos + 7) & ~(uint64_t)7;
        if (gzip_) {  // CRC-32 and ISIZE, little-endian, taken together
          if (nbits < pos || nbits - pos < 64) return;
          const size_t byte = (size_t)(pos >> 3);
          sum();
          if (le32(in + byte) != crc_) fail("incorrect data check");
          if (le32(in + byte + 4) != (uint32_t)(total_out_ - member_out_)) fail("incorrect length check");
          bitpos_ = pos + 64;
          state_ = kDone;
          break;  // (a member of no output must not read as "needs input" while another follows)
        }
        if (nbits < pos || nbits - pos < 32) return;
        const size_t byte = (size_t)(pos >> 3);
        const uint32_t stored = ((uint32_t)in[byte] << 24) | ((uint32_t)in[byte + 1] << 16) | ((uint32_t)in[byte + 2] << 8) | in[byte + 3];
        sum();
        if (stored != ((adler_b_ << 16) | adler_a_)) fail("Adler-32 mismatch");
        bitpos_ = pos + 32;
        state_ = kDone;
        return;
      }
      case kDone:
        if (gzip_ && next_member()) break;
        return;
    }
  }
}

namespace {
bool one_shot(Inflater::Container c, const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len, size_t* consumed) {
  *out_len = 0;
  if (consumed) *consumed = 0;
  try {
    Inflater inf(c);
    inf.feed(src, n);
    size_t got = 0;
    for (size_t k; got < cap && (k = inf.read(dst + got, cap - got)) > 0;) got += k;
    uint8_t over;
    if (inf.read(&over, 1) != 0) return false;  // more output than cap
    if (!inf.finished()) return false;          // truncated
    *out_len = got;
    if (consumed) *consumed = (size_t)inf.consumed();
    return true;
  } catch (const UdaError&) {
    return false;
  }
}
}  // namespace

bool zlib_decompress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len, size_t* consumed) {
  return one_shot(Inflater::Container::kZlib, src, n, dst, cap, out_len, consumed);
}

bool gzip_decompress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len, size_t* consumed) {
  return one_shot(Inflater::Container::kGzip, src, n, dst, cap, out_len, consumed);
}

}  // namespace uda
