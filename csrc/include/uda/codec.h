// Map-output compression codecs and Hadoop block-stream framing.
//
// Parity: DecompressorWrapper + LzoDecompressor + SnappyDecompressor (src/Merger/
// DecompressorWrapper.cc, LzoDecompressor.cc, SnappyDecompressor.cc). The reference dlopens
// liblzo2 / libsnappy; neither exists here, so both decoders are implemented in-tree (host C++;
// the GPU engine has its own per-block device decoders). LZ4 (Hadoop's Lz4Codec, same framing) goes
// beyond the reference, whose getCompAlg throws on it. Framing (Hadoop BlockCompressorStream):
//   block := [u32 BE uncompressed_len] { [u32 BE compressed_len][compressed bytes] }+
// The reference assumes one compressed chunk per block (LzoDecompressor.cc:151-167); we accept
// several chunks per block, which Hadoop emits when a block's compressed output is split.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace uda {

// kZlib (Hadoop's DefaultCodec / DeflateCodec) is no block codec: a partition is one RFC 1950 zlib stream
// with no framing, so block_compress, plan_block_streams* and launch_block_decode refuse it and the
// inflate entry points below (and csrc/gpu/inflate.hip) take it. Beyond the reference, like LZ4.
// kGzip (GzipCodec) is the same deflate data in another wrapper: one RFC 1952 member per partition, checked by
// a CRC-32 and a length where zlib has an Adler-32. It goes wherever kZlib goes (is_stream_codec).
enum class Codec { kNone = 0, kSnappy = 1, kLzo = 2, kLz4 = 3, kZlib = 4, kGzip = 5 };

// The codecs whose partition is one unframed deflate stream (zlib or gzip wrapper), not a sequence of blocks.
inline bool is_stream_codec(Codec c) { return c == Codec::kZlib || c == Codec::kGzip; }

// Map a Hadoop codec class name ("...SnappyCodec", "...LzoCodec", "...Lz4Codec", "...DefaultCodec",
// "...DeflateCodec") to a codec; kNone for ""/null. Unsupported names (Gzip, BZip2, ZStandard ...) return
// kNone and set *unsupported.
// This is the table of names the block and zlib entry points know, and it keeps every answer it ever gave:
// GzipCodec stays unsupported here. What a job's map outputs are written with is resolved by
// map_output_codec below, which is the one to call on a job's codec class.
Codec codec_from_class(const std::string& cls, bool* unsupported);
// The codec of a job's map outputs (mapreduce.map.output.compress.codec): kGzip for a class name containing
// "GzipCodec", otherwise exactly what codec_from_class answers. There are two resolvers because
// codec_from_class's answers are pinned (its callers and tests rely on Gzip being refused there); INIT and
// every other place that turns the job's codec class into a Codec call this one.
Codec map_output_codec(const std::string& cls, bool* unsupported);
const char* codec_name(Codec c);

// ---- Snappy (raw format: varint uncompressed length, then literal/copy tags)
size_t snappy_max_compressed_length(size_t n);
size_t snappy_compress(const uint8_t* src, size_t n, uint8_t* dst);
bool snappy_uncompressed_length(const uint8_t* src, size_t n, size_t* out);
bool snappy_decompress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len);

// ---- LZO1X (the format liblzo2's lzo1x_decompress_safe reads)
size_t lzo1x_max_compressed_length(size_t n);
size_t lzo1x_compress(const uint8_t* src, size_t n, uint8_t* dst);
bool lzo1x_decompress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len);

// ---- LZ4 (raw block format, what Hadoop's Lz4Compressor / Lz4Decompressor put in a chunk: no frame
// header, no stored length). The decoder is the safe variant; the encoder keeps the end-of-block rules.
size_t lz4_max_compressed_length(size_t n);
size_t lz4_compress(const uint8_t* src, size_t n, uint8_t* dst);
bool lz4_decompress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len);

// ---- zlib (RFC 1950 stream around RFC 1951 deflate: what DefaultCodec's CompressorStream writes, one
// stream per partition). Decode only; csrc/codec/inflate.cc. Refuses what zlib's inflate refuses.
// One shot: decodes the stream at src into dst[0, cap); *consumed = bytes of src the stream took (header
// to Adler-32). false: corrupt, truncated, Adler-32 mismatch, or more than cap bytes of output.
bool zlib_decompress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len, size_t* consumed);

// ---- gzip (RFC 1952 members around the same deflate data: what GzipCodec writes, one member per partition;
// Hadoop's writers emit the bare 10-byte header, its readers take the optional header fields and concatenated
// members, and so does this). Decodes the members at src into one output; every member's CRC-32 and ISIZE are
// verified. Behind a member's trailer another member begins only if at least 18 bytes remain and they start
// with 1f 8b 08; otherwise decoding stops there and *consumed says where (an IFile checksum behind the last
// member is the caller's tail, as with zlib). false: what zlib's inflate with wbits = 31 refuses (wrong magic,
// CM != 8, a reserved FLG bit, a wrong FHCRC, anything truncated, a CRC-32 or ISIZE that does not match), or
// more than cap bytes of output.
bool gzip_decompress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len, size_t* consumed);

// Incremental: feed compressed bytes in arbitrary pieces, read raw. Memory is a 32 KiB history plus a
// fixed output buffer however long the stream is. The decoder restarts at unit boundaries: it commits its
// bit position only after a whole block header (a dynamic header's code lengths included), a whole symbol
// with its extra bits, or a chunk of a stored block, and otherwise waits for more input.
// Container::kGzip: the same decoder around gzip members, with the same restart rules: a member's header
// (optional fields included) is committed only once it is whole, whatever the feed granularity, and so is its
// 8-byte trailer. finished(), idle(), starved() and consumed() then speak of the last member: behind a
// trailer the decoder goes on into another member once 18 bytes starting 1f 8b 08 are there, and stays
// finished otherwise.
class Inflater {
 public:
  enum class Container { kZlib, kGzip };
  explicit Inflater(Container c = Container::kZlib);
  void feed(const uint8_t* p, size_t n);
  // Copy up to `cap` decoded bytes into dst; 0 = needs more input, or the stream has ended.
  // Throws UdaError ("corrupt zlib stream: ...", "corrupt gzip stream: ...") on a stream zlib's inflate would refuse.
  size_t read(uint8_t* dst, size_t cap);
  bool finished() const { return state_ == kDone; }  // the Adler-32 (gzip: CRC-32 and ISIZE) was read and matched
  // Stream finished, no buffered output, no unconsumed input.
  bool idle() const { return finished() && rpos_ == wpos_ && (bitpos_ + 7) / 8 == in_.size(); }
  // After a read(): nothing is buffered and the stream has not ended: it needs more input.
  bool starved() const { return !finished() && rpos_ == wpos_; }
  uint64_t consumed() const { return dropped_ + (bitpos_ + 7) / 8; }  // input bytes the stream took so far

 private:
  enum State { kHeader, kBlockHeader, kStored, kSymbols, kAdler, kDone };  // kAdler: either container's trailer
  void run();  // decode until the output buffer is full, the input runs out or the stream ends
  void fail(const char* what) const;
  void slide();
  void sum();
  bool next_member();
  size_t gzip_header(const uint8_t* p, size_t n) const;
  std::vector<uint8_t> in_;
  uint64_t bitpos_ = 0;   // next unread bit of in_
  uint64_t dropped_ = 0;  // input bytes already dropped from in_
  std::vector<uint8_t> buf_;  // history + output: [0, wpos_) decoded, [rpos_, wpos_) not yet read
  size_t wpos_ = 0, rpos_ = 0, spos_ = 0;  // spos_: the Adler-32 covers [.., spos_)
  uint64_t total_out_ = 0;
  uint32_t adler_a_ = 1, adler_b_ = 0;
  const bool gzip_;
  uint32_t crc_ = 0;        // gzip: CRC-32 of the current member's output [.., spos_)
  uint64_t member_out_ = 0; // gzip: total_out_ where the current member began
  State state_ = kHeader;
  bool last_ = false;
  uint32_t stored_left_ = 0;
  std::vector<uint16_t> lit_, dist_;
};

// Compress `n` bytes into Hadoop block framing with blocks of at most `block_size` raw bytes.
std::vector<uint8_t> block_compress(Codec c, const uint8_t* src, size_t n, size_t block_size);

// Incremental decoder of a framed stream: feed compressed bytes in arbitrary pieces, read raw.
class BlockDecoder {
 public:
  explicit BlockDecoder(Codec c);
  // Append compressed input.
  void feed(const uint8_t* p, size_t n);
  // Copy up to `cap` decoded bytes into dst; returns bytes produced (0 = need more input).
  // Throws UdaError on a corrupt stream.
  size_t read(uint8_t* dst, size_t cap);
  // True when no buffered raw bytes remain and the input ended on a block boundary (kZlib: the stream
  // ended, with no input behind it).
  bool idle() const {
    if (zlib_) return zlib_->idle();
    return out_pos_ == out_.size() && in_.size() == in_pos_ && block_remaining_ == 0;
  }
  // kZlib / kGzip only: every decoded byte was read and the stream has not ended, so it waits for input (a block
  // codec's blocks end where their framing says, and this is always false).
  bool starved() const { return zlib_ && zlib_->starved(); }
  int64_t blocks() const { return blocks_; }

 private:
  bool decode_some();
  Codec codec_;
  std::unique_ptr<Inflater> zlib_;  // kZlib / kGzip: feed / read / idle go to it
  std::vector<uint8_t> in_;
  size_t in_pos_ = 0;
  std::vector<uint8_t> out_;
  size_t out_pos_ = 0;
  int64_t block_remaining_ = 0;  // raw bytes of the current block not yet produced
  int64_t blocks_ = 0;
};

}  // namespace uda
