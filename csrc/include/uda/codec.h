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
// kZstd (ZStandardCodec) is a stream codec too, with a format of its own: one RFC 8878 frame per partition
// (csrc/codec/zstd.cc on the host, csrc/gpu/zstd.hip on the device). It goes wherever kZlib goes too; whoever
// goes on to decode dispatches three ways (DeviceStreamDecoder::decode, BlockDecoder).
enum class Codec { kNone = 0, kSnappy = 1, kLzo = 2, kLz4 = 3, kZlib = 4, kGzip = 5, kZstd = 6 };

// The codecs whose partition is one unframed stream (a zlib stream, a gzip member, a zstd frame), not a sequence
// of blocks.
inline bool is_stream_codec(Codec c) { return c == Codec::kZlib || c == Codec::kGzip || c == Codec::kZstd; }

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
// The same for a job, with ZStandardCodec: kZstd for a class name containing "ZStandardCodec", otherwise exactly
// what map_output_codec answers (whose answers are pinned by tests in turn, ZStandard refused among them). INIT
// and every other place that turns a job's codec class into a Codec call this one.
// Three resolvers are debt: each codec added since codec_from_class was pinned has left one behind. Folding them
// into one is a later change, which is then allowed to touch the tests that pin the two older ones.
Codec job_codec(const std::string& cls, bool* unsupported);
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

// ---- zstd (RFC 8878 frames: what ZStandardCodec's CompressorStream writes, one frame per partition, to our
// knowledge without dictionary, content size or checksum; the decoder takes everything the format allows).
// One shot, the contract of gzip_decompress: decodes the frames at src into one output, skipping skippable
// frames; stops where the bytes that follow cannot start a frame (fewer than 4 bytes, or no frame magic) and says
// where in *consumed (an IFile checksum behind the last frame is the caller's tail). false: a wrong magic, a
// reserved descriptor bit or block type, a dictionary id, a block larger than min(window, 128 KiB), a content size
// or content checksum that does not match, an offset that reaches before the frame's first byte, anything
// truncated, or more than cap bytes of output. An offset beyond Window_Size but inside the frame's output is
// taken, as libzstd's one-shot ZSTD_decompress takes it.
struct ZstdStats {  // what a decode met (coverage counters of the tests)
  int64_t frames = 0, skippable = 0, max_frame_blocks = 0;
  int64_t blocks[3] = {0, 0, 0};    // Raw, RLE, Compressed
  int64_t literals[4] = {0, 0, 0, 0};  // Raw, RLE, Compressed, Treeless
  int64_t huf_streams[2] = {0, 0};  // sections of 1 stream, of 4 streams
  int64_t weights[2] = {0, 0};      // direct, FSE-compressed
  int64_t modes[3][4] = {};         // [LL, OF, ML][Predefined, RLE, FSE_Compressed, Repeat]
  int64_t sequences = 0, max_offset = 0, checksums = 0;
};
bool zstd_decompress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len, size_t* consumed,
                     ZstdStats* stats = nullptr, std::string* why = nullptr);
// A small encoder, so that writers and tests can make zstd partitions with no zstd library: one frame, no
// checksum, no content size, blocks of at most 128 KiB; a greedy hash-chain matcher; compressed blocks with Raw
// literals and Predefined-mode sequences, an RLE block for a block of one repeated byte, a Raw block where
// the compressed form is not smaller.
size_t zstd_max_compressed_length(size_t n);
size_t zstd_compress(const uint8_t* src, size_t n, uint8_t* dst);

// Incremental zstd decoder: feed / read / finished / idle / starved / consumed as Inflater below. It restarts at
// unit boundaries: a frame header, a block header with its whole block, and a 4-byte content checksum are each
// committed only once whole, whatever the feed granularity. Memory is the frame's Window_Size plus one block (at
// most 128 KiB) of history and output, and one block of input, however long the frame is; a Window_Size above
// 128 MiB is refused by name. An offset beyond Window_Size is refused here, wherever the buffer stands (the
// one-shot decoder, which has the whole output, takes it as libzstd's one-shot call does).
class ZstdDecoder {
 public:
  ZstdDecoder();
  ~ZstdDecoder();
  void feed(const uint8_t* p, size_t n);
  size_t read(uint8_t* dst, size_t cap);  // throws UdaError("corrupt zstd frame: ...")
  bool finished() const { return state_ == kDone && skip_ == 0; }  // the last frame ended (a skippable one: all skipped)
  bool idle() const { return finished() && rpos_ == wpos_ && ipos_ == in_.size(); }
  bool starved() const { return !finished() && rpos_ == wpos_; }
  uint64_t consumed() const { return dropped_ + ipos_; }
  size_t history_bytes() const { return buf_.capacity(); }  // memory held for history and output (tests)
  size_t input_bytes() const { return in_.capacity(); }     // memory held for input not yet decoded (tests)

 private:
  enum State { kFrame, kBlock, kChecksum, kDone };
  struct Tables;
  bool run();
  std::unique_ptr<Tables> t_;
  std::vector<uint8_t> in_;
  size_t ipos_ = 0;
  uint64_t dropped_ = 0;
  std::vector<uint8_t> buf_;  // history + output: [0, wpos_) decoded, [rpos_, wpos_) not yet read
  size_t wpos_ = 0, rpos_ = 0, fstart_ = 0;  // fstart_: where the frame's output begins in buf_ (0 once slid away)
  uint64_t window_ = 0, frame_out_ = 0, fcs_ = 0, skip_ = 0;  // skip_: bytes of a skippable frame still to drop
  bool has_fcs_ = false, has_sum_ = false, any_frame_ = false;
  State state_ = kFrame;
};

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
    if (zstd_) return zstd_->idle();
    return out_pos_ == out_.size() && in_.size() == in_pos_ && block_remaining_ == 0;
  }
  // kZlib / kGzip / kZstd only: every decoded byte was read and the stream has not ended, so it waits for input (a block
  // codec's blocks end where their framing says, and this is always false).
  bool starved() const { return zlib_ ? zlib_->starved() : zstd_ && zstd_->starved(); }
  int64_t blocks() const { return blocks_; }

 private:
  bool decode_some();
  Codec codec_;
  std::unique_ptr<Inflater> zlib_;  // kZlib / kGzip: feed / read / idle go to it
  std::unique_ptr<ZstdDecoder> zstd_;  // kZstd: the same
  std::vector<uint8_t> in_;
  size_t in_pos_ = 0;
  std::vector<uint8_t> out_;
  size_t out_pos_ = 0;
  int64_t block_remaining_ = 0;  // raw bytes of the current block not yet produced
  int64_t blocks_ = 0;
};

}  // namespace uda
