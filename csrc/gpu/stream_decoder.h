// Host side of the zlib (DefaultCodec), gzip (GzipCodec) and zstd (ZStandardCodec) device decode: one inflate descriptor per partition and the launches
// of csrc/gpu/inflate.hip and adler32.hip (gzip: crc32.hip). The sibling of block_decoder.h for the codec that has no blocks:
// a partition is one zlib stream, its raw size comes from the index and its end (and with it whether an IFile
// checksum trailer follows) is known only once it has been decoded.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "device_engine.h"
#include "kernels.h"
#include "uda/codec.h"

namespace uda {
namespace gpu {

struct StreamPlan {
  std::vector<InflateDesc> descs;   // one per stream, outputs back to back
  std::vector<int64_t> raw_offset;  // per stream: first raw byte (size streams + 1)
  int64_t raw_total = 0;
};

// Streams of lens[i] bytes that decode to raw_lens[i] bytes (the index's rawLength). ptrs given: absolute
// device addresses (decode with d_in = nullptr); ptrs empty: stream i lies at sum(lens[<i]) of one buffer.
// false: a raw length is unknown (<= 0), or a stream or its output is 2 GiB or more: the caller decodes on
// the host.
bool plan_zlib_streams(const std::vector<const uint8_t*>& ptrs, const std::vector<int64_t>& lens,
                       const std::vector<int64_t>& raw_lens, StreamPlan* plan);

class DeviceStreamDecoder {
 public:
  // Inflate every stream of the plan into d_out and sum the decoded bytes (Adler-32) in the same pass over
  // the stream s; synchronizes s. ids[i] names map output i in the errors (may be short: "#i" then). Throws
  // UdaError: "corrupt zlib stream in map output <id>" (truncated streams and output past the raw length
  // included, the reason in brackets), "compressed map output <id> decodes to N bytes, its index says M",
  // "zlib Adler-32 mismatch in map output <id>: stored 0x..., computed 0x...", and a malformed tail.
  // tails[i] = bytes of stream i behind its Adler-32: 0, or 4 (an IFile checksum trailer).
  // container = Codec::kGzip: the streams are gzip members. The launch decodes them in gzip mode and the
  // batched CRC-32 (launch_crc32, its descriptors and chunk plan laid from the host-known output addresses
  // and raw lengths, its workspace from this decoder's scratch) takes the Adler-32's place on the same
  // stream. Errors: "corrupt gzip stream in map output <id> (<reason>, device inflate)", "gzip CRC-32
  // mismatch in map output <id>: stored 0x..., computed 0x...", "gzip length mismatch in map output <id>:
  // stored N, decoded M" (ISIZE against the bytes produced mod 2^32), and, the device inflate decoding one
  // member per stream, "gzip map output <id> holds more than one member (...)" when the bytes behind a good
  // member are neither 0 nor 4 and are 18 or more starting 1f 8b 08. The zlib messages are unchanged.
  // container = Codec::kZstd: the streams are zstd frames (zstd.hip, one frame per stream). The scratch grows by
  // zstd_literal_scratch() = 128 KiB per stream for the blocks' decoded literals. XXH64 (xxh64.hip) runs over
  // the outputs of the frames that carry a content checksum, and is not launched when none does. Errors:
  // "corrupt zstd frame in map output <id> (<reason>, device decode)" (a dictionary id among the reasons: "needs
  // a dictionary"), "zstd content checksum mismatch in map output <id>: stored 0x..., computed 0x...", and
  // "zstd map output <id> holds more than one frame (...)" when the bytes behind a good frame are neither 0 nor
  // 4 and begin with a frame or skippable-frame magic.
  // failed (optional): instead of throwing, the first stream in error is reported there with its message in
  // *why (-1: none) and the other streams' tails are still filled in. A stream that does not decode has no
  // known end, so the caller that verifies IFile checksums can first hold that partition's bytes against the
  // trailer its neighbours show it to have, and report a partition damaged on its way as a checksum mismatch.
  void decode(const StreamPlan& plan, const uint8_t* d_in, uint8_t* d_out, const std::vector<std::string>& ids,
              hipStream_t s, std::vector<int>* tails, int* failed = nullptr, std::string* why = nullptr,
              Codec container = Codec::kZlib);
  const std::vector<InflateResult>& results() const { return results_; }
  const std::vector<ZstdResult>& zstd_results() const { return zresults_; }
  int64_t scratch_bytes() const { return (int64_t)scratch_.held(); }  // device memory held between decodes
  int64_t xxh64_launches() const { return xxh64_launches_; }  // launches of the content-checksum kernel so far

 private:
  void decode_zstd(const StreamPlan& plan, const uint8_t* d_in, uint8_t* d_out, const std::vector<std::string>& ids,
                   hipStream_t s, std::vector<int>* tails, int* failed, std::string* why);
  std::vector<ZstdResult> zresults_;
  int64_t xxh64_launches_ = 0;
  DeviceBuffer scratch_;
  std::vector<InflateResult> results_;
};

}  // namespace gpu
}  // namespace uda
