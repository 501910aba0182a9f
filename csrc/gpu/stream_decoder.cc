// zlib / gzip / zstd stream plan and device decode: see stream_decoder.h.
#include "stream_decoder.h"

#include <cstdio>
#include <cstring>

#include "uda/error.h"
#include "uda/ifile.h"
#include "uda/trace.h"

namespace uda {
namespace gpu {

bool plan_zlib_streams(const std::vector<const uint8_t*>& ptrs, const std::vector<int64_t>& lens,
                       const std::vector<int64_t>& raw_lens, StreamPlan* plan) {
  constexpr int64_t kLimit = 1ll << 31;  // the kernel's positions are 32-bit
  plan->descs.clear();
  plan->raw_offset.assign(1, 0);
  plan->raw_total = 0;
  int64_t in_off = 0, raw = 0;
  for (size_t i = 0; i < lens.size(); ++i) {
    if (raw_lens[i] <= 0 || raw_lens[i] >= kLimit || lens[i] >= kLimit) return false;
    const int64_t src = ptrs.empty() ? in_off : (int64_t)reinterpret_cast<uintptr_t>(ptrs[i]);
    plan->descs.push_back(InflateDesc{src, lens[i], raw, raw_lens[i]});
    in_off += lens[i];
    raw += raw_lens[i];
    plan->raw_offset.push_back(raw);
  }
  plan->raw_total = raw;
  return true;
}

namespace {
const char* status_text(int st) {
  switch (st) {
    case kInflateTruncated: return "truncated";
    case kInflateOverflow: return "more output than its index says";
    case kInflateTooBig: return "2 GiB or more";
    default: return "refused";
  }
}
size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
}  // namespace

void DeviceStreamDecoder::decode(const StreamPlan& plan, const uint8_t* d_in, uint8_t* d_out,
                                 const std::vector<std::string>& ids, hipStream_t s, std::vector<int>* tails,
                                 int* failed, std::string* why, Codec container) {
  if (!is_stream_codec(container)) throw UdaError("DeviceStreamDecoder: " + std::string(codec_name(container)) + " is no stream codec");
  if (container == Codec::kZstd) return decode_zstd(plan, d_in, d_out, ids, s, tails, failed, why);
  const bool gzip = container == Codec::kGzip;
  const int n = (int)plan.descs.size();
  if (failed) *failed = -1;
  if (tails) tails->assign((size_t)n, 0);
  results_.assign((size_t)n, InflateResult{});
  if (n == 0) return;
  trace::Range tr("uda.inflate_streams");
  // scratch: descs | results | out ptrs | out lens | check out | adler work; gzip, in place of the last:
  // crc descs | chunk_first | crc chunk states
  const size_t o_desc = 0, o_res = up16(o_desc + (size_t)n * sizeof(InflateDesc));
  const size_t o_ptr = up16(o_res + (size_t)n * sizeof(InflateResult)), o_len = o_ptr + (size_t)n * 8;
  const size_t o_adler = up16(o_len + (size_t)n * 8), o_work = up16(o_adler + (size_t)n * 4);
  std::vector<CrcDesc> cdesc;
  std::vector<int64_t> cfirst;
  int64_t chunks = 0;
  const size_t o_first = up16(o_work + (size_t)n * sizeof(CrcDesc));
  size_t o_states = 0, bytes = o_work + (size_t)n * 16;
  if (gzip) {  // the output addresses and raw lengths are known here, so is the CRC kernel's chunk plan
    cdesc.resize((size_t)n);
    cfirst.resize((size_t)n + 1);
    for (int i = 0; i < n; ++i) cdesc[(size_t)i] = CrcDesc{d_out + plan.descs[(size_t)i].dst, plan.descs[(size_t)i].raw_len};
    chunks = crc32_chunk_plan(cdesc.data(), n, cfirst.data());
    o_states = up16(o_first + ((size_t)n + 1) * 8);
    bytes = o_states + crc32_ws_bytes(chunks);
  }
  if (scratch_.size() < bytes) scratch_.alloc(bytes + bytes / 2);
  uint8_t* const base = scratch_.as<uint8_t>();
  std::vector<const uint8_t*> optr((size_t)n);
  std::vector<int64_t> olen((size_t)n);
  for (int i = 0; i < n; ++i) {
    optr[(size_t)i] = d_out + plan.descs[(size_t)i].dst;
    olen[(size_t)i] = plan.descs[(size_t)i].raw_len;
  }
  HIP_CHECK(hipMemcpyAsync(base + o_desc, plan.descs.data(), (size_t)n * sizeof(InflateDesc), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(base + o_ptr, optr.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(base + o_len, olen.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(base + o_res, 0xFF, (size_t)n * sizeof(InflateResult), s));  // (a status no wave wrote reads as an error)
  if (gzip) {
    HIP_CHECK(hipMemcpyAsync(base + o_work, cdesc.data(), (size_t)n * sizeof(CrcDesc), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(base + o_first, cfirst.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
  }
  launch_inflate_streams(d_in, d_out, reinterpret_cast<const InflateDesc*>(base + o_desc), n,
                         reinterpret_cast<InflateResult*>(base + o_res), s, gzip ? kContainerGzip : kContainerZlib);
  HIP_CHECK(hipGetLastError());
  // the format's own integrity check, always on: over the bytes just decoded, in the same pass over s
  if (gzip)
    launch_crc32(reinterpret_cast<const CrcDesc*>(base + o_work), n, reinterpret_cast<const int64_t*>(base + o_first), chunks,
                 base + o_states, reinterpret_cast<uint32_t*>(base + o_adler), s);
  else
    launch_adler32(reinterpret_cast<const uint8_t* const*>(base + o_ptr), reinterpret_cast<const int64_t*>(base + o_len), n,
                   reinterpret_cast<uint32_t*>(base + o_adler), reinterpret_cast<uint64_t*>(base + o_work), s);
  HIP_CHECK(hipGetLastError());
  std::vector<uint32_t> adler((size_t)n);
  HIP_CHECK(hipMemcpyAsync(results_.data(), base + o_res, (size_t)n * sizeof(InflateResult), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(adler.data(), base + o_adler, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  auto check = [&](int i) -> std::string {  // "" = stream i is good, its tail filled in
    const InflateResult& r = results_[(size_t)i];
    const InflateDesc& d = plan.descs[(size_t)i];
    const std::string id = (size_t)i < ids.size() ? ids[(size_t)i] : "#" + std::to_string(i);
    if (r.status != kInflateOk)
      return std::string(gzip ? "corrupt gzip stream in map output " : "corrupt zlib stream in map output ") + id + " (" +
             status_text(r.status) + ", device inflate)";
    const int64_t tail = d.src_len - r.consumed;
    if (gzip && tail >= 18) {
      // what the host decoders take for the start of another member (Inflater::next_member). Asked first: the
      // index's raw length covers every member, so the length and CRC comparisons below (over raw_len bytes)
      // would only say that one member decodes to less. The three bytes are read from where the stream lies:
      // the device input, or the absolute address the descriptor holds
      uint8_t head[3] = {0, 0, 0};
      const uint8_t* at = (d_in ? d_in + d.src : reinterpret_cast<const uint8_t*>((uintptr_t)d.src)) + r.consumed;
      HIP_CHECK(hipMemcpy(head, at, sizeof head, hipMemcpyDefault));
      if (head[0] == 0x1f && head[1] == 0x8b && head[2] == 8)
        return "gzip map output " + id + " holds more than one member (the device inflate decodes one; "
               "mapred.uda.gpu.decompress=0 decodes it on the host)";
    }
    if (r.produced != d.raw_len)
      return "compressed map output " + id + " decodes to " + std::to_string(r.produced) + " bytes, its index says " +
             std::to_string(d.raw_len);
    if (r.check_stored != adler[(size_t)i]) {
      char buf[64];
      std::snprintf(buf, sizeof buf, "stored 0x%08x, computed 0x%08x", r.check_stored, adler[(size_t)i]);
      return std::string(gzip ? "gzip CRC-32 mismatch in map output " : "zlib Adler-32 mismatch in map output ") + id + ": " + buf;
    }
    if (gzip && r.isize != (uint32_t)r.produced)
      return "gzip length mismatch in map output " + id + ": stored " + std::to_string(r.isize) + ", decoded " +
             std::to_string(r.produced);
    if (tail != 0 && tail != kIFileChecksumBytes)
      return std::string(gzip ? "corrupt gzip stream in map output " : "corrupt zlib stream in map output ") + id + ": " + std::to_string(tail) +
             " bytes behind its end (an IFile checksum has " + std::to_string(kIFileChecksumBytes) + ")";
    if (tails) (*tails)[(size_t)i] = (int)tail;
    return std::string();
  };
  for (int i = 0; i < n; ++i) {
    const std::string err = check(i);
    if (err.empty()) continue;
    if (!failed) throw UdaError(err);
    if (*failed < 0) {
      *failed = i;
      if (why) *why = err;
    }
  }
}

void DeviceStreamDecoder::decode_zstd(const StreamPlan& plan, const uint8_t* d_in, uint8_t* d_out,
                                      const std::vector<std::string>& ids, hipStream_t s, std::vector<int>* tails,
                                      int* failed, std::string* why) {
  const int n = (int)plan.descs.size();
  if (failed) *failed = -1;
  if (tails) tails->assign((size_t)n, 0);
  zresults_.assign((size_t)n, ZstdResult{});
  if (n == 0) return;
  trace::Range tr("uda.zstd_frames");
  // scratch: descs | results | xxh ptrs | xxh lens | xxh out | literal scratch (128 KiB a frame)
  const size_t o_desc = 0, o_res = up16(o_desc + (size_t)n * sizeof(InflateDesc));
  const size_t o_ptr = up16(o_res + (size_t)n * sizeof(ZstdResult)), o_len = o_ptr + (size_t)n * 8;
  const size_t o_sum = up16(o_len + (size_t)n * 8), o_lit = up16(o_sum + (size_t)n * 8);
  const size_t bytes = o_lit + (size_t)n * (size_t)zstd_literal_scratch();
  if (scratch_.size() < bytes) scratch_.alloc(bytes);  // (exactly: admission reserves 128 KiB a frame, no slack)
  uint8_t* const base = scratch_.as<uint8_t>();
  HIP_CHECK(hipMemcpyAsync(base + o_desc, plan.descs.data(), (size_t)n * sizeof(InflateDesc), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(base + o_res, 0xFF, (size_t)n * sizeof(ZstdResult), s));  // (a status no wave wrote reads as an error)
  launch_zstd_frames(d_in, d_out, reinterpret_cast<const InflateDesc*>(base + o_desc), n,
                     reinterpret_cast<ZstdResult*>(base + o_res), base + o_lit, s);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(zresults_.data(), base + o_res, (size_t)n * sizeof(ZstdResult), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  // the content checksum, where a frame carries one: over the bytes just decoded. Only the frames that decoded
  // and say so are summed (the others get an empty range), and with none there is no launch
  std::vector<uint64_t> sums((size_t)n, 0);
  std::vector<const uint8_t*> xptr((size_t)n, nullptr);
  std::vector<int64_t> xlen((size_t)n, 0);
  bool any_sum = false;
  for (int i = 0; i < n; ++i) {
    const ZstdResult& r = zresults_[(size_t)i];
    if (r.status != kInflateOk || !r.has_checksum) continue;
    xptr[(size_t)i] = d_out + plan.descs[(size_t)i].dst;
    xlen[(size_t)i] = r.produced;  // (<= raw_len: the kernel wrote no further)
    any_sum = true;
  }
  if (any_sum) {
    HIP_CHECK(hipMemcpyAsync(base + o_ptr, xptr.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(base + o_len, xlen.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    launch_xxh64(reinterpret_cast<const uint8_t* const*>(base + o_ptr), reinterpret_cast<const int64_t*>(base + o_len), n,
                 reinterpret_cast<uint64_t*>(base + o_sum), s);
    HIP_CHECK(hipGetLastError());
    ++xxh64_launches_;
    HIP_CHECK(hipMemcpyAsync(sums.data(), base + o_sum, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  auto check = [&](int i) -> std::string {  // "" = frame i is good, its tail filled in
    const ZstdResult& r = zresults_[(size_t)i];
    const InflateDesc& d = plan.descs[(size_t)i];
    const std::string id = (size_t)i < ids.size() ? ids[(size_t)i] : "#" + std::to_string(i);
    if (r.status != kInflateOk)
      return "corrupt zstd frame in map output " + id + " (" +
             (r.status == kInflateTooBig ? "2 GiB or more" : zstd_reason_text(r.reason)) + ", device decode)";
    const int64_t tail = d.src_len - r.consumed;
    if (tail >= 4 && tail != kIFileChecksumBytes) {
      // what the host decoders take for the start of another frame. Asked first: the index's raw length covers
      // every frame, so the length comparison below would only say that one frame decodes to less
      uint8_t head[4] = {0, 0, 0, 0};
      const uint8_t* at = (d_in ? d_in + d.src : reinterpret_cast<const uint8_t*>((uintptr_t)d.src)) + r.consumed;
      HIP_CHECK(hipMemcpy(head, at, sizeof head, hipMemcpyDefault));
      const uint32_t magic = (uint32_t)head[0] | ((uint32_t)head[1] << 8) | ((uint32_t)head[2] << 16) | ((uint32_t)head[3] << 24);
      if (magic == 0xFD2FB528u || (magic & 0xFFFFFFF0u) == 0x184D2A50u)
        return "zstd map output " + id + " holds more than one frame (the device decode takes one; "
               "mapred.uda.gpu.decompress=0 decodes it on the host)";
    }
    if (r.produced != d.raw_len)
      return "compressed map output " + id + " decodes to " + std::to_string(r.produced) + " bytes, its index says " +
             std::to_string(d.raw_len);
    if (r.has_checksum && r.check_stored != (uint32_t)sums[(size_t)i]) {
      char buf[64];
      std::snprintf(buf, sizeof buf, "stored 0x%08x, computed 0x%08x", r.check_stored, (uint32_t)sums[(size_t)i]);
      return "zstd content checksum mismatch in map output " + id + ": " + buf;
    }
    if (tail != 0 && tail != kIFileChecksumBytes)
      return "corrupt zstd frame in map output " + id + ": " + std::to_string(tail) +
             " bytes behind its end (an IFile checksum has " + std::to_string(kIFileChecksumBytes) + ")";
    if (tails) (*tails)[(size_t)i] = (int)tail;
    return std::string();
  };
  for (int i = 0; i < n; ++i) {
    const std::string err = check(i);
    if (err.empty()) continue;
    if (!failed) throw UdaError(err);
    if (*failed < 0) {
      *failed = i;
      if (why) *why = err;
    }
  }
}

}  // namespace gpu
}  // namespace uda
