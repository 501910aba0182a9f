#include "gpu_workspace.h"

namespace uda {

const int kOutSlots = [] {
  const char* e = std::getenv("UDA_OUT_SLOTS");
  return e ? std::max(2, std::min(64, std::atoi(e))) : 8;
}();
const int64_t kOutPiece = [] {
  const char* e = std::getenv("UDA_OUT_PIECE_MB");
  return (e ? std::max<int64_t>(1, std::min<int64_t>(256, std::atoll(e))) : 16) << 20;
}();

template <class T>
DevicePool<T>& DevicePool<T>::get() {
  static DevicePool* p = [] {
    auto* q = new DevicePool;  // never destroyed: HIP may be torn down first at exit
    // idle objects hold HBM: the device's byte budget trims them (largest first) under pressure
    gpu::HbmLedger::get().add_pool({[q](int d, int64_t want) { return q->trim(d, want); },
                                    [q](int d) { return q->idle(d); }});
    return q;
  }();
  return *p;
}
template DevicePool<DeviceWorkspace>& DevicePool<DeviceWorkspace>::get();
template DevicePool<EarlyStager>& DevicePool<EarlyStager>::get();

DeviceGate& DeviceGate::get(int which) {
  // never destroyed: tasks may outlive static teardown
  static DeviceGate* g[3] = {new DeviceGate, new DeviceGate, new DeviceGate};
  return *g[(unsigned)which % 3];
}

std::atomic<int>& staged_merges(int device) {
  static std::atomic<int> n[64];
  return n[device & 63];
}

DeviceMergeOut device_merge(DeviceWorkspace& ws, const std::vector<Span>& in_runs, Codec codec, KeyKind kind,
                            int64_t spacing, hipStream_t s, const gpu::GenericMerger::RoundFn& on_round,
                            bool pinned_src, CombineOp combine, int64_t round_bytes) {
  double round_ms = 0;
  gpu::GenericMerger::RoundFn timed;
  if (on_round)
    timed = [&](const std::vector<int64_t>& cuts, int64_t records, bool last) {
      const auto tr = std::chrono::steady_clock::now();
      on_round(cuts, records, last);
      round_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr).count();
    };
  auto t0 = std::chrono::steady_clock::now();
  std::vector<const uint8_t*> ptrs;
  std::vector<int64_t> lens;
  bool all_staged = codec == Codec::kNone && !in_runs.empty();
  for (const Span& sp : in_runs) {
    ptrs.push_back(sp.p);
    lens.push_back(sp.len);
    all_staged = all_staged && sp.dev != nullptr;
  }
  if (all_staged) {  // the partitions reached HBM while the fetch went on
    int64_t total = 0;
    std::vector<const uint8_t*> runs;
    for (const Span& sp : in_runs) {
      runs.push_back(sp.dev);
      total += sp.len;
    }
    DeviceWorkspace::ensure(ws.out, total);
    auto t1 = std::chrono::steady_clock::now();
    ws.h2d_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
    gpu::GenericMergeResult r =
        ws.merger.merge(runs, lens, (int)kind, ws.out.as<uint8_t>(), total, spacing, s, timed, round_bytes, combine);
    HIP_CHECK(hipStreamSynchronize(s));
    ws.device_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count() - round_ms;
    DeviceMergeOut res;
    res.bytes = r.bytes;
    res.cuts = std::move(r.cuts);
    res.records = r.records;
    res.records_in = r.records_in;
    return res;
  }
  gpu::BlockPlan plan;
  bool decode_on_device = false;
  std::vector<std::vector<uint8_t>> host_raw;  // host-decoded fallback
  if (codec != Codec::kNone) {
    decode_on_device = gpu::plan_block_streams(codec, ptrs, lens, &plan);
    if (!decode_on_device) {
      UDA_LOG(kInfo, "device decode: framing needs a host decode (multi-chunk %s block)", codec_name(codec));
      for (size_t i = 0; i < ptrs.size(); ++i) {
        BlockDecoder dec(codec);
        dec.feed(ptrs[i], (size_t)lens[i]);
        std::vector<uint8_t> raw, buf(1 << 20);
        for (size_t n; (n = dec.read(buf.data(), buf.size())) > 0;) raw.insert(raw.end(), buf.begin(), buf.begin() + (long)n);
        if (!dec.idle()) throw UdaError("truncated compressed partition");
        host_raw.push_back(std::move(raw));
      }
      ptrs.clear();
      lens.clear();
      for (auto& r : host_raw) {
        ptrs.push_back(r.data());
        lens.push_back((int64_t)r.size());
      }
    }
  }
  int64_t staged = 0;
  for (auto l : lens) staged += l;
  const int64_t total = decode_on_device ? plan.raw_total : staged;
  DeviceWorkspace::ensure(ws.in, total);
  DeviceWorkspace::ensure(ws.out, total);
  if (decode_on_device) DeviceWorkspace::ensure(ws.packed, staged);
  gpu::DeviceBuffer& in = ws.in;
  gpu::DeviceBuffer& out = ws.out;
  uint8_t* stage = decode_on_device ? ws.packed.as<uint8_t>() : in.as<uint8_t>();
  std::vector<const uint8_t*> runs;
  std::vector<int64_t> bytes;
  int64_t off = 0;
  gpu::SdmaEngine* h2d = nullptr;
  if (pinned_src && host_raw.empty() && ws.h2d_sdma_ok) {
    try {
      int dev = 0;
      HIP_CHECK(hipGetDevice(&dev));
      h2d = &gpu::SdmaEngine::for_device(dev);
      if (!ws.h2d_sig.handle) ws.h2d_sig = h2d->make_signal();
      gpu::SdmaEngine::arm(ws.h2d_sig, 0);
    } catch (const std::exception&) {
      h2d = nullptr;
      ws.h2d_sdma_ok = false;
    }
  }
  for (size_t i = 0; i < ptrs.size(); ++i) {
    if (lens[i] > 0 && h2d) {
      gpu::SdmaEngine::add(ws.h2d_sig, 1);
      h2d->copy_h2d(stage + off, ptrs[i], (size_t)lens[i], ws.h2d_sig);
    } else if (lens[i] > 0) {
      HIP_CHECK(hipMemcpyAsync(stage + off, ptrs[i], (size_t)lens[i], hipMemcpyHostToDevice, s));
    }
    if (decode_on_device) {
      runs.push_back(in.as<uint8_t>() + plan.raw_offset[i]);
      bytes.push_back(plan.raw_offset[i + 1] - plan.raw_offset[i]);
    } else {
      runs.push_back(in.as<uint8_t>() + off);
      bytes.push_back(lens[i]);
    }
    off += lens[i];
  }
  if (h2d) gpu::SdmaEngine::wait(ws.h2d_sig);
  HIP_CHECK(hipStreamSynchronize(s));
  auto t1 = std::chrono::steady_clock::now();
  ws.h2d_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
  const int64_t tm = trace::host_enabled() ? trace::now_ns() : 0;
  if (tm) trace::host_event("dm_h2d", staged, (int64_t)ptrs.size(), tm - (int64_t)((t1 - t0).count()), tm);
  DeviceMergeOut res;
  if (decode_on_device) {
    ws.decoder.decode(codec, plan, ws.packed.as<uint8_t>(), in.as<uint8_t>(), s);
    res.decoded_blocks = (int64_t)plan.descs.size();
  }
  host_raw.clear();
  gpu::GenericMergeResult r =
      ws.merger.merge(runs, bytes, (int)kind, out.as<uint8_t>(), total, spacing, s, timed, round_bytes, combine);
  HIP_CHECK(hipStreamSynchronize(s));
  ws.device_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count() - round_ms;
  if (tm) trace::host_event("dm_merge", total, (int64_t)ptrs.size(), tm, trace::now_ns());
  res.bytes = r.bytes;
  res.cuts = std::move(r.cuts);
  res.records = r.records;
  res.records_in = r.records_in;
  return res;
}

std::vector<size_t> piece_bounds(const std::vector<int64_t>& cuts, int64_t limit) {
  const size_t nb = cuts.size() - 1;
  std::vector<size_t> pb{0};
  while (pb.back() < nb) {
    const size_t j = pb.back();
    if (cuts[j + 1] - cuts[j] > limit) return {};
    size_t k = j + 1;
    while (k < nb && cuts[k + 1] - cuts[j] <= limit) ++k;
    pb.push_back(k);
  }
  return pb;
}

}  // namespace uda
