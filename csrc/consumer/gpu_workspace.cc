#include "gpu_workspace.h"

#include "uda/ifile.h"

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

std::vector<uint8_t> host_decode_partition(Codec codec, const uint8_t* p, int64_t n, int* tail) {
  *tail = 0;
  BlockDecoder dec(codec);
  std::vector<uint8_t> raw, buf(1 << 20);
  auto drain = [&] {
    for (size_t k; (k = dec.read(buf.data(), buf.size())) > 0;) raw.insert(raw.end(), buf.begin(), buf.begin() + (long)k);
  };
  // all but the last four bytes first: if the blocks end there, those four are the IFile checksum
  const int64_t hold = n >= kIFileChecksumBytes ? kIFileChecksumBytes : 0;
  dec.feed(p, (size_t)(n - hold));
  drain();
  if (hold && dec.idle()) {
    *tail = kIFileChecksumBytes;
    return raw;
  }
  dec.feed(p + (n - hold), (size_t)hold);
  drain();
  if (!dec.idle()) throw UdaError("truncated compressed partition");
  return raw;
}

DeviceMergeOut device_merge(DeviceWorkspace& ws, const std::vector<Span>& in_runs, Codec codec, KeyKind kind,
                            int64_t spacing, hipStream_t s, const gpu::GenericMerger::RoundFn& on_round,
                            bool pinned_src, CombineOp combine, int64_t round_bytes, const ChecksumPolicy* ck) {
  double round_ms = 0;
  DeviceMergeOut res;
  const bool verify = ck && ck->verify;
  const bool slice_states = ck && ck->slice_states;
  if (slice_states && codec != Codec::kNone) throw UdaError("device_merge: slice checksum states of compressed runs");
  auto name_of = [&](const Span& sp) {
    return ck && ck->map_ids && sp.id >= 0 && (size_t)sp.id < ck->map_ids->size() ? (*ck->map_ids)[(size_t)sp.id]
                                                                                   : std::string("?");
  };
  std::vector<gpu::DeviceChecksum::Item> items;
  auto verified = [&] {  // the launch's results are in
    res.checksum_parts += ws.checksum.partitions();
    res.checksum_bytes += ws.checksum.bytes();
    res.checksum_ms += ws.checksum.ms();
    ws.checksum.reset();
  };
  // a numeric kind's key of the wrong length (gpu::BadKeyError): the failure names the map output
  auto merge_runs = [&](const std::vector<const uint8_t*>& runs, const std::vector<int64_t>& lens, uint8_t* out,
                        int64_t total, const gpu::GenericMerger::RoundFn& fn) {
    try {
      return ws.merger.merge(runs, lens, (int)kind, out, total, spacing, s, fn, round_bytes, combine);
    } catch (const gpu::BadKeyError& e) {
      std::string who = e.run >= 0 && (size_t)e.run < in_runs.size() ? name_of(in_runs[(size_t)e.run]) : std::string("?");
      if (who == "?") who = "#" + std::to_string(e.run);
      throw UdaError(key_bad_length_message(kind, e.klen, "map output " + who));
    }
  };
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
    // IFile checksums where the staged bytes are (the stager copied every partition whole: its trailer
    // lies behind its body); the merge hands records over as it goes, so the result is read first
    for (const Span& sp : in_runs) {
      if (!sp.tail) continue;
      ++res.trailers;
      if (verify) items.push_back(gpu::DeviceChecksum::Item{sp.dev, sp.len, name_of(sp), false, 0});
    }
    if (!items.empty()) {
      ws.checksum.reset();
      ws.checksum.launch(std::move(items), s);
      ws.checksum.finish(s, false);
      verified();
    }
    auto t1 = std::chrono::steady_clock::now();
    ws.h2d_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
    gpu::GenericMergeResult r = merge_runs(runs, lens, ws.out.as<uint8_t>(), total, timed);
    HIP_CHECK(hipStreamSynchronize(s));
    ws.device_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count() - round_ms;
    res.bytes = r.bytes;
    res.cuts = std::move(r.cuts);
    res.records = r.records;
    res.records_in = r.records_in;
    return res;
  }
  gpu::BlockPlan plan;
  bool decode_on_device = false;
  std::vector<std::vector<uint8_t>> host_raw;  // host-decoded fallback
  std::vector<int> tails(ptrs.size(), 0);  // IFile checksum trailer of run i: bytes behind its body
  auto check_raw_len = [&](size_t i, int64_t decoded) {
    if (tails[i] && in_runs[i].raw_len > 0 && decoded != in_runs[i].raw_len)
      throw UdaError("compressed map output " + name_of(in_runs[i]) + " decodes to " + std::to_string(decoded) +
                     " bytes, its index says " + std::to_string(in_runs[i].raw_len));
  };
  // zlib (DefaultCodec) and gzip (GzipCodec): no framing to walk. One inflate descriptor per run from the index's raw lengths; the
  // runs' ends, and with them their trailers, are known only once they are decoded (below, behind the copies).
  gpu::StreamPlan zplan;
  bool inflate_on_device = false;
  if (is_stream_codec(codec)) {
    std::vector<int64_t> raws;
    for (const Span& sp : in_runs) raws.push_back(sp.raw_len);
    inflate_on_device = gpu::plan_zlib_streams({}, lens, raws, &zplan);
    if (inflate_on_device) {
      plan.raw_offset = zplan.raw_offset;
      plan.raw_total = zplan.raw_total;
    }
  }
  if (codec != Codec::kNone) {
    decode_on_device = inflate_on_device || (!is_stream_codec(codec) && gpu::plan_block_streams(codec, ptrs, lens, &plan, &tails));
    if (decode_on_device && !inflate_on_device)
      for (size_t i = 0; i < ptrs.size(); ++i) check_raw_len(i, plan.raw_offset[i + 1] - plan.raw_offset[i]);
    if (!decode_on_device) {
      if (is_stream_codec(codec))
        UDA_LOG(kInfo, "device decode: a %s partition of unknown or 2 GiB raw length needs a host decode", codec_name(codec));
      else
        UDA_LOG(kInfo, "device decode: framing needs a host decode (multi-chunk %s block)", codec_name(codec));
      for (size_t i = 0; i < ptrs.size(); ++i) {
        // (the bytes are decoded here, on the host: so is their checksum)
        std::vector<uint8_t> raw = host_decode_partition(codec, ptrs[i], lens[i], &tails[i]);
        check_raw_len(i, (int64_t)raw.size());
        if (tails[i]) {
          ++res.trailers;
          const int64_t body = lens[i] - tails[i];
          if (verify) {
            const uint32_t stored = ifile_stored_checksum(ptrs[i] + body), got = crc32_ieee(ptrs[i], (size_t)body);
            if (stored != got) throw UdaError(ifile_checksum_mismatch(name_of(in_runs[i]), stored, got, body));
            ++res.checksum_parts;
            res.checksum_bytes += body;
          }
          tails[i] = 0;  // (done with: what is staged below is the decoded partition)
        }
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
    // the partition's bytes as fetched, where they were just staged; the stored value from the host copy
    const int tail = codec != Codec::kNone ? tails[i] : (host_raw.empty() ? in_runs[i].tail : 0);
    if (slice_states) {  // every run, empty ones too: slice_crc is indexed by run
      items.push_back(gpu::DeviceChecksum::Item{stage + off, lens[i], std::string(), true, 0});
    } else if (tail) {
      ++res.trailers;
      const int64_t body = codec != Codec::kNone ? lens[i] - tail : lens[i];
      if (verify)
        items.push_back(gpu::DeviceChecksum::Item{stage + off, body, name_of(in_runs[i]), true,
                                                  ifile_stored_checksum(ptrs[i] + body)});
    }
    off += lens[i];
  }
  if (h2d) gpu::SdmaEngine::wait(ws.h2d_sig);
  if (!items.empty()) {  // behind the copies on s (SDMA copies have landed), ahead of the wait for them
    ws.checksum.reset();
    ws.checksum.launch(std::move(items), s, slice_states);
  }
  HIP_CHECK(hipStreamSynchronize(s));
  if (ws.checksum.pending()) {
    ws.checksum.finish(s, true, slice_states ? &res.slice_crc : nullptr);
    verified();
  }
  auto t1 = std::chrono::steady_clock::now();
  ws.h2d_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
  const int64_t tm = trace::host_enabled() ? trace::now_ns() : 0;
  if (tm) trace::host_event("dm_h2d", staged, (int64_t)ptrs.size(), tm - (int64_t)((t1 - t0).count()), tm);
  if (inflate_on_device) {
    std::vector<gpu::DeviceChecksum::Item> zitems;  // (`items` may have been moved from above)
    std::vector<std::string> ids;
    for (const Span& sp : in_runs) ids.push_back(name_of(sp));
    int bad = -1;
    std::string why;
    ws.inflater.decode(zplan, ws.packed.as<uint8_t>(), in.as<uint8_t>(), ids, s, &tails, &bad, &why, codec);
    if (bad >= 0) {
      // a stream that does not decode has no known end. Where the merge's other runs carry a trailer, so does
      // this one: its CRC tells a run damaged on its way (the checksum mismatch, as for every other codec) from
      // a stream that was written wrong (the decoder's own message)
      bool trailers_seen = false;
      for (int t : tails) trailers_seen = trailers_seen || t == kIFileChecksumBytes;
      const size_t b = (size_t)bad;
      if (verify && trailers_seen && lens[b] > kIFileChecksumBytes) {
        int64_t boff = 0;
        for (size_t i = 0; i < b; ++i) boff += lens[i];
        const int64_t body = lens[b] - kIFileChecksumBytes;
        zitems.push_back(gpu::DeviceChecksum::Item{ws.packed.as<uint8_t>() + boff, body, name_of(in_runs[b]), true,
                                                  ifile_stored_checksum(ptrs[b] + body)});
        ws.checksum.reset();
        ws.checksum.launch(std::move(zitems), s);
        ws.checksum.finish(s, false);
      }
      throw UdaError(why);
    }
    res.decoded_streams = (int64_t)zplan.descs.size();
    // the tails are known now: the IFile checksums over the bytes as staged, verified before the merge below
    // hands a record over (the stored value from the host copy)
    int64_t zoff = 0;
    for (size_t i = 0; i < ptrs.size(); ++i) {
      if (tails[i]) {
        ++res.trailers;
        const int64_t body = lens[i] - tails[i];
        if (verify)
          zitems.push_back(gpu::DeviceChecksum::Item{ws.packed.as<uint8_t>() + zoff, body, name_of(in_runs[i]), true,
                                                    ifile_stored_checksum(ptrs[i] + body)});
      }
      zoff += lens[i];
    }
    if (!zitems.empty()) {
      ws.checksum.reset();
      ws.checksum.launch(std::move(zitems), s);
      ws.checksum.finish(s, false);
      verified();
    }
  } else if (decode_on_device) {
    ws.decoder.decode(codec, plan, ws.packed.as<uint8_t>(), in.as<uint8_t>(), s);
    res.decoded_blocks = (int64_t)plan.descs.size();
  }
  host_raw.clear();
  gpu::GenericMergeResult r = merge_runs(runs, bytes, out.as<uint8_t>(), total, timed);
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
