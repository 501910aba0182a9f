// NetMerger GPU backend, device fetch (mapred.uda.gpu.fetch=device): the providers answer FETCH with
// descriptors of partitions resident in their HBM store; the task maps them and merges in place, and
// fetches the bytes of the partitions a provider declined. See gpu_merge_staged.cc for the staged path.
#include <fcntl.h>
#include <sys/stat.h>
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <ctime>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <future>
#include <random>
#include <set>
#include <thread>

#include "../gpu/block_decoder.h"
#include "../gpu/device_ptr.h"
#include "../gpu/device_reduce.h"
#include "../gpu/device_engine.h"
#include "../gpu/fixed_delivery.h"
#include "../gpu/generic_merger.h"
#include "../gpu/generic_rounds.h"
#include "../gpu/hbm_ledger.h"
#include "../gpu/sdma.h"
#include "reduce_task.h"
#include "gpu_workspace.h"
#include "uda/aio.h"
#include "uda/fault.h"
#include "uda/compare.h"
#include "uda/ifile.h"
#include "uda/log.h"
#include "uda/safe_file.h"
#include "uda/topology.h"
#include "uda/trace.h"

namespace uda {

void ReduceTask::release_descriptors(const std::set<std::string>& hosts, const std::string& holder) {
  if (hosts.empty() || !transport_) return;
  struct Wait {  // outlives this call if a provider answers late
    std::mutex m;
    std::condition_variable c;
    size_t left = 0;
  };
  auto w = std::make_shared<Wait>();
  w->left = hosts.size();
  for (const auto& h : hosts) {
    FetchRequest req;
    req.job_id = init_.job_id;
    req.map_id = "*";
    req.reduce_id = 0;
    req.buf_len = kDescriptorRelease;
    req.holder = holder;
    fetch_begin();
    transport_->fetch(h, req, nullptr, [this, w](const FetchAck&) {
      {
        std::lock_guard<std::mutex> g(w->m);
        --w->left;
        w->c.notify_all();
      }
      fetch_end();
    });
  }
  std::unique_lock<std::mutex> lk(w->m);
  // a provider that does not answer keeps the references until its backstop drops them
  if (!w->c.wait_for(lk, std::chrono::seconds(10), [&] { return w->left == 0; }))
    throw UdaError("descriptor release not acknowledged by " + std::to_string(w->left) + " provider(s)");
}

// The partitions a device-fetch task gets no usable descriptor for (the provider's HBM store is full or
// off, or the descriptor cannot be mapped here). Two sources:
//  * the MOF file itself, when the provider runs on this node and named the file in its answer, and the
//    file is a regular file of this process's user (mapred.uda.gpu.fetch.local.read, default on; never for
//    a confined task): pread into pinned slots, one copy out of the page cache;
//  * otherwise the provider, over the transport: three requests of `chunk` bytes in flight per worker.
// `streams` workers (mapred.uda.gpu.fetch.bytes.streams, default 4) take partitions in turn; every landed
// chunk goes on to the device (H2D on the worker's stream) while the next ones come in. The round-5 loop
// had one request of the task's buffer size (1 MiB) in flight at a time: a round trip per MiB, 3.3 GB/s
// per task, 19.6 GB/s for a node of 15 tasks with 42.9 GB of 62.4 GB declined per wave; pipelined TCP
// 24.0 (profiles/r6/r6j_*, r6k_nodefiles62_store20.log). Over TCP every byte is copied twice by the CPU
// (the provider's sendfile, the reducer's receive) next to the consumers' own copies. The reference's
// fetcher keeps its requests in flight the same way (Segment::send_request, src/Merger/StreamRW.cc).
bool mof_host_is_local(const std::string& spec) {
  std::string h = spec;
  if (const size_t c = h.rfind(':'); c != std::string::npos && h.find(':') == c) h = h.substr(0, c);
  if (h == "127.0.0.1" || h == "localhost" || h == "::1" || h.empty()) return true;
  char me[256] = {0};
  if (::gethostname(me, sizeof(me) - 1) != 0) return false;
  const std::string m = me;
  return h == m || h == m.substr(0, m.find('.')) || m == h.substr(0, h.find('.'));
}

int open_local_mof(const std::string& path, int64_t off, int64_t len) {
  if (path.empty() || path[0] != '/') return -1;
  const int fd = ::open(path.c_str(), O_RDONLY | O_NOFOLLOW | O_CLOEXEC);
  if (fd < 0) return -1;
  struct stat sb;
  if (::fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_uid != ::geteuid() || sb.st_size < off + len) {
    ::close(fd);
    return -1;
  }
  return fd;
}

int64_t ReduceTask::fetch_declined_bytes(int device, const std::vector<DeclinedPart>& parts, gpu::DeviceBuffer& dst,
                                         std::vector<const uint8_t*>* where, int64_t* local) {
  const size_t n = parts.size();
  std::vector<int64_t> at(n + 1, 0);
  for (size_t k = 0; k < n; ++k) at[k + 1] = at[k] + ((parts[k].len + 255) & ~(int64_t)255);
  DeviceWorkspace::ensure(dst, at[n]);
  uint8_t* base = dst.as<uint8_t>();
  where->assign(n, nullptr);
  for (size_t k = 0; k < n; ++k) (*where)[k] = base + at[k];
  const int streams = (int)std::clamp<int64_t>(host_->conf_i64("mapred.uda.gpu.fetch.bytes.streams", 4), 1, 16);
  int64_t chunk = std::max<int64_t>(buffer_size_, host_->conf_i64("mapred.uda.gpu.fetch.bytes.chunk", 8ll << 20));
  chunk = (chunk + 4095) & ~(int64_t)4095;
  const bool local_ok = !sandbox_.enabled && host_->conf_i64("mapred.uda.gpu.fetch.local.read", 1) != 0;
  constexpr int kSlots = 3;
  std::atomic<size_t> next{0};
  std::atomic<int64_t> fetched{0}, read_here{0};
  std::mutex em;
  std::string err;
  auto failed = [&] {
    std::lock_guard<std::mutex> g(em);
    return !err.empty();
  };
  auto worker = [&] {
    struct Slot {
      gpu::PinnedPool::Block b;
      hipEvent_t ev = nullptr;
      bool h2d = false;   // an H2D from this slot may still be reading it
      bool busy = false;  // a request into this slot is in flight
      bool done = false;
      int64_t off = 0, want = 0;
      FetchAck a;
    };
    Slot sl[kSlots];
    std::mutex m;
    std::condition_variable cv;
    hipStream_t hs = nullptr;
    int fd = -1;
    auto drain = [&] {  // every request answered (their callbacks touch sl), every H2D done
      std::unique_lock<std::mutex> lk(m);
      cv.wait(lk, [&] {
        for (auto& x : sl)
          if (x.busy && !x.done) return false;
        return true;
      });
      lk.unlock();
      if (hs) (void)hipStreamSynchronize(hs);
    };
    auto reuse = [&](Slot& x) {  // the slot's previous H2D has read it
      if (x.h2d) {
        HIP_CHECK(hipEventSynchronize(x.ev));
        x.h2d = false;
      }
    };
    auto to_device = [&](Slot& x, uint8_t* dev) {
      HIP_CHECK(hipMemcpyAsync(dev + x.off, x.b.p, (size_t)x.want, hipMemcpyHostToDevice, hs));
      HIP_CHECK(hipEventRecord(x.ev, hs));
      x.h2d = true;
      fetched += x.want;
    };
    try {
      HIP_CHECK(hipSetDevice(device));
      hs = gpu::pooled_stream();
      for (auto& x : sl) {
        x.b = gpu::PinnedPool::instance().acquire((size_t)chunk);
        HIP_CHECK(hipEventCreateWithFlags(&x.ev, hipEventDisableTiming));
      }
      for (;;) {
        const size_t k = next.fetch_add(1);
        if (k >= n || failed() || stop_) break;
        const DeclinedPart& d = parts[k];
        const FetchParams& f = d.f;
        const int64_t L = d.len;
        uint8_t* dev = base + at[k];
        fd = local_ok && mof_host_is_local(f.host) ? open_local_mof(d.path, d.file_off, L) : -1;
        if (fd >= 0) {
          for (int64_t off = 0, s = 0; off < L; s = (s + 1) % kSlots) {
            Slot& x = sl[s];
            reuse(x);
            x.off = off;
            x.want = std::min(chunk, L - off);
            for (int64_t got = 0; got < x.want;) {
              const ssize_t r = ::pread(fd, x.b.p + got, (size_t)(x.want - got), (off_t)(d.file_off + off + got));
              if (r < 0 && errno == EINTR) continue;
              if (r <= 0)
                throw UdaError("reading " + d.path + " for " + f.map_id + ": " + (r < 0 ? strerror(errno) : "short file"));
              got += r;
            }
            to_device(x, dev);
            read_here += x.want;
            off += x.want;
          }
          ::close(fd);
          fd = -1;
          continue;
        }
        int64_t issue_off = 0;
        int outstanding = 0, head = 0, tail = 0;  // slots in request order: tail (oldest) .. head
        auto issue = [&](int s) {
          Slot& x = sl[s];
          reuse(x);
          FetchRequest req;
          req.job_id = f.job_id;
          req.map_id = f.map_id;
          req.reduce_id = f.reduce_id;
          req.fetched = issue_off;
          req.buf_len = chunk;
          {
            std::lock_guard<std::mutex> g(m);
            x.busy = true;
            x.done = false;
            x.off = issue_off;
            x.want = std::min(chunk, L - issue_off);
          }
          issue_off += x.want;
          ++outstanding;
          fetch_begin();
          transport_->fetch(f.host, req, x.b.p, [&, s](const FetchAck& a) {
            {
              // notify under the lock: once drain() sees every answer the worker's frame (m, cv) goes away
              std::lock_guard<std::mutex> g(m);
              sl[s].a = a;
              sl[s].done = true;
              cv.notify_all();
            }
            fetch_end();
          });
        };
        while (outstanding < kSlots && issue_off < L) {
          issue(head);
          head = (head + 1) % kSlots;
        }
        while (outstanding > 0) {
          Slot& x = sl[tail];
          {
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [&] { return x.done; });
            x.busy = false;
          }
          --outstanding;
          if (x.a.status != 0) throw UdaError("fetch of " + f.map_id + " failed: " + x.a.error);
          if (x.a.sent != x.want || x.a.part_len != L)
            throw UdaError("fetch of " + f.map_id + ": provider sent " + std::to_string(x.a.sent) + " bytes of a " +
                           std::to_string(x.a.part_len) + "-byte partition at offset " + std::to_string(x.off) +
                           " (expected " + std::to_string(x.want) + " of " + std::to_string(L) + ")");
          to_device(x, dev);
          tail = (tail + 1) % kSlots;
          if (issue_off < L) {
            issue(head);
            head = (head + 1) % kSlots;
          }
        }
      }
    } catch (const std::exception& e) {
      std::lock_guard<std::mutex> g(em);
      if (err.empty()) err = e.what();
    }
    if (fd >= 0) ::close(fd);
    drain();
    for (auto& x : sl) {
      if (x.ev) (void)hipEventDestroy(x.ev);
      if (x.b.p) gpu::PinnedPool::instance().release(x.b);
    }
    if (hs) gpu::return_stream(hs);
  };
  std::vector<std::thread> ts;
  const int nw = (int)std::min<size_t>((size_t)streams, n);
  for (int i = 1; i < nw; ++i) ts.emplace_back(worker);
  worker();
  for (auto& t : ts) t.join();
  if (!err.empty()) throw UdaError(err);
  if (stop_) throw UdaError("reduce task stopped during fetch");
  *local = read_here.load();
  return fetched.load();
}

// GPU backend, device fetch (mapred.uda.gpu.fetch=device, uncompressed map outputs): every FETCH is
// a descriptor fetch, so partitions the provider holds in HBM are merged where they live (same
// process: the address; another process on the node: an IPC mapping) and never cross PCIe on the
// way in. MOFs that are not device-resident are fetched as bytes and copied to the device.
// TeraSort-shaped inputs go through the key-range-round FIXED10 merge with SDMA delivery
// (device_reduce.cc); other key classes through the generic merge tree.
// Reference: start_fetch_req / RDMA WRITE into the reducer buffer (src/DataNet/RDMAClient.cc:559-600,
// src/DataNet/RDMAServer.cc:537-631) and merge_online (src/Merger/MergeManager.cc:184-193).
bool ReduceTask::merge_gpu_device(bool probe) {
  join_prewarm();
  if (gpu::device_count() <= 0) throw UdaError("mapred.uda.merge.backend=gpu but no HIP device is visible");
  // The task's device memory mostly comes from pooled workspaces sized by earlier tasks, so a
  // DeviceBuffer allocation may never happen in this task: the injected device-allocation failure
  // (UDA_FAULT_DEVICE_ALLOC) also counts the task taking its workspaces.
  if (fault_hit("DEVICE_ALLOC")) throw UdaError("injected device allocation failure (GPU merge workspaces)");
  auto t0 = std::chrono::steady_clock::now();
  auto boot_ms = [] {
    timespec ts{};
    clock_gettime(CLOCK_BOOTTIME, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec / 1e6;
  };
  {
    std::lock_guard<std::mutex> g(st_mu_);
    st_.merge_start_boot_ms = boot_ms();
  }
  const int maps = init_.num_maps;
  const int device = device_;
  HIP_CHECK(hipSetDevice(device));
  HIP_PENDING("the device fetch");
  StreamGuard sg;
  sg.s = gpu::pooled_stream();
  hipStream_t s = sg.s;
  // Descriptors are references the providers keep for this task (gpu/mof_cache.h): released when the
  // task is done with them -- its merge finished, or it failed -- after the device has stopped
  // reading the partitions (the merge stream is synchronized first).
  const std::string holder = gpu::reducer_holder_id(init_.reduce_task_id);
  struct DescRelease {
    ReduceTask* t;
    StreamGuard& sg;
    const std::string& holder;
    std::vector<std::string> descs;
    std::set<std::string> hosts;
    ~DescRelease() {
      if (sg.s) (void)hipStreamSynchronize(sg.s);
      for (const auto& d : descs) gpu::release_device_descriptor(d);
      try {
        t->release_descriptors(hosts, holder);
      } catch (const std::exception& e) {
        UDA_LOG(kWarn, "releasing descriptors: %s", e.what());
      }
    }
  } desc_release{this, sg, holder, {}, {}};
  struct Part {
    const uint8_t* dptr = nullptr;
    int64_t part_len = 0;
    int64_t raw_len = 0;  // the index's rawLength, as the provider answered it (<= 0: it did not say)
    std::string map_id;
  };
  std::vector<std::unique_ptr<Part>> parts;
  int64_t host_bytes = 0, descriptors = 0, unmapped = 0;
  // partitions answered "not device-resident" (or with a descriptor this process cannot map): their
  // bytes are fetched once every descriptor answer is in (fetch_declined, below)
  std::vector<DeclinedPart> declined;
  std::vector<size_t> declined_part;  // index into parts

  // ---- fetch phase: descriptors for every MOF as its FETCH arrives
  int resolved = 0;
  while (resolved < maps) {
    std::vector<FetchParams> batch;
    const auto tw = std::chrono::steady_clock::now();
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] { return stop_ || !fetch_list_.empty(); });
      if (stop_) throw UdaError("reduce task stopped during fetch");
      while (!fetch_list_.empty()) {
        batch.push_back(fetch_list_.front());
        fetch_list_.pop_front();
      }
    }
    const auto ta = std::chrono::steady_clock::now();
    if (resolved == 0) {
      std::lock_guard<std::mutex> g(st_mu_);
      st_.fetch_sent_boot_ms = boot_ms();
    }
    std::vector<FetchAck> acks(batch.size());
    std::mutex m;
    std::condition_variable c;
    size_t left = batch.size();
    for (size_t i = 0; i < batch.size(); ++i) {
      FetchRequest req;
      req.job_id = batch[i].job_id;
      req.map_id = batch[i].map_id;
      req.reduce_id = batch[i].reduce_id;
      req.buf_len = kDescriptorFetch;
      req.holder = holder;
      desc_release.hosts.insert(batch[i].host);
      fetch_begin();
      transport_->fetch(batch[i].host, req, nullptr, [&, i](const FetchAck& a) {
        std::lock_guard<std::mutex> g(m);
        acks[i] = a;
        --left;
        c.notify_all();
        fetch_end();
      });
    }
    {
      std::unique_lock<std::mutex> lk(m);
      c.wait(lk, [&] { return left == 0; });
    }
    {
      std::lock_guard<std::mutex> g(st_mu_);
      st_.fetch_cmd_wait_ms += std::chrono::duration<double, std::milli>(ta - tw).count();
      st_.fetch_ack_wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta).count();
    }
    if (probe && resolved == 0 && descriptors == 0) {
      // auto mode: the first answers decide; host-resident map outputs keep the staged path
      bool any_device = false;
      for (const auto& a : acks) any_device |= a.status == 0 && gpu::is_device_descriptor(a.path);
      if (!any_device) {
        std::lock_guard<std::mutex> g(mu_);
        for (auto it = batch.rbegin(); it != batch.rend(); ++it) fetch_list_.push_front(*it);
        return false;
      }
    }
    for (size_t i = 0; i < batch.size(); ++i) {
      const FetchAck& a = acks[i];
      auto part = std::make_unique<Part>();
      part->raw_len = a.raw_len;
      part->map_id = batch[i].map_id;
      std::string why;
      const uint8_t* dp = nullptr;
      const auto tm = std::chrono::steady_clock::now();
      if (a.status == 0 && gpu::is_device_descriptor(a.path)) {
        dp = gpu::try_resolve_device_descriptor(a.path, device, &why);
        std::lock_guard<std::mutex> g(st_mu_);
        st_.descriptor_map_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tm).count();
      }
      if (dp != nullptr) {
        part->dptr = dp;
        part->part_len = a.part_len;
        desc_release.descs.push_back(a.path);
        ++descriptors;
      } else if (a.status == 0 && gpu::is_device_descriptor(a.path)) {
        // not mappable here (another node, no IPC handle, import failure): fetch its bytes
        UDA_LOG(kInfo, "descriptor of %s not usable (%s): fetching bytes", batch[i].map_id.c_str(), why.c_str());
        if (unmapped == 0) {
          std::lock_guard<std::mutex> g(st_mu_);
          st_.unmapped_reason = why;
        }
        if (a.part_len < kEofBytes)
          throw UdaError("fetch of " + batch[i].map_id + ": descriptor answer carries no partition length");
        part->part_len = a.part_len;
        declined.push_back(DeclinedPart{batch[i], a.part_len, std::string(), 0});
        declined_part.push_back(parts.size());
        ++unmapped;
      } else if (a.status == kNotDeviceResident) {
        // every partition holds at least the IFile EOF marker: a length of 0 is a provider that did not say
        if (a.part_len < kEofBytes)
          throw UdaError("fetch of " + batch[i].map_id + ": declined descriptor fetch carries no partition length (" +
                         std::to_string(a.part_len) + ")");
        part->part_len = a.part_len;
        declined.push_back(DeclinedPart{batch[i], a.part_len, a.path, a.mof_offset});
        declined_part.push_back(parts.size());
      } else {
        throw UdaError("fetch of " + batch[i].map_id + " failed: " + (a.status ? a.error : "no device descriptor"));
      }
      parts.push_back(std::move(part));
      resolved++;
      note_map_fetched(parts.back()->part_len);
    }
  }
  double fetch_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  HIP_PENDING("the end of the descriptor fetch");
  {
    std::lock_guard<std::mutex> g(st_mu_);
    st_.device_descriptors = descriptors;
    st_.unmapped_descriptors = unmapped;
  }

  auto sink = [&](const uint8_t* p, int64_t len) -> int {
    if (stop_) throw UdaError("reduce task stopped during merge");
    const int r = host_->data_from_uda(p, (int32_t)len);
    std::lock_guard<std::mutex> g(st_mu_);
    if (st_.buffers == 0)
      st_.first_data_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st_.buffers++;
    st_.bytes_delivered += len;
    return r;
  };
  int64_t in_bytes = 0;
  for (const auto& p : parts) in_bytes += p->part_len;
  PoolLease<DeviceWorkspace> ws_lease{device, DevicePool<DeviceWorkspace>::get().acquire_fit(
                                                  device, in_bytes, [] { return std::make_unique<DeviceWorkspace>(); })};
  DeviceWorkspace& ws = *ws_lease.obj;
  ws.reset_stats();
  HIP_PENDING("the merge workspace");
  int64_t local_bytes = 0;
  if (!declined.empty()) {
    const auto tf = std::chrono::steady_clock::now();
    // the node's tasks take turns (FIFO, mapred.uda.gpu.fetch.bytes.slots at once; 0 = no limit): served
    // in turn, the first tasks' bytes are in and their merges deliver while later tasks still fetch;
    // all at once, every task's bytes landed late together and the link idled until then
    GateLease bgate;
    bgate.which = 2;
    if (const int slots = (int)host_->conf_i64("mapred.uda.gpu.fetch.bytes.slots", 4); slots > 0) {
      if (!DeviceGate::get(2).acquire(device, slots, [&] { return stop_.load(); }))
        throw UdaError("reduce task stopped while waiting for its turn to fetch bytes");
      bgate.device = device;
    }
    const double tg = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf).count();
    std::vector<const uint8_t*> where;
    host_bytes = fetch_declined_bytes(device, declined, ws.fetched, &where, &local_bytes);
    for (size_t k = 0; k < declined.size(); ++k) parts[declined_part[k]]->dptr = where[k];
    fetch_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf).count();
    std::lock_guard<std::mutex> g(st_mu_);
    st_.gpu_gate_wait_ms += tg;
  }
  {
    std::lock_guard<std::mutex> g(st_mu_);
    st_.host_fetched_bytes = host_bytes;
    st_.local_read_bytes = local_bytes;
  }
  // IFile checksum trailers (uda/ifile.h). Every partition has its device address now: the trailers are
  // stripped here, where the parts' lengths are set, so everything below sees what it sees without them,
  // and (mapred.uda.ifile.checksum=auto) one batched CRC launch over the partitions as fetched goes on the
  // task's stream ahead of the decode and the merge. Its result is read at the first synchronize of that
  // stream the task makes anyway; no record is delivered before. A job without trailers launches nothing.
  const bool verify = checksum_ == ChecksumMode::kAuto;
  int64_t trailers = 0;
  auto launch_checksums = [&](const std::vector<int>& tails) {
    std::vector<gpu::DeviceChecksum::Item> items;
    for (size_t i = 0; i < parts.size(); ++i) {
      if (!tails[i]) continue;
      ++trailers;
      parts[i]->part_len -= tails[i];
      if (verify) items.push_back(gpu::DeviceChecksum::Item{parts[i]->dptr, parts[i]->part_len, parts[i]->map_id, false, 0});
    }
    if (!items.empty()) ws.checksum.launch(std::move(items), s);
  };
  // synced: s has been synchronized since the launch
  auto finish_checksums = [&](bool synced) {
    if (ws.checksum.pending()) {
      ws.checksum.finish(s, synced);
      note_checksum(ws.checksum.partitions(), ws.checksum.bytes(), ws.checksum.ms());
    } else if (trailers > 0 && !verify) {
      note_checksum(0, 0);
    }
  };
  if (codec_ == Codec::kNone) {
    std::vector<int> tails;
    for (const auto& p : parts) tails.push_back(ifile_trailer_bytes(p->raw_len, p->part_len));
    launch_checksums(tails);
  }
  // HBM admission (gpu/hbm_ledger.h): the task's device working set -- decoded partitions, the
  // key-range round's output slots and merge tables -- is reserved before it is allocated, under the
  // device's byte budget shared with the provider's store and every other task on the node. A round
  // that could never fit is halved until it does; a task that fits later waits (FIFO) for it.
  gpu::HbmLedger& ledger = gpu::HbmLedger::get();
  std::unique_ptr<gpu::HbmLedger::Reservation> hbm_res;
  int64_t round_bytes = host_->conf_i64("mapred.uda.gpu.round.bytes", 2ll << 30);
  auto admit = [&](int64_t fixed, const std::function<int64_t(int64_t)>& round_ws) {
    const int64_t hr = ledger.headroom(device);
    while (round_bytes > (64ll << 20) && fixed + round_ws(round_bytes) > hr) round_bytes /= 2;
    hbm_res = ledger.reserve(device, std::max<int64_t>(0, fixed + round_ws(round_bytes)), [&] { return stop_.load(); });
    std::lock_guard<std::mutex> g(st_mu_);
    st_.hbm_wait_ms += hbm_res->wait_ms();
    st_.hbm_reserved = hbm_res->granted();
    st_.round_bytes = round_bytes;
  };
  // ---- compressed map outputs: F6 block decode straight from the partitions (descriptors or fetched
  // bytes) into the workspace; the framing is walked on the device
  if (codec_ != Codec::kNone) {
    const auto td = std::chrono::steady_clock::now();
    std::vector<const uint8_t*> cp;
    std::vector<int64_t> cl;
    for (const auto& p : parts) {
      cp.push_back(p->dptr);
      cl.push_back(p->part_len);
    }
    gpu::BlockPlan bp;
    std::vector<int64_t> roff;
    int64_t blocks = 0;
    // (the framing walk finds the trailers; the checksum kernels go between its two passes, and the second
    // pass's synchronize brings their result)
    std::vector<int> tails;
    // zlib (DefaultCodec) and gzip (GzipCodec): a partition is one stream with no framing, so there is nothing to walk and no
    // per-round decode; the index's raw lengths lay the outputs out, and the trailers are found by the decode
    gpu::StreamPlan zplan;
    bool dev_inflate = false;
    int64_t streams = 0;
    if (is_stream_codec(codec_)) {
      std::vector<int64_t> raws;
      for (const auto& p : parts) raws.push_back(p->raw_len);
      dev_inflate = gpu::plan_zlib_streams(cp, cl, raws, &zplan);
    }
    const bool dev_frames = !is_stream_codec(codec_) &&
                            gpu::plan_block_streams_device(codec_, cp, cl, &bp, ws.frame_scratch, ws.frame_descs, s,
                                                           &tails, launch_checksums);
    if (dev_frames) {
      finish_checksums(!bp.descs.empty());
      for (size_t i = 0; i < parts.size(); ++i)
        if (tails[i] && parts[i]->raw_len > 0 && bp.raw_offset[i + 1] - bp.raw_offset[i] != parts[i]->raw_len)
          throw UdaError("compressed map output " + parts[i]->map_id + " decodes to " +
                         std::to_string(bp.raw_offset[i + 1] - bp.raw_offset[i]) + " bytes, its index says " +
                         std::to_string(parts[i]->raw_len));
    }
    // TeraSort-shaped partitions: decode per key-range round, only the blocks each round covers, so the
    // task's device memory is round-sized instead of its decoded partitions (DecompressorWrapper decodes
    // block by block next to the merge too, src/Merger/DecompressorWrapper.cc:85-114)
    if (dev_frames && kind_ == KeyKind::kText && combine_ == CombineOp::kNone &&
        host_->conf_i64("mapred.uda.gpu.decode.stream", 1) != 0) {
      gpu::DeviceReduceConfig cfg;
      cfg.device = device;
      cfg.kv_buf_bytes = kv_buf_size_;
      cfg.round_bytes = round_bytes;
      cfg.pack_version = delivery_pack_;
      cfg.piece_bytes = delivery_piece_bytes_;
      cfg.stop = [&] { return stop_.load(); };
      // the node's tasks take turns for each round's block decode (FIFO, this many at once; 0 = no
      // limit). One round's decode (a wave per 256 KiB block, ~8k blocks) leaves the device idle: 130 GB
      // LZO 38.7 GB/s with one at a time, 45.7 with two, 49.3 with three; Snappy 54.0 / 53.9 / 53.3,
      // link-bound (profiles/r5/r5{j,k,l}_*130*.log)
      if (const int slots = (int)host_->conf_i64("mapred.uda.gpu.decode.stream.slots", 3); slots > 0) {
        cfg.decode_turn = [this, device, slots] {
          return DeviceGate::get(1).acquire(device, slots, [&] { return stop_.load(); });
        };
        cfg.decode_done = [device] { DeviceGate::get(1).release(device); };
      }
      bool streamed = false;
      const gpu::DeviceReduceStats ds = gpu::device_reduce_fixed_blocks(cfg, (int)codec_, bp, sink, &streamed);
      if (streamed) {
        std::lock_guard<std::mutex> g(st_mu_);
        st_.hbm_wait_ms += ds.hbm_wait_ms;
        st_.gpu_gate_wait_ms += ds.decode_wait_ms;
        st_.hbm_reserved = ds.hbm_reserved;
        st_.round_bytes = ds.round_bytes;
        st_.records = ds.records;
        st_.rpq_rounds = ds.rounds;
        st_.device_decoded_blocks += ds.decoded_blocks;
        st_.gpu_device_ms = ds.plan_ms + ds.merge_wait_ms;
        st_.gpu_d2h_wait_ms = ds.d2h_wait_ms;
        st_.gpu_sink_ms = ds.sink_ms;
        st_.gpu_d2h_bytes = ds.d2h_bytes;
        st_.gpu_packed_pieces = ds.packed_pieces;
        st_.gpu_raw_pieces = ds.raw_pieces;
        st_.gpu_unpack_ms = ds.unpack_ms;
        st_.fetch_ms = fetch_ms;
        st_.merge_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - fetch_ms;
        st_.merge_path = "device-fixed10-stream";
        ws_lease.clean = true;
        return true;
      }
    }
    if (dev_frames || dev_inflate) {
      // decode output and the merge's rounds at once: a task holding its decoded partitions must
      // not then wait for merge memory behind tasks doing the same
      const int64_t raw = dev_inflate ? zplan.raw_total : bp.raw_total;
      gpu::DeviceReduceConfig pcfg;  // the merge below packs its delivery: the packed slots count too
      pcfg.kv_buf_bytes = kv_buf_size_;
      pcfg.pack_version = delivery_pack_;
      pcfg.piece_bytes = delivery_piece_bytes_;
      // (zstd: what a zlib task takes plus the decoder's literal scratch, 128 KiB a partition)
      const int64_t lit = dev_inflate && codec_ == Codec::kZstd ? (int64_t)parts.size() * gpu::zstd_literal_scratch() : 0;
      admit(std::max<int64_t>(0, raw + raw / 8 + lit - (int64_t)ws.in.held()), [&](int64_t rb) {
        return gpu::fixed_round_ws_bytes(std::min(rb, raw), (int)parts.size(), &pcfg);
      });
    }
    // Decodes of concurrent tasks take turns (FIFO, mapred.uda.gpu.decode.slots at once, default 1;
    // 0 = no limit): a decode fills the device by itself, so running them in turn costs no decode
    // throughput, and the first tasks reach their merge and D2H delivery while later ones still
    // decode. All at once, every task finished decoding together and PCIe idled until then.
    GateLease dgate;
    dgate.which = 1;
    if (const int slots = (int)host_->conf_i64("mapred.uda.gpu.decode.slots", 1); slots > 0) {
      if (!DeviceGate::get(1).acquire(device, slots, [&] { return stop_.load(); }))
        throw UdaError("reduce task stopped while waiting for a device decode slot");
      dgate.device = device;
    }
    if (dev_inflate) {
      DeviceWorkspace::ensure(ws.in, zplan.raw_total);
      std::vector<std::string> ids;
      for (const auto& p : parts) ids.push_back(p->map_id);
      int bad = -1;
      std::string why;
      ws.inflater.decode(zplan, nullptr, ws.in.as<uint8_t>(), ids, s, &tails, &bad, &why, codec_);
      if (bad >= 0) {
        // a stream that does not decode has no known end. Where the task's other partitions carry a trailer,
        // so does this one: its CRC tells a partition damaged on its way (the checksum mismatch, as for every
        // other codec) from a stream that was written wrong (the decoder's own message)
        bool trailers_seen = false;
        for (int t : tails) trailers_seen = trailers_seen || t == kIFileChecksumBytes;
        if (verify && trailers_seen && cl[(size_t)bad] > kIFileChecksumBytes) {
          std::vector<int> only(parts.size(), 0);
          only[(size_t)bad] = kIFileChecksumBytes;
          launch_checksums(only);
          finish_checksums(false);
        }
        throw UdaError(why);
      }
      // only now are the tails known: the checksums run over the partitions as fetched and are read here,
      // before the merge below delivers a record
      launch_checksums(tails);
      finish_checksums(false);
      roff = zplan.raw_offset;
      streams = (int64_t)zplan.descs.size();
    } else if (dev_frames) {
      DeviceWorkspace::ensure(ws.in, bp.raw_total);
      ws.decoder.decode(codec_, bp, nullptr, ws.in.as<uint8_t>(), s);
      roff = bp.raw_offset;
      blocks = (int64_t)bp.descs.size();
    } else {  // framing that needs a decode (multi-chunk LZO or LZ4 blocks): decode on the host
      UDA_LOG(kInfo, "device decode: %s needs a host decode (%s)",
              is_stream_codec(codec_) ? "a partition of unknown or 2 GiB raw length" : "framing", codec_name(codec_));
      std::vector<std::vector<uint8_t>> raws;
      roff.assign(1, 0);
      for (size_t i = 0; i < cp.size(); ++i) {
        std::vector<uint8_t> c((size_t)cl[i]);
        if (cl[i] > 0) HIP_CHECK(hipMemcpy(c.data(), cp[i], (size_t)cl[i], hipMemcpyDefault));
        int tail = 0;  // (the bytes are decoded here, on the host: so is their checksum)
        std::vector<uint8_t> raw = host_decode_partition(codec_, c.data(), (int64_t)c.size(), &tail);
        if (tail) {
          ++trailers;
          const int64_t body = (int64_t)c.size() - tail;
          if (parts[i]->raw_len > 0 && (int64_t)raw.size() != parts[i]->raw_len)
            throw UdaError("compressed map output " + parts[i]->map_id + " decodes to " + std::to_string(raw.size()) +
                           " bytes, its index says " + std::to_string(parts[i]->raw_len));
          if (verify) {
            const uint32_t stored = ifile_stored_checksum(c.data() + body), got = crc32_ieee(c.data(), (size_t)body);
            if (stored != got) throw UdaError(ifile_checksum_mismatch(parts[i]->map_id, stored, got, body));
            note_checksum(1, body);
          }
        }
        roff.push_back(roff.back() + (int64_t)raw.size());
        raws.push_back(std::move(raw));
      }
      DeviceWorkspace::ensure(ws.in, roff.back());
      for (size_t i = 0; i < raws.size(); ++i)
        if (!raws[i].empty())
          HIP_CHECK(hipMemcpy(ws.in.as<uint8_t>() + roff[i], raws[i].data(), raws[i].size(), hipMemcpyHostToDevice));
    }
    for (size_t i = 0; i < parts.size(); ++i) {
      parts[i]->dptr = ws.in.as<uint8_t>() + roff[i];
      parts[i]->part_len = roff[i + 1] - roff[i];
    }
    HIP_CHECK(hipStreamSynchronize(s));  // (the merge below syncs it anyway): decode time on its own
    std::lock_guard<std::mutex> g(st_mu_);
    st_.device_decoded_blocks += blocks;
    st_.device_decoded_streams += streams;
    st_.gpu_decode_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - td).count();
  }
  // ---- TeraSort-shaped input: FIXED10 rounds straight over the partitions
  bool fixed = kind_ == KeyKind::kText && combine_ == CombineOp::kNone;  // a combiner takes the generic merge
  std::vector<gpu::RunDesc> runs;
  for (const auto& p : parts) {
    const int64_t rec_bytes = p->part_len - kEofBytes;
    if (rec_bytes < 0 || rec_bytes % gpu::kTeraRecordBytes != 0) fixed = false;
    gpu::RunDesc d;
    d.base = p->dptr;
    d.nbytes = std::max<int64_t>(rec_bytes, 0);
    d.nrec = d.nbytes / gpu::kTeraRecordBytes;
    d.offsets = nullptr;
    runs.push_back(d);
  }
  const bool fixed10 = fixed && gpu::runs_are_fixed10(runs, s);  // (synchronizes s)
  finish_checksums(fixed && !runs.empty());
  if (fixed10) {
    gpu::DeviceReduceConfig cfg;
    cfg.device = device;
    cfg.kv_buf_bytes = kv_buf_size_;
    cfg.round_bytes = round_bytes;
    cfg.pack_version = delivery_pack_;
    cfg.piece_bytes = delivery_piece_bytes_;
    cfg.stop = [&] { return stop_.load(); };
    gpu::DeviceReduceStats ds = gpu::device_reduce_fixed(cfg, runs, sink);
    std::lock_guard<std::mutex> g(st_mu_);
    if (!hbm_res) {
      st_.hbm_wait_ms += ds.hbm_wait_ms;
      st_.hbm_reserved = ds.hbm_reserved;
    }
    st_.round_bytes = ds.round_bytes;
    st_.records = ds.records;
    st_.rpq_rounds = ds.rounds;
    st_.gpu_device_ms = ds.plan_ms + ds.merge_wait_ms;
    st_.gpu_d2h_wait_ms = ds.d2h_wait_ms;
    st_.gpu_sink_ms = ds.sink_ms;
    st_.gpu_d2h_bytes = ds.d2h_bytes;
    st_.gpu_packed_pieces = ds.packed_pieces;
    st_.gpu_raw_pieces = ds.raw_pieces;
    st_.gpu_unpack_ms = ds.unpack_ms;
    st_.fetch_ms = fetch_ms;
    st_.merge_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - fetch_ms;
    st_.merge_path = "device-fixed10";
    ws_lease.clean = true;
    return true;
  }
  // ---- any other key class: the generic merge, reading the partitions where they live, in key-range
  // rounds of at most mapred.uda.gpu.round.bytes of input (generic_rounds.h), so the device working
  // set (output + ~80 B/record of merge metadata) is bounded by the round, not by the partition
  int64_t total = 0;
  std::vector<const uint8_t*> rptr;
  std::vector<int64_t> rlen;
  for (const auto& p : parts) {
    rptr.push_back(p->dptr);
    rlen.push_back(p->part_len);
    total += p->part_len;
  }
  // working set of a generic round of rb input bytes: two output slots + ~88 B of merge metadata per
  // record (records of >= 64 B) over what the pooled workspace already holds
  if (!hbm_res) {
    const int64_t have = (int64_t)(ws.out.held() + ws.out2.held()) + ws.merger.workspace_bytes();
    admit(0, [&](int64_t rb) {
      const int64_t b = std::min(rb, total);
      // (a combiner's group index and sums: 17 B per record more, 0.27 of the bytes at 64 B records)
      const double comb = combine_ != CombineOp::kNone ? 0.27 * (double)b : 0.0;
      // (a numeric kind's normalized keys: 8 B per record more, 0.125 of the bytes at 64 B records)
      const double norm = key_kind_numeric(kind_) ? 0.125 * (double)b : 0.0;
      return std::max<int64_t>(0, (int64_t)(2.25 * (double)b + 1.4 * (double)b + comb + norm) - have);
    });
  }
  if (total > round_bytes) {
    // a task holding more than a round (a skewed partition) is the job's long pole: its merge kernels
    // go first when the device is shared with the other tasks' merges
    int lo = 0, hi = 0;
    HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_CHECK(hipStreamSynchronize(s));
    gpu::return_stream(sg.s);
    sg.s = nullptr;
    sg.s = gpu::pooled_stream(hi);
    s = sg.s;
    // and its delivery pieces go over two SDMA engines instead of one: the link is shared per queued copy,
    // so while the other tasks deliver, this one's output keeps a larger share of it
    ws.out_ways = 2;
  }
  const gpu::GenericRoundsPlan rplan = gpu::plan_generic_rounds(rptr, rlen, (int)kind_, round_bytes, ws.rounds, s);
  // Round q merges into outs[q & 1] while a delivery thread streams round q-1 out (D2H pieces +
  // dataFromUda): the consumer's work (the reduce task's bound when one task holds most of the data)
  // never waits for the merge driver, and the merge reuses an output only after its delivery.
  DeviceWorkspace::ensure(ws.out, rplan.max_round_bytes);
  if (rplan.rounds > 1) DeviceWorkspace::ensure(ws.out2, rplan.max_round_bytes);
  gpu::DeviceBuffer* outs[2] = {&ws.out, rplan.rounds > 1 ? &ws.out2 : &ws.out};
  const int64_t kv = kv_buf_size_ - kEofBytes;
  std::vector<uint8_t> tail((size_t)kv_buf_size_ + kEofBytes);
  bool eof_sent = false;
  struct DJob {
    const uint8_t* src;
    std::vector<int64_t> cuts;
    bool last;          // the task's final records: the EOF marker goes after them
    bool end_of_round;  // the key-range round's output is fully handed over after this job
  };
  std::mutex dmu;
  std::condition_variable dcv;
  std::deque<DJob> djobs;
  int delivered = 0;  // key-range rounds fully delivered
  bool dstop = false;
  std::string derr;
  std::thread dthr([&] {
    try {
      bind_thread_to_cpus(gpu::device_consumer_cpus(device));  // the D2H ring and the consumer copies
      HIP_CHECK(hipSetDevice(device));
      for (;;) {
        DJob j;
        {
          const int64_t ti = trace::host_enabled() ? trace::now_ns() : 0;
          std::unique_lock<std::mutex> lk(dmu);
          dcv.wait(lk, [&] { return dstop || !djobs.empty(); });
          if (djobs.empty()) return;
          j = std::move(djobs.front());
          djobs.pop_front();
          if (ti) trace::host_event("gr_idle", (int64_t)(uintptr_t)&ws, 0, ti, trace::now_ns());
        }
        DeviceMergeOut m;
        m.cuts = std::move(j.cuts);
        const size_t nb = m.cuts.size() < 2 ? 0 : m.cuts.size() - 1;
        stream_out(ws, m, ws.copy_stream(), [&](const uint8_t* piece, size_t c0, size_t c1) {
          for (size_t x = c0; x < c1; ++x) {
            const uint8_t* p = piece + (m.cuts[x] - m.cuts[c0]);
            int64_t len = m.cuts[x + 1] - m.cuts[x];
            if (j.last && x + 1 == nb) {
              std::memcpy(tail.data(), p, (size_t)len);
              tail[(size_t)len] = tail[(size_t)len + 1] = 0xFF;
              p = tail.data();
              len += kEofBytes;
              eof_sent = true;
            }
            if (sink(p, len) != 0) throw UdaError("dataFromUda callback failed");
          }
        }, j.src);
        if (j.end_of_round) {
          std::lock_guard<std::mutex> g(dmu);
          ++delivered;
          dcv.notify_all();
        }
      }
    } catch (const std::exception& e) {
      std::lock_guard<std::mutex> g(dmu);
      derr = e.what();
      dstop = true;
      dcv.notify_all();
    }
  });
  struct DJoin {
    std::thread& t;
    std::mutex& mu;
    std::condition_variable& cv;
    bool& stop;
    ~DJoin() {
      {
        std::lock_guard<std::mutex> g(mu);
        stop = true;
      }
      cv.notify_all();
      if (t.joinable()) t.join();
    }
  } djoin{dthr, dmu, dcv, dstop};
  auto push = [&](DJob j) {
    std::lock_guard<std::mutex> g(dmu);
    if (!derr.empty()) throw UdaError("delivery failed: " + derr);
    djobs.push_back(std::move(j));
    dcv.notify_all();
  };
  DeviceMergeOut m;
  int64_t merge_rounds = 0;
  for (int q = 0; q < rplan.rounds; ++q) {
    {
      const int64_t tw = trace::host_enabled() ? trace::now_ns() : 0;
      std::unique_lock<std::mutex> lk(dmu);  // outs[q & 1] held round q - 2: delivered?
      dcv.wait(lk, [&] { return delivered >= q - 1 || !derr.empty(); });
      if (!derr.empty()) throw UdaError("delivery failed: " + derr);
      if (tw) trace::host_event("gr_slot_wait", (int64_t)(uintptr_t)&ws, q, tw, trace::now_ns());
    }
    std::vector<const uint8_t*> sp;
    std::vector<int64_t> sl;
    for (size_t k = 0; k < rptr.size(); ++k) {
      const int64_t b = rplan.at((int)k, q), e = rplan.at((int)k, q + 1);
      if (e > b) {
        sp.push_back(rptr[k] + b);
        sl.push_back(e - b);
      }
    }
    const bool last_outer = q + 1 == rplan.rounds;
    if (sp.empty()) {
      push(DJob{nullptr, {}, false, true});
      continue;
    }
    const uint8_t* dst = outs[q & 1]->as<uint8_t>();
    const auto tq = std::chrono::steady_clock::now();
    bool round_closed = false;
    gpu::GenericMergeResult r = ws.merger.merge(
        sp, sl, (int)kind_, outs[q & 1]->as<uint8_t>(), (int64_t)outs[q & 1]->size(), kv, s,
        [&](const std::vector<int64_t>& cuts, int64_t, bool last_inner) {
          push(DJob{dst, cuts, last_inner && last_outer, last_inner});
          round_closed = round_closed || last_inner;
        },
        merge_round_bytes_, combine_);
    // slices holding only EOF markers: the merge saw no records and never called back, but the
    // delivery thread still has to count this round as handed over
    if (!round_closed) push(DJob{nullptr, {}, false, true});
    m.records += r.records;
    m.records_in += r.records_in;
    merge_rounds += r.rounds;
    if (trace::host_enabled())
      trace::host_event("gr_merge", (int64_t)(uintptr_t)&ws, q,
                        trace::now_ns() - (int64_t)(std::chrono::steady_clock::now() - tq).count(), trace::now_ns());
    static const bool trace = std::getenv("UDA_DEVICE_REDUCE_TRACE") != nullptr;  // tools: per-round lines
    if (trace)
      std::fprintf(stderr, "[generic rounds] round %d/%d: %ld records merged in %.1f ms\n", q, rplan.rounds,
                   (long)r.records, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tq).count());
  }
  {
    std::unique_lock<std::mutex> lk(dmu);
    dcv.wait(lk, [&] { return delivered >= rplan.rounds || !derr.empty(); });
    if (!derr.empty()) throw UdaError("delivery failed: " + derr);
  }
  {
    std::lock_guard<std::mutex> g(st_mu_);
    st_.rpq_rounds = rplan.rounds;
    st_.gpu_ws_bytes = (int64_t)ws.out.size() + (rplan.rounds > 1 ? (int64_t)ws.out2.size() : 0) +
                       ws.merger.workspace_bytes();
    st_.gpu_device_ms = rplan.plan_ms;
    st_.gpu_d2h_wait_ms = ws.d2h_ms;
    st_.gpu_sink_ms = ws.sink_ms;
  }
  if (!eof_sent) {
    tail[0] = tail[1] = 0xFF;
    if (sink(tail.data(), kEofBytes) != 0) throw UdaError("dataFromUda callback failed");
  }
  HIP_CHECK(hipStreamSynchronize(s));
  ws_lease.clean = true;
  std::lock_guard<std::mutex> g(st_mu_);
  st_.records = m.records;
  st_.merge_rounds = merge_rounds;
  if (combine_ != CombineOp::kNone) {
    st_.combine_in_records = m.records_in;
    st_.combine_groups = m.records;
  }
  st_.fetch_ms = fetch_ms;
  st_.merge_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - fetch_ms;
  st_.merge_path = "device-generic";
  return true;
}

}  // namespace uda
