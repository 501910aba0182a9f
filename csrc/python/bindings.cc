// Python bindings (pybind11) for the native runtime: the "fake JVM" host used by tests and the
// bench drives the same C ABI / engine objects a JNI host would.
#include <map>
#include <memory>
#include <condition_variable>
#include <mutex>
#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <fcntl.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstring>
#include <random>

#include "block_decoder.h"
#include "block_rounds.h"
#include "device_engine.h"
#include "device_ptr.h"
#include "device_reduce.h"
#include "fixed_delivery.h"
#include "mof_cache.h"
#include "consumer/gpu_workspace.h"
#include "consumer/reduce_task.h"
#include "service/merge_service.h"
#include "exchange.h"
#include "api_bench.h"
#include "generic_merger.h"
#include "generic_rounds.h"
#include "j2c_sink.h"
#include "stream_decoder.h"
#include "stream_sampler.h"
#include "uda/aio.h"
#include "uda/codec.h"
#include "uda/datagen.h"
#include "uda/error.h"
#include "uda/hash.h"
#include "uda/ifile.h"
#include "uda/uda_bridge.h"
#include "uda/cmd.h"
#include "uda/compare.h"
#include "uda/log.h"
#include "uda/vint.h"
#include "uda/shm_group.h"
#include "uda/node_registry.h"
#include "uda/topology.h"
#include "uda/transport.h"
#include "../gpu/hbm_ledger.h"
#include "../gpu/kernels.h"
#include "codec/colpack.h"
#include <atomic>
#include <thread>

namespace py = pybind11;
using namespace uda;

namespace {

struct GpuNoise {  // start_gpu_noise / stop_gpu_noise
  std::atomic<bool> stop{false};
  std::thread thr;
  std::atomic<int64_t> ops{0};
};
GpuNoise* g_noise = nullptr;

py::dict stats_to_dict(const gpu::StepStats& s) {
  py::dict d;
  d["wall_ms"] = s.wall_ms;
  d["comm_ms"] = s.comm_ms;
  d["plan_ms"] = s.plan_ms;
  d["merge_ms"] = s.merge_ms;
  d["d2h_ms"] = s.d2h_ms;
  d["wait_out_ms"] = s.wait_out_ms;
  d["stage_ms"] = s.stage_ms;
  d["bytes_in"] = s.bytes_in;
  d["records"] = s.records;
  d["bytes_sent"] = s.bytes_sent;
  d["bytes_h2d"] = s.bytes_h2d;
  d["buffers"] = s.buffers;
  d["d2h_bytes"] = s.d2h_bytes;
  d["packed_pieces"] = s.packed_pieces;
  d["pack_delta_pieces"] = s.pack_delta_pieces;
  d["pack_stride_min"] = s.pack_stride_min;
  d["pack_stride_max"] = s.pack_stride_max;
  d["raw_pieces"] = s.raw_pieces;
  d["unpack_ms"] = s.unpack_ms;
  d["lead_in_ms"] = s.lead_in_ms;
  d["link_idle_ms"] = s.link_idle_ms;
  d["tail_ms"] = s.tail_ms;
  d["slot_wait_ms"] = s.slot_wait_ms;
  d["merge_passes"] = s.merge_passes;
  d["order_errors"] = s.order_errors;
  d["checksum"] = s.checksum;
  d["exchange_errors"] = s.exchange_errors;
  d["validated"] = s.validated;
  d["bad_layout"] = s.bad_layout;
  d["pre_merge_errors"] = s.pre_merge_errors;
  d["own_errors"] = s.own_errors;
  d["merge_errors"] = s.merge_errors;
  d["pre_d2h_errors"] = s.pre_d2h_errors;
  d["delivery_errors"] = s.delivery_errors;
  d["diag"] = s.diag;
  d["round_comm_ms"] = s.round_comm_ms;
  d["round_merge_ms"] = s.round_merge_ms;
  return d;
}

gpu::ShuffleConfig config_from_dict(const py::dict& d) {
  gpu::ShuffleConfig c;
  auto get = [&](const char* k, auto& field) {
    if (d.contains(k)) field = d[k].cast<std::decay_t<decltype(field)>>();
  };
  get("device", c.device);
  get("rank", c.rank);
  get("world", c.world);
  get("maps_per_rank", c.maps_per_rank);
  get("records_per_map", c.records_per_map);
  get("rounds", c.rounds);
  get("reducers", c.reducers);
  get("seed", c.seed);
  get("kv_buf_bytes", c.kv_buf_bytes);
  get("d2h_piece_bytes", c.d2h_piece_bytes);
  get("pinned_slots", c.pinned_slots);
  get("d2h_engines", c.d2h_engines);
  get("d2h", c.d2h);
  get("deliver_host", c.deliver_host);
  get("validate", c.validate);
  get("local_group", c.local_group);
  get("store", c.store);
  get("local_dirs", c.local_dirs);
  get("replan", c.replan);
  get("map_sort", c.map_sort);
  get("check_delivery", c.check_delivery);
  get("delivery_pack", c.delivery_pack);
  get("delivery_order", c.delivery_order);
  return c;
}

// Python host for the C ABI (the "fake JVM"): Python callables stand in for the UdaBridge.java
// static callbacks. Native threads take the GIL for each callback; bridge entry points release it.
struct PyBridge {
  py::object fetch_over, data_from_uda, get_path, get_conf, log, failure;
  uda_handle* h = nullptr;
  std::vector<std::shared_ptr<std::string>> keep;

  static PyBridge* self(void* ctx) { return static_cast<PyBridge*>(ctx); }
  static void t_fetch_over(void* ctx) {
    py::gil_scoped_acquire g;
    try {
      if (!self(ctx)->fetch_over.is_none()) self(ctx)->fetch_over();
    } catch (py::error_already_set& e) {
      e.discard_as_unraisable("fetch_over");
    }
  }
  static int t_data(void* ctx, const void* buf, int32_t len) {
    py::gil_scoped_acquire g;
    try {
      if (self(ctx)->data_from_uda.is_none()) return 0;
      // zero-copy like the JNI DirectByteBuffer: a read-only view valid only during the call
      py::memoryview mv = py::memoryview::from_memory(const_cast<void*>(buf), (py::ssize_t)len, true);
      py::object r = self(ctx)->data_from_uda(mv);
      mv.attr("release")();
      return r.is_none() ? 0 : r.cast<int>();
    } catch (py::error_already_set& e) {
      e.discard_as_unraisable("data_from_uda");
      return -1;
    }
  }
  static int t_get_path(void* ctx, const char* job, const char* map, int32_t reduce, uda_index_record* out) {
    py::gil_scoped_acquire g;
    try {
      if (self(ctx)->get_path.is_none()) return -1;
      py::object r = self(ctx)->get_path(std::string(job), std::string(map), reduce);
      if (r.is_none()) return -1;
      auto t = r.cast<py::tuple>();
      out->start_offset = t[0].cast<int64_t>();
      out->raw_length = t[1].cast<int64_t>();
      out->part_length = t[2].cast<int64_t>();
      std::string path = t[3].cast<std::string>();
      std::strncpy(out->path, path.c_str(), UDA_PATH_MAX - 1);
      return 0;
    } catch (py::error_already_set& e) {
      e.discard_as_unraisable("get_path");
      return -1;
    }
  }
  static int t_get_conf(void* ctx, const char* key, const char* dflt, char* out, int32_t outlen) {
    py::gil_scoped_acquire g;
    try {
      std::string v = dflt ? dflt : "";
      if (!self(ctx)->get_conf.is_none()) {
        py::object r = self(ctx)->get_conf(std::string(key), v);
        if (!r.is_none()) v = r.cast<std::string>();
      }
      int32_t n = (int32_t)std::min<size_t>(v.size(), (size_t)outlen - 1);
      std::memcpy(out, v.data(), (size_t)n);
      out[n] = 0;
      return n;
    } catch (py::error_already_set& e) {
      e.discard_as_unraisable("get_conf");
      return -1;
    }
  }
  static void t_log(void* ctx, const char* msg, int32_t sev) {
    py::gil_scoped_acquire g;
    try {
      if (!self(ctx)->log.is_none()) self(ctx)->log(std::string(msg), sev);
    } catch (py::error_already_set& e) {
      e.discard_as_unraisable("log");
    }
  }
  static void t_failure(void* ctx, const char* reason) {
    py::gil_scoped_acquire g;
    try {
      if (!self(ctx)->failure.is_none()) self(ctx)->failure(std::string(reason ? reason : ""));
    } catch (py::error_already_set& e) {
      e.discard_as_unraisable("failure");
    }
  }
  ~PyBridge() {
    if (h) {
      py::gil_scoped_release r;
      uda_destroy(h);
    }
  }
};

CombineOp combine_op_arg(const std::string& v) {
  CombineOp op;
  if (!combine_op_from_conf(v, &op)) throw py::value_error("unknown combine \"" + v + "\" (" + kCombineAllowed + ")");
  return op;
}

// The comparator kind of a key class under a mapred.uda.key.order value ("reference" or "hadoop").
KeyKind key_kind_arg(const std::string& key_class, const std::string& key_order = "reference") {
  KeyOrder order;
  if (!key_order_from_conf(key_order, &order))
    throw py::value_error("unknown key_order \"" + key_order + "\" (reference or hadoop)");
  const KeyKind kind = key_kind_from_class(key_class.c_str(), order);
  if (kind == KeyKind::kUnsupported) throw py::value_error("unsupported key class");
  return kind;
}

py::bytes cpu_merge_impl(const std::vector<std::string>& runs, const std::string& key_class, int64_t buf,
                         std::vector<int64_t>* lens, CombineOp combine = CombineOp::kNone,
                         const std::string& key_order = "reference") {
  KeyKind kind = key_kind_arg(key_class, key_order);
  MergeQueue q(kind);
  for (size_t i = 0; i < runs.size(); ++i) {
    auto seg = std::make_unique<MemorySegment>(reinterpret_cast<const uint8_t*>(runs[i].data()), runs[i].size());
    seg->index = (int)i;
    q.insert(std::move(seg));
  }
  KVWriter w(&q, kind, combine);
  std::string out;
  std::vector<uint8_t> b((size_t)buf);
  bool done = false;
  while (!done) {
    int64_t len = 0;
    done = w.fill(b.data(), buf, &len);
    out.append(reinterpret_cast<const char*>(b.data()), (size_t)len);
    lens->push_back(len);
  }
  return py::bytes(out);
}

// A block plan as Python sees it: ([(stream, src, src_end, dst, raw)], raw_offset, tails), src and src_end
// as offsets into the block's own stream. `base` is what the descriptors' src counts from (0: the streams
// back to back in one host buffer; a device address: the same layout in device memory).
py::tuple block_plan_tuple(const gpu::BlockPlan& plan, const std::vector<int64_t>& lens, int64_t base,
                           const std::vector<int>& tails, bool with_tails) {
  std::vector<int64_t> at(lens.size() + 1, 0);
  for (size_t i = 0; i < lens.size(); ++i) at[i + 1] = at[i] + lens[i];
  py::list descs;
  size_t k = 0;
  for (const auto& d : plan.descs) {
    // a stream's blocks are those with dst in [raw_offset[k], raw_offset[k + 1]) (every block has raw > 0)
    while (k + 1 < lens.size() && d.dst >= plan.raw_offset[k + 1]) ++k;
    descs.append(py::make_tuple((int64_t)k, d.src - base - at[k], d.src_end - base - at[k], d.dst, d.raw));
  }
  py::list ro, tl;
  for (int64_t v : plan.raw_offset) ro.append(v);
  if (with_tails)
    for (int v : tails) tl.append(v);
  return py::make_tuple(descs, ro, tl);
}

constexpr int64_t kStreamGuard = 256;

// The streams back to back in one device buffer (no alignment between them, as partitions lie in a MOF)
// with kStreamGuard bytes of 0xA5 behind the last.
void upload_streams(const std::vector<std::string>& streams, gpu::DeviceBuffer* buf, std::vector<const uint8_t*>* dptrs,
                    std::vector<int64_t>* lens) {
  std::string all;
  for (const auto& st : streams) all += st;
  all.append((size_t)kStreamGuard, (char)0xA5);
  buf->alloc(all.size());
  HIP_CHECK(hipMemcpy(buf->as(), all.data(), all.size(), hipMemcpyHostToDevice));
  size_t off = 0;
  for (const auto& st : streams) {
    dptrs->push_back(buf->as<uint8_t>() + off);
    lens->push_back((int64_t)st.size());
    off += st.size();
  }
}

void check_stream_guard(const gpu::DeviceBuffer& buf, const std::vector<int64_t>& lens) {
  int64_t data = 0;
  for (int64_t l : lens) data += l;
  std::string g((size_t)kStreamGuard, '\0');
  HIP_CHECK(hipMemcpy(&g[0], buf.as<uint8_t>() + data, g.size(), hipMemcpyDeviceToHost));
  for (char c : g)
    if ((uint8_t)c != 0xA5) throw UdaError("the guard bytes behind the compressed streams changed");
}

gpu::BlockKey block_key_of(const std::string& k) {
  if (k.size() != 10) throw py::value_error("a key is 10 bytes");
  gpu::BlockKey v;
  for (int i = 0; i < 8; ++i) v.hi = (v.hi << 8) | (uint8_t)k[(size_t)i];
  v.lo = (((uint64_t)(uint8_t)k[8] << 8) | (uint8_t)k[9]) << 48;
  return v;
}

py::bytes block_key_bytes(const gpu::BlockKey& v) {
  char k[10];
  for (int i = 0; i < 8; ++i) k[i] = (char)(v.hi >> (56 - 8 * i));
  k[8] = (char)(v.lo >> 56);
  k[9] = (char)(v.lo >> 48);
  return py::bytes(k, 10);
}

}  // namespace

PYBIND11_MODULE(_uda_native, m) {
  m.doc() = "MI355X-native UDA shuffle/merge runtime";

  // ---------------------------------------------------------------- common
  m.def("vint_encode", [](int64_t v) {
    uint8_t b[9];
    int n = vint_encode(v, b);
    return py::bytes(reinterpret_cast<char*>(b), n);
  });
  m.def("vint_decode", [](py::bytes data) {
    std::string s = data;
    int64_t v = 0;
    int n = vint_decode(reinterpret_cast<const uint8_t*>(s.data()), s.size(), &v);
    return py::make_tuple(v, n);
  });
  m.def("vint_size", &vint_size);
  m.def("vint_decode_size", &vint_decode_size);
  m.def("parse_cmd", [](const std::string& s) {
    HadoopCmd c;
    if (!parse_cmd(s, &c)) throw py::value_error("malformed command");
    return py::make_tuple(c.count, (int)c.header, c.params);
  });
  m.def("form_cmd", &form_cmd);
  m.def("parse_options", [](const std::vector<std::string>& args) {
    NetlevOptions o;
    std::string err;
    if (!parse_options(args, &o, &err)) throw py::value_error(err);
    py::dict d;
    d["wqes_per_conn"] = o.wqes_per_conn;
    d["data_port"] = o.data_port;
    d["online"] = o.online;
    d["mode"] = o.mode;
    d["log_dir"] = o.log_dir;
    d["trace_level"] = o.trace_level;
    d["buf_size"] = o.buf_size;
    return d;
  });
  m.def("key_kind", [](const std::string& cls) { return (int)key_kind_from_class(cls.c_str()); });
  // key_kind under a mapred.uda.key.order value; -1 for a class that order does not support
  m.def("key_kind_ordered", [](const std::string& cls, const std::string& key_order) {
    KeyOrder order;
    if (!key_order_from_conf(key_order, &order))
      throw py::value_error("unknown key_order \"" + key_order + "\" (reference or hadoop)");
    return (int)key_kind_from_class(cls.c_str(), order);
  }, py::arg("cls"), py::arg("key_order"));
  // the sortable word of a numeric key (uda/compare.h); ValueError for a key of the wrong length
  m.def("key_sortable", [](int kind, py::bytes key) {
    std::string k = key;
    bool ok = false;
    const uint64_t v = key_sortable((KeyKind)kind, reinterpret_cast<const uint8_t*>(k.data()), (int)k.size(), &ok);
    if (!ok) throw py::value_error(key_bad_length_message((KeyKind)kind, (int64_t)k.size(), "key_sortable"));
    return v;
  });
  m.def("key_compare", [](int kind, py::bytes a, py::bytes b) {
    std::string sa = a, sb = b;
    return key_compare((KeyKind)kind, reinterpret_cast<const uint8_t*>(sa.data()), (int)sa.size(),
                       reinterpret_cast<const uint8_t*>(sb.data()), (int)sb.size());
  });
  m.def("record_hash", [](py::bytes b) {
    std::string s = b;
    return record_hash(reinterpret_cast<const uint8_t*>(s.data()), (int64_t)s.size());
  });
  m.def("log_set_threshold", &log_set_threshold);

  m.def("version", &uda_version);

  // ---------------------------------------------------------------- codecs
  m.def("snappy_compress", [](py::bytes b) {
    std::string s = b;
    std::string out(snappy_max_compressed_length(s.size()), '\0');
    size_t n = snappy_compress((const uint8_t*)s.data(), s.size(), (uint8_t*)&out[0]);
    out.resize(n);
    return py::bytes(out);
  });
  m.def("snappy_decompress", [](py::bytes b, size_t cap) {
    std::string s = b;
    std::string out(cap, '\0');
    size_t n = 0;
    if (!snappy_decompress((const uint8_t*)s.data(), s.size(), (uint8_t*)&out[0], cap, &n))
      throw py::value_error("corrupt snappy data");
    out.resize(n);
    return py::bytes(out);
  });
  m.def("lzo1x_compress", [](py::bytes b) {
    std::string s = b;
    std::string out(lzo1x_max_compressed_length(s.size()), '\0');
    size_t n = lzo1x_compress((const uint8_t*)s.data(), s.size(), (uint8_t*)&out[0]);
    out.resize(n);
    return py::bytes(out);
  });
  m.def("lzo1x_decompress", [](py::bytes b, size_t cap) {
    std::string s = b;
    std::string out(cap, '\0');
    size_t n = 0;
    if (!lzo1x_decompress((const uint8_t*)s.data(), s.size(), (uint8_t*)&out[0], cap, &n))
      throw py::value_error("corrupt lzo1x data");
    out.resize(n);
    return py::bytes(out);
  });
  m.def("lz4_compress", [](py::bytes b) {
    std::string s = b;
    std::string out(lz4_max_compressed_length(s.size()), '\0');
    size_t n = lz4_compress((const uint8_t*)s.data(), s.size(), (uint8_t*)&out[0]);
    out.resize(n);
    return py::bytes(out);
  });
  m.def("lz4_decompress", [](py::bytes b, size_t cap) {
    std::string s = b;
    std::string out(cap, '\0');
    size_t n = 0;
    if (!lz4_decompress((const uint8_t*)s.data(), s.size(), (uint8_t*)&out[0], cap, &n))
      throw py::value_error("corrupt lz4 data");
    out.resize(n);
    return py::bytes(out);
  });
  // The D2H pieces of a delivery round in the copy thread's issue order (gpu/delivery_schedule.h):
  // dicts of reducer, src_off, len, pack_index, last_of_reducer. ValueError for an unknown order.
  m.def("delivery_schedule", [](const std::vector<int64_t>& group_recs, int64_t piece_bytes, const std::string& order,
                                int64_t record_bytes) {
    if (order != "wave" && order != "reducer") throw py::value_error("delivery_order must be wave or reducer");
    py::list out;
    for (const gpu::DeliveryPiece& p : gpu::delivery_schedule(group_recs, piece_bytes, order, record_bytes)) {
      py::dict d;
      d["reducer"] = p.reducer;
      d["src_off"] = p.src_off;
      d["len"] = p.len;
      d["pack_index"] = p.pack_index;
      d["last_of_reducer"] = p.last_of_reducer;
      out.append(d);
    }
    return out;
  }, py::arg("group_recs"), py::arg("piece_bytes"), py::arg("order") = "wave", py::arg("record_bytes") = 104);
  // colpack (codec/colpack.h): the host reference encoder and the consumers' decoder
  m.def("colpack_header_bytes", [] { return (int64_t)kColpackHeaderBytes; });
  m.def("colpack_have_bmi2", &colpack_have_bmi2);
  m.def("colpack_encode", [](py::bytes b, int L, int64_t buf_records) {
    std::string s = b;
    if (L < 1 || L > kColpackMaxRecordBytes || s.empty() || s.size() % (size_t)L)
      throw py::value_error("colpack_encode: need whole records of 1..256 bytes");
    const int64_t nrec = (int64_t)s.size() / L;
    std::string out((size_t)colpack_bound(L, nrec), '\0');
    const int64_t n = colpack_encode((const uint8_t*)s.data(), nrec, L, buf_records, (uint8_t*)&out[0]);
    out.resize((size_t)n);
    return py::bytes(out);
  }, py::arg("records"), py::arg("record_bytes"), py::arg("buf_records") = 1);
  // version 2 of the format: key differences (key field key_off, key_len; 0: no key) and bit-contiguous rows
  m.def("colpack2_encode", [](py::bytes b, int L, int64_t buf_records, int key_off, int key_len) {
    std::string s = b;
    if (L < 1 || L > kColpackMaxRecordBytes || s.empty() || s.size() % (size_t)L)
      throw py::value_error("colpack2_encode: need whole records of 1..256 bytes");
    if (key_off < 0 || key_len < 0 || key_len > kColpackMaxKeyBytes || key_off + key_len > L)
      throw py::value_error("colpack2_encode: key field outside the record or longer than 16 bytes");
    const int64_t nrec = (int64_t)s.size() / L;
    std::string out((size_t)colpack2_bound(L, nrec, buf_records), '\0');
    const int64_t n = colpack2_encode((const uint8_t*)s.data(), nrec, L, buf_records, key_off, key_len, (uint8_t*)&out[0]);
    out.resize((size_t)n);
    return py::bytes(out);
  }, py::arg("records"), py::arg("record_bytes"), py::arg("buf_records"), py::arg("key_off"), py::arg("key_len"));
  // path: "auto", "bmi2" or "scalar"; rows [row0, row0 + rows) (rows < 0: to the end). Raises ValueError for a
  // piece whose header fails its checks, or that is marked raw.
  m.def("colpack_decode", [](py::bytes b, int expect_L, int64_t expect_records, const std::string& path, int64_t row0,
                             int64_t rows) {
    std::string s = b;
    ColpackPiece p;
    const char* why = "";
    if (!colpack_open((const uint8_t*)s.data(), (int64_t)s.size(), expect_L, expect_records, &p, &why))
      throw py::value_error(std::string("colpack: ") + why);
    if (!p.packed) throw py::value_error("colpack: raw piece");
    if (rows < 0) rows = p.records - row0;
    if (row0 < 0 || rows < 0 || row0 + rows > p.records) throw py::value_error("colpack: rows out of range");
    std::string out((size_t)(rows * p.L), '\0');
    if (path == "bmi2") {
      if (!colpack_unpack_bmi2(p, row0, rows, (uint8_t*)&out[0])) throw std::runtime_error("no BMI2 on this CPU");
    } else if (path == "scalar") {
      colpack_unpack_scalar(p, row0, rows, (uint8_t*)&out[0]);
    } else {
      colpack_unpack(p, row0, rows, (uint8_t*)&out[0]);
    }
    return py::bytes(out);
  }, py::arg("piece"), py::arg("expect_record_bytes") = 0, py::arg("expect_records") = 0, py::arg("path") = "auto",
     py::arg("row0") = 0, py::arg("rows") = -1);
  // The three device kernels over `pieces` (each a bytes object of whole records of record_bytes): returns
  // per piece (the bytes the kernels wrote: header, rows, padding; packed flag; stride).
  auto gpu_encode = [](const std::vector<std::string>& pieces, int L, int64_t buf_records, int device, int version,
                       int key_off, int key_len) {
    if (L < 1 || L > kColpackMaxRecordBytes || pieces.empty()) throw py::value_error("gpu_colpack_encode: bad arguments");
    if (key_off < 0 || key_len < 0 || key_len > kColpackMaxKeyBytes || key_off + key_len > L)
      throw py::value_error("gpu_colpack_encode: key field outside the record or longer than 16 bytes");
    auto bound = [&](int64_t n) { return version == 2 ? colpack2_bound(L, n, buf_records) : colpack_bound(L, n); };
    std::vector<int64_t> src_off, dst_off, nrec;
    int64_t src_bytes = 0, dst_bytes = 0, max_nrec = 0;
    for (const auto& s : pieces) {
      if (s.empty() || s.size() % (size_t)L) throw py::value_error("gpu_colpack_encode: need whole records");
      src_off.push_back(src_bytes);
      dst_off.push_back(dst_bytes);
      nrec.push_back((int64_t)s.size() / L);
      max_nrec = std::max(max_nrec, nrec.back());
      src_bytes += ((int64_t)s.size() + 7) / 8 * 8;
      dst_bytes += bound(nrec.back());
    }
    const int n = (int)pieces.size();
    std::vector<gpu::ColpackResult> res((size_t)n);
    std::vector<std::string> out((size_t)n);
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      gpu::DeviceBuffer dsrc, ddst, ddesc, dtab, dres;
      dsrc.alloc((size_t)src_bytes);
      ddst.alloc((size_t)dst_bytes);
      ddesc.alloc((size_t)n * sizeof(gpu::ColpackPieceDesc));
      dtab.alloc(gpu::colpack_table_bytes(n));
      dres.alloc((size_t)n * sizeof(gpu::ColpackResult));
      std::vector<gpu::ColpackPieceDesc> descs;
      for (int i = 0; i < n; ++i) {
        HIP_CHECK(hipMemcpy(dsrc.as<uint8_t>() + src_off[i], pieces[i].data(), pieces[i].size(), hipMemcpyHostToDevice));
        descs.push_back(gpu::ColpackPieceDesc{dsrc.as<uint8_t>() + src_off[i], ddst.as<uint8_t>() + dst_off[i], nrec[i]});
      }
      HIP_CHECK(hipMemset(ddst.as(), 0xEE, (size_t)dst_bytes));  // whatever the kernels do not write shows
      HIP_CHECK(hipMemcpy(ddesc.as(), descs.data(), descs.size() * sizeof(descs[0]), hipMemcpyHostToDevice));
      hipStream_t s = nullptr;
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      gpu::launch_colpack(ddesc.as<gpu::ColpackPieceDesc>(), n, max_nrec, L, buf_records, dtab.as<uint32_t>(),
                          dres.as<gpu::ColpackResult>(), s, version, key_off, key_len);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipStreamSynchronize(s));
      HIP_CHECK(hipStreamDestroy(s));
      HIP_CHECK(hipMemcpy(res.data(), dres.as(), res.size() * sizeof(res[0]), hipMemcpyDeviceToHost));
      for (int i = 0; i < n; ++i) {
        if (res[(size_t)i].bytes < 0 || res[(size_t)i].bytes > bound(nrec[i]))
          throw std::runtime_error("gpu_colpack_encode: a piece's length is outside its region");
        out[(size_t)i].resize((size_t)res[(size_t)i].bytes);
        HIP_CHECK(hipMemcpy(&out[(size_t)i][0], ddst.as<uint8_t>() + dst_off[i], out[(size_t)i].size(), hipMemcpyDeviceToHost));
      }
    }
    py::list ret;
    for (int i = 0; i < n; ++i)
      ret.append(py::make_tuple(py::bytes(out[(size_t)i]), res[(size_t)i].packed != 0, (int64_t)res[(size_t)i].stride));
    return ret;
  };
  m.def("gpu_colpack_encode", [gpu_encode](const std::vector<std::string>& pieces, int L, int64_t buf_records, int device) {
    return gpu_encode(pieces, L, buf_records, device, 1, 0, 0);
  }, py::arg("pieces"), py::arg("record_bytes"), py::arg("buf_records") = 1, py::arg("device") = 0);
  m.def("gpu_colpack2_encode", [gpu_encode](const std::vector<std::string>& pieces, int L, int64_t buf_records,
                                            int key_off, int key_len, int device) {
    return gpu_encode(pieces, L, buf_records, device, 2, key_off, key_len);
  }, py::arg("pieces"), py::arg("record_bytes"), py::arg("buf_records"), py::arg("key_off"), py::arg("key_len"),
     py::arg("device") = 0);
  // FIXED10 delivery (gpu/fixed_delivery.h, gpu/device_reduce.h)
  // The buffers the host side of the delivery hands the sink for one landed piece. No GPU. deliver=False:
  // an empty sink; returns the counters (buffers, eof_sent, unpack_ms) instead.
  m.def("fixed_delivery_piece", [](py::bytes piece, int64_t record_bytes, int64_t buf_bytes, int64_t kv_buf, bool packed,
                                   bool last, bool deliver) -> py::object {
    std::string s = piece;
    if (kv_buf < 1 || buf_bytes < 1) throw py::value_error("fixed_delivery_piece: bad buffer sizes");
    const size_t one = (size_t)std::max(kv_buf, buf_bytes) + 16;
    std::vector<uint8_t> stg(2 * one), tail(one);
    gpu::FixedBuffers bufs;
    bufs.staging[0] = stg.data();
    bufs.staging[1] = stg.data() + one;
    bufs.tail = tail.data();
    gpu::FixedPiece p;
    p.base = (const uint8_t*)s.data();
    p.copied = (int64_t)s.size();
    p.record_bytes = record_bytes;
    p.packed = packed;
    p.last = last;
    std::vector<std::string> out;
    gpu::FixedDeliveryCounters c;
    gpu::FixedSink sink;
    if (deliver)
      sink = [&](const uint8_t* b, int64_t len) {
        out.emplace_back((const char*)b, (size_t)len);
        return 0;
      };
    gpu::deliver_fixed_piece(p, buf_bytes, kv_buf, bufs, sink, &c);
    if (!deliver) {
      py::dict d;
      d["buffers"] = c.buffers;
      d["eof_sent"] = c.eof_sent;
      d["unpack_ms"] = c.unpack_ms;
      return d;
    }
    py::list ret;
    for (const auto& b : out) ret.append(py::bytes(b));
    return ret;
  }, py::arg("piece"), py::arg("record_bytes"), py::arg("buf_bytes"), py::arg("kv_buf"), py::arg("packed"), py::arg("last"),
     py::arg("deliver") = true);
  m.def("delivery_pack_version", &gpu::delivery_pack_version);
  // FixedLayout::packed_copy_len of the layout fixed_delivery_layout describes
  m.def("fixed_delivery_packed_copy_len", [](int64_t kv_buf, int64_t piece_bytes, int pinned_slots, int pack_version,
                                             int64_t packed_bytes, int64_t nrec) {
    return gpu::fixed_layout(kv_buf, piece_bytes, pinned_slots, pack_version).packed_copy_len(packed_bytes, nrec);
  });
  m.def("fixed_delivery_layout", [](int64_t kv_buf, int64_t piece_bytes, int pinned_slots, int pack_version) {
    const gpu::FixedLayout l = gpu::fixed_layout(kv_buf, piece_bytes, pinned_slots, pack_version);
    py::dict d;
    d["buf_records"] = l.buf_records;
    d["piece"] = l.piece;
    d["slots"] = l.slots;
    d["slot_bytes"] = l.slot_bytes;
    d["region_bytes"] = l.region_bytes;
    d["staging_bytes"] = l.staging_bytes;
    d["ring_bytes"] = (int64_t)l.ring_bytes;
    d["bound_full"] = pack_version ? l.piece_bound(l.piece_recs) : 0;
    return d;
  });
  // Upload `runs` (sorted FIXED10 records), run device_reduce_fixed over them and return the delivered
  // buffers with the run's statistics. pack: mapred.uda.gpu.delivery.pack's values.
  m.def("gpu_device_reduce_fixed", [](const std::vector<std::string>& runs, int64_t kv_buf, int64_t round_bytes,
                                      int64_t piece_bytes, const std::string& pack, int device) {
    gpu::DeviceReduceConfig cfg;
    cfg.device = device;
    cfg.kv_buf_bytes = kv_buf;
    cfg.round_bytes = round_bytes;
    cfg.piece_bytes = piece_bytes;
    cfg.sample_every = 16;
    cfg.pack_version = gpu::delivery_pack_version(pack);
    if (cfg.pack_version < 0) throw py::value_error("gpu_device_reduce_fixed: pack is auto, v1 or off");
    if (kv_buf < 1 || round_bytes < 1 || piece_bytes < 1) throw py::value_error("gpu_device_reduce_fixed: bad sizes");
    for (const auto& r : runs)
      if (r.size() % (size_t)gpu::kTeraRecordBytes) throw py::value_error("gpu_device_reduce_fixed: need whole records");
    std::vector<std::string> out;
    gpu::DeviceReduceStats st;
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      std::vector<gpu::DeviceBuffer> dev(runs.size());
      std::vector<gpu::RunDesc> rd(runs.size());
      for (size_t i = 0; i < runs.size(); ++i) {
        dev[i].alloc(std::max<size_t>(runs[i].size(), 16));
        if (!runs[i].empty()) HIP_CHECK(hipMemcpy(dev[i].as(), runs[i].data(), runs[i].size(), hipMemcpyHostToDevice));
        rd[i].base = dev[i].as<uint8_t>();
        rd[i].nbytes = (int64_t)runs[i].size();
        rd[i].nrec = rd[i].nbytes / gpu::kTeraRecordBytes;
        rd[i].offsets = nullptr;
      }
      st = gpu::device_reduce_fixed(cfg, rd, [&](const uint8_t* b, int64_t len) {
        out.emplace_back((const char*)b, (size_t)len);
        return 0;
      });
    }
    py::list bufs;
    for (const auto& b : out) bufs.append(py::bytes(b));
    py::dict d;
    d["records"] = st.records;
    d["bytes"] = st.bytes;
    d["buffers"] = st.buffers;
    d["rounds"] = st.rounds;
    d["round_bytes"] = st.round_bytes;
    d["hbm_reserved"] = st.hbm_reserved;
    d["d2h_bytes"] = st.d2h_bytes;
    d["pieces"] = st.pieces;
    d["packed_pieces"] = st.packed_pieces;
    d["raw_pieces"] = st.raw_pieces;
    d["delta_pieces"] = st.delta_pieces;
    d["unpack_ms"] = st.unpack_ms;
    d["pack_wait_ms"] = st.pack_wait_ms;
    d["d2h_wait_ms"] = st.d2h_wait_ms;
    d["sink_ms"] = st.sink_ms;
    return py::make_tuple(bufs, d);
  }, py::arg("runs"), py::arg("kv_buf"), py::arg("round_bytes"), py::arg("piece_bytes") = 64ll << 20,
     py::arg("pack") = "auto", py::arg("device") = 0);
  // Upload block-compressed FIXED10 partitions back to back (followed by a guard), walk their framing on
  // the device and run device_reduce_fixed_blocks over the plan. Returns (buffers, stats); stats["streamed"]
  // False: nothing was delivered (the caller of the C++ function decodes the partitions whole). trailers:
  // every stream may end in an IFile checksum.
  m.def("gpu_device_reduce_fixed_blocks", [](int codec, const std::vector<std::string>& streams, int64_t kv_buf,
                                             int64_t round_bytes, int64_t piece_bytes, const std::string& pack,
                                             int device, bool trailers) {
    gpu::DeviceReduceConfig cfg;
    cfg.device = device;
    cfg.kv_buf_bytes = kv_buf;
    cfg.round_bytes = round_bytes;
    cfg.piece_bytes = piece_bytes;
    cfg.pack_version = gpu::delivery_pack_version(pack);
    if (cfg.pack_version < 0) throw py::value_error("gpu_device_reduce_fixed_blocks: pack is auto, v1 or off");
    if (kv_buf < 1 || round_bytes < 1 || piece_bytes < 1) throw py::value_error("gpu_device_reduce_fixed_blocks: bad sizes");
    if (codec < 1 || codec > 3) throw py::value_error("gpu_device_reduce_fixed_blocks: codec is 1 (snappy), 2 (lzo) or 3 (lz4)");
    std::vector<std::string> out;
    gpu::DeviceReduceStats st;
    bool streamed = false;
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      gpu::DeviceBuffer din, scratch, desc_scratch;
      std::vector<const uint8_t*> dptrs;
      std::vector<int64_t> lens;
      upload_streams(streams, &din, &dptrs, &lens);
      gpu::BlockPlan plan;
      std::vector<int> tl;
      hipStream_t s;
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      bool ok = false;
      try {
        ok = gpu::plan_block_streams_device((Codec)codec, dptrs, lens, &plan, scratch, desc_scratch, s, trailers ? &tl : nullptr);
      } catch (...) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
        throw;
      }
      HIP_CHECK(hipStreamDestroy(s));
      if (!ok) throw UdaError("block framing not resolvable on the device");
      st = gpu::device_reduce_fixed_blocks(cfg, codec, plan, [&](const uint8_t* b, int64_t len) {
        out.emplace_back((const char*)b, (size_t)len);
        return 0;
      }, &streamed);
      check_stream_guard(din, lens);
    }
    py::list bufs;
    for (const auto& b : out) bufs.append(py::bytes(b));
    py::dict d;
    d["streamed"] = streamed;
    d["records"] = st.records;
    d["bytes"] = st.bytes;
    d["buffers"] = st.buffers;
    d["rounds"] = st.rounds;
    d["round_bytes"] = st.round_bytes;
    d["decoded_blocks"] = st.decoded_blocks;
    d["d2h_bytes"] = st.d2h_bytes;
    d["pieces"] = st.pieces;
    d["packed_pieces"] = st.packed_pieces;
    d["raw_pieces"] = st.raw_pieces;
    d["delta_pieces"] = st.delta_pieces;
    return py::make_tuple(bufs, d);
  }, py::arg("codec"), py::arg("streams"), py::arg("kv_buf"), py::arg("round_bytes"), py::arg("piece_bytes") = 64ll << 20,
     py::arg("pack") = "auto", py::arg("device") = 0, py::arg("trailers") = false);
  // Merge given sorted FIXED10 runs (whole 104-byte records, no EOF marker) with a DeviceMerger made for
  // this call, so the UDA_KWAY* environment of the moment applies. The runs share one device buffer; each
  // starts at a multiple of 16 bytes plus `pad` (8: the staged kernel's half-chunk offset; 2: the
  // alignment of Hadoop MOF partitions). Returns (merged bytes, {passes, overflow_cells, bad_layout, kway}).
  m.def("gpu_merge_fixed", [](const py::list& runs, const py::object& group_first, int device, int pad) {
    if (pad != 0 && pad != 8 && pad != 2) throw py::value_error("gpu_merge_fixed: pad is 0, 8 or 2");
    const int K = (int)runs.size();
    std::vector<std::string> host((size_t)K);
    std::vector<size_t> at((size_t)K);
    size_t in_bytes = 0;
    int64_t total = 0;
    for (int i = 0; i < K; ++i) {
      py::buffer_info v = py::cast<py::buffer>(runs[i]).request();
      host[i].assign((const char*)v.ptr, (size_t)(v.size * v.itemsize));
      if (host[i].size() % (size_t)gpu::kTeraRecordBytes) throw py::value_error("gpu_merge_fixed: need whole records");
      at[i] = ((in_bytes + 15) & ~(size_t)15) + (size_t)pad;
      in_bytes = at[i] + host[i].size();
      total += (int64_t)(host[i].size() / (size_t)gpu::kTeraRecordBytes);
    }
    std::vector<int> gf = group_first.is_none() ? std::vector<int>{0, K} : group_first.cast<std::vector<int>>();
    for (size_t g = 0; g + 1 < gf.size(); ++g)
      if (gf[g] > gf[g + 1]) throw py::value_error("gpu_merge_fixed: group_first must not decrease");
    const int64_t out_bytes = total * gpu::kTeraRecordBytes;
    PyObject* o = PyBytes_FromStringAndSize(nullptr, (Py_ssize_t)out_bytes);
    if (!o) throw py::error_already_set();
    py::bytes out = py::reinterpret_steal<py::bytes>(o);
    int passes = 0, overflow = 0;
    bool bad = false, kway = false;
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      gpu::DeviceBuffer in, merged;
      in.alloc(std::max<size_t>(in_bytes, 16));
      merged.alloc((size_t)std::max<int64_t>(out_bytes, 16));
      std::vector<gpu::RunDesc> rd((size_t)K);
      for (int i = 0; i < K; ++i) {
        if (!host[i].empty())
          HIP_CHECK(hipMemcpy(in.as<uint8_t>() + at[i], host[i].data(), host[i].size(), hipMemcpyHostToDevice));
        rd[i].base = in.as<uint8_t>() + at[i];
        rd[i].nbytes = (int64_t)host[i].size();
        rd[i].nrec = rd[i].nbytes / gpu::kTeraRecordBytes;
        rd[i].offsets = nullptr;
      }
      hipStream_t s = nullptr;
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      try {
        gpu::DeviceMerger merger(std::max<int64_t>(total, 1), std::max(K, 1));
        merger.merge_fixed(rd, gf, merged.as<uint8_t>(), s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
        if (out_bytes)
          HIP_CHECK(hipMemcpy(PyBytes_AS_STRING(o), merged.as(), (size_t)out_bytes, hipMemcpyDeviceToHost));
        passes = merger.last_passes();
        overflow = merger.kway_overflow_cells();
        bad = merger.bad_layout();
        kway = merger.kway_enabled();
      } catch (...) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
        throw;
      }
      (void)hipStreamDestroy(s);
    }
    py::dict d;
    d["passes"] = passes;
    d["overflow_cells"] = overflow;
    d["bad_layout"] = bad;
    d["kway"] = kway;
    return py::make_tuple(out, d);
  }, py::arg("runs"), py::arg("group_first") = py::none(), py::arg("device") = 0, py::arg("pad") = 0);
  m.def("codec_from_class", [](const std::string& c) {
    bool unsup = false;
    int v = (int)codec_from_class(c, &unsup);
    return unsup ? -1 : v;
  });
  // The codec of a job's map outputs, as INIT resolves it: codec_from_class's answers plus GzipCodec -> 5
  // (codec_from_class itself keeps refusing Gzip: see uda/codec.h). -1 = unsupported.
  m.def("map_output_codec", [](const std::string& c) {
    bool unsup = false;
    int v = (int)map_output_codec(c, &unsup);
    return unsup ? -1 : v;
  });
  // What INIT calls: map_output_codec's answers plus ZStandardCodec -> 6. -1 = unsupported.
  m.def("job_codec", [](const std::string& c) {
    bool unsup = false;
    int v = (int)job_codec(c, &unsup);
    return unsup ? -1 : v;
  });
  // zstd (ZStandardCodec): the in-tree encoder (one frame, Raw literals, Predefined-mode sequences) and the
  // one-shot host decode of one or more frames: (raw bytes, bytes of the input the frames took). ValueError
  // with the decoder's reason for anything it refuses or more than cap bytes of output.
  m.def("zstd_compress", [](py::bytes b) {
    std::string s = b;
    std::string out(zstd_max_compressed_length(s.size()), '\0');
    out.resize(zstd_compress((const uint8_t*)s.data(), s.size(), (uint8_t*)&out[0]));
    return py::bytes(out);
  });
  m.def("zstd_decompress", [](py::bytes b, size_t cap) {
    std::string s = b;
    std::string out(cap, '\0'), why;
    size_t n = 0, used = 0;
    if (!zstd_decompress((const uint8_t*)s.data(), s.size(), (uint8_t*)&out[0], cap, &n, &used, nullptr, &why))
      throw py::value_error(why);
    out.resize(n);
    return py::make_tuple(py::bytes(out), used);
  }, py::arg("data"), py::arg("cap"));
  // What a decode of `stream` meets: block types, literal types (1 and 4 streams), weight encodings, each
  // sequence mode per table. Coverage counters for the tests. ValueError if the stream does not decode into cap bytes.
  m.def("zstd_decoder_stats", [](py::bytes b, size_t cap) {
    std::string s = b;
    std::string out(cap, '\0'), why;
    size_t n = 0, used = 0;
    ZstdStats st;
    if (!zstd_decompress((const uint8_t*)s.data(), s.size(), (uint8_t*)&out[0], cap, &n, &used, &st, &why))
      throw py::value_error(why);
    py::dict d;
    d["frames"] = st.frames;
    d["skippable"] = st.skippable;
    d["max_frame_blocks"] = st.max_frame_blocks;
    d["blocks"] = py::dict(py::arg("raw") = st.blocks[0], py::arg("rle") = st.blocks[1], py::arg("compressed") = st.blocks[2]);
    d["literals"] = py::dict(py::arg("raw") = st.literals[0], py::arg("rle") = st.literals[1],
                             py::arg("compressed") = st.literals[2], py::arg("treeless") = st.literals[3],
                             py::arg("streams1") = st.huf_streams[0], py::arg("streams4") = st.huf_streams[1]);
    d["weights"] = py::dict(py::arg("direct") = st.weights[0], py::arg("fse") = st.weights[1]);
    const char* tables[3] = {"ll", "of", "ml"};
    py::dict modes;
    for (int t = 0; t < 3; ++t)
      modes[tables[t]] = py::dict(py::arg("predefined") = st.modes[t][0], py::arg("rle") = st.modes[t][1],
                                  py::arg("fse") = st.modes[t][2], py::arg("repeat") = st.modes[t][3]);
    d["modes"] = modes;
    d["sequences"] = st.sequences;
    d["max_offset"] = st.max_offset;
    d["checksums"] = st.checksums;
    return d;
  }, py::arg("stream"), py::arg("cap") = (size_t)4 << 20);
  // The incremental decoder fed in pieces of `piece` bytes, read dry after every feed: (raw, consumed, finished,
  // the most bytes its history / output buffer held, the most its input buffer held). UdaError text as ValueError.
  m.def("zstd_stream_decode", [](py::bytes b, size_t piece) {
    std::string s = b;
    if (piece == 0) throw py::value_error("piece == 0");
    ZstdDecoder d;
    std::string out;
    std::vector<uint8_t> tmp(1 << 16);
    size_t most = 0, most_in = 0;
    try {
      for (size_t off = 0; off < s.size(); off += piece) {
        d.feed((const uint8_t*)s.data() + off, std::min(piece, s.size() - off));
        for (size_t k; (k = d.read(tmp.data(), tmp.size())) > 0;) out.append((const char*)tmp.data(), k);
        most = std::max(most, d.history_bytes());
        most_in = std::max(most_in, d.input_bytes());
      }
    } catch (const UdaError& e) {
      throw py::value_error(e.what());
    }
    return py::make_tuple(py::bytes(out), d.consumed(), d.finished(), most, most_in);
  }, py::arg("stream"), py::arg("piece"));
  m.def("block_compress", [](int codec, py::bytes b, size_t block) {
    std::string s = b;
    auto v = block_compress((Codec)codec, (const uint8_t*)s.data(), s.size(), block);
    return py::bytes((const char*)v.data(), v.size());
  });
  m.def("block_decompress", [](int codec, py::bytes b, size_t feed_chunk) {
    std::string s = b;
    BlockDecoder d((Codec)codec);
    std::string out;
    std::vector<uint8_t> tmp(1 << 16);
    for (size_t off = 0; off < s.size(); off += feed_chunk) {
      d.feed((const uint8_t*)s.data() + off, std::min(feed_chunk, s.size() - off));
      for (;;) {
        size_t n = d.read(tmp.data(), tmp.size());
        if (!n) break;
        out.append((const char*)tmp.data(), n);
      }
    }
    if (!d.idle()) throw py::value_error("truncated block stream");
    return py::bytes(out);
  });

  // zlib (DefaultCodec) one-shot host decode: (raw bytes, bytes of the input the stream took). ValueError for
  // anything zlib's inflate refuses, a truncated stream, an Adler-32 mismatch or more than cap bytes of output.
  m.def("zlib_decompress", [](py::bytes b, size_t cap) {
    std::string s = b;
    std::string out(cap, '\0');
    size_t n = 0, used = 0;
    if (!zlib_decompress((const uint8_t*)s.data(), s.size(), (uint8_t*)&out[0], cap, &n, &used))
      throw py::value_error("corrupt zlib data");
    out.resize(n);
    return py::make_tuple(py::bytes(out), used);
  }, py::arg("data"), py::arg("cap"));
  // gzip (GzipCodec) one-shot host decode of one or more concatenated members: (raw bytes, bytes of the input
  // the members took). ValueError for anything zlib's inflate with wbits = 31 refuses, anything truncated, a
  // CRC-32 or ISIZE mismatch or more than cap bytes of output.
  m.def("gzip_decompress", [](py::bytes b, size_t cap) {
    std::string s = b;
    std::string out(cap, '\0');
    size_t n = 0, used = 0;
    if (!gzip_decompress((const uint8_t*)s.data(), s.size(), (uint8_t*)&out[0], cap, &n, &used))
      throw py::value_error("corrupt gzip data");
    out.resize(n);
    return py::make_tuple(py::bytes(out), used);
  }, py::arg("data"), py::arg("cap"));
  // A whole compressed partition as the GPU paths decode it on the host (consumer/gpu_workspace.h): all but
  // the last four bytes first, and the decoder says whether those four are an IFile checksum. (raw, tail)
  m.def("host_decode_partition", [](int codec, py::bytes b) {
    std::string s = b;
    int tail = 0;
    std::vector<uint8_t> raw = host_decode_partition((Codec)codec, (const uint8_t*)s.data(), (int64_t)s.size(), &tail);
    return py::make_tuple(py::bytes((const char*)raw.data(), raw.size()), tail);
  }, py::arg("codec"), py::arg("partition"));

  // ---- IFile checksum trailer (uda/ifile.h)
  m.def("crc32", [](py::bytes b, uint32_t seed) {
    std::string s = b;
    return crc32_ieee((const uint8_t*)s.data(), s.size(), seed);
  }, py::arg("data"), py::arg("seed") = 0);
  m.def("crc32_combine", [](uint32_t a, uint32_t b, int64_t len_b) { return crc32_combine(a, b, len_b); },
        py::arg("crc_a"), py::arg("crc_b"), py::arg("len_b"));
  m.def("crc32_fold_state", [](uint32_t state, uint32_t seg_state, int64_t seg_len) {
    return crc32_fold_state(state, seg_state, seg_len);
  }, py::arg("state"), py::arg("seg_state"), py::arg("seg_len"));
  m.def("ifile_trailer_bytes", &ifile_trailer_bytes, py::arg("raw_len"), py::arg("part_len"));
  // the trailer-aware host framing walk of one block-compressed stream: (blocks, tail bytes)
  m.def("plan_block_streams", [](int codec, py::bytes b) {
    std::string s = b;
    gpu::BlockPlan plan;
    std::vector<int> tails;
    if (!gpu::plan_block_streams((Codec)codec, {(const uint8_t*)s.data()}, {(int64_t)s.size()}, &plan, &tails))
      throw py::value_error("block framing malformed or not resolvable without decoding");
    return py::make_tuple((int64_t)plan.descs.size(), tails[0]);
  }, py::arg("codec"), py::arg("stream"));
  // the host walk of several streams in full: ([(stream, src, src_end, dst, raw) per block], raw_offset,
  // tails), src and src_end as offsets into the block's stream; None when the framing is not resolvable
  m.def("plan_block_streams_descs", [](int codec, const std::vector<std::string>& streams, bool tails) -> py::object {
    std::vector<const uint8_t*> ptrs;
    std::vector<int64_t> lens;
    for (const auto& st : streams) {
      ptrs.push_back((const uint8_t*)st.data());
      lens.push_back((int64_t)st.size());
    }
    gpu::BlockPlan plan;
    std::vector<int> tl;
    if (!gpu::plan_block_streams((Codec)codec, ptrs, lens, &plan, tails ? &tl : nullptr)) return py::none();
    return block_plan_tuple(plan, lens, 0, tl, tails);
  }, py::arg("codec"), py::arg("streams"), py::arg("tails") = false);
  // the device walk (plan_block_streams_device) of the same streams, uploaded back to back without
  // alignment and followed by a guard; the same tuple, or None
  m.def("gpu_plan_block_streams_device", [](int codec, const std::vector<std::string>& streams, bool tails,
                                            int device) -> py::object {
    gpu::BlockPlan plan;
    std::vector<int> tl;
    std::vector<int64_t> lens;
    bool ok = false;
    int64_t base = 0;
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      gpu::DeviceBuffer din, scratch, desc_scratch;
      std::vector<const uint8_t*> dptrs;
      upload_streams(streams, &din, &dptrs, &lens);
      base = (int64_t)(uintptr_t)din.as<uint8_t>();
      hipStream_t s;
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      try {
        ok = gpu::plan_block_streams_device((Codec)codec, dptrs, lens, &plan, scratch, desc_scratch, s, tails ? &tl : nullptr);
      } catch (...) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
        throw;
      }
      HIP_CHECK(hipStreamDestroy(s));
      check_stream_guard(din, lens);
    }
    if (!ok) return py::none();
    return block_plan_tuple(plan, lens, base, tl, tails);
  }, py::arg("codec"), py::arg("streams"), py::arg("tails") = false, py::arg("device") = 0);
  // The round plan of the streaming block decode (block_rounds.h), no device needed. nrec: records per
  // stream; blocks: per stream the raw sizes of its non-empty blocks; first_keys: per block (all streams, in
  // order) the 10 key bytes of the first record that starts in it, or None where there is none (only the
  // entries of blocks whose `first` is >= 0 are read). Returns {first, sorted, Q, bounds, spans, in_bytes,
  // in_recs}; spans[q][k] = {b0, b1, rec0, rec1, in_off}, blocks numbered over all streams. sorted False
  // (the keys of a stream descend): no rounds are planned.
  m.def("block_round_plan", [](const std::vector<int64_t>& nrec, const std::vector<std::vector<int64_t>>& blocks,
                               const std::vector<py::object>& first_keys, int64_t round_bytes) {
    if (nrec.size() != blocks.size()) throw py::value_error("block_round_plan: one block list per stream");
    if (round_bytes < 1) throw py::value_error("block_round_plan: round_bytes < 1");
    gpu::BlockGeometry g;
    g.nrec = nrec;
    g.blk0.push_back(0);
    for (size_t k = 0; k < blocks.size(); ++k) {
      int64_t rel = 0;
      for (int64_t raw : blocks[k]) {
        if (raw < 1) throw py::value_error("block_round_plan: a block holds at least one byte");
        g.rel.push_back(rel);
        g.raw.push_back(raw);
        rel += raw;
      }
      if (nrec[k] < 0 || rel != nrec[k] * gpu::kBlockRecordBytes + 2)
        throw py::value_error("block_round_plan: a stream's blocks hold its records and the EOF marker");
      g.blk0.push_back((int64_t)g.rel.size());
    }
    if (first_keys.size() != g.rel.size()) throw py::value_error("block_round_plan: one first key (or None) per block");
    const std::vector<int32_t> first = gpu::block_first_offsets(g);
    std::vector<gpu::BlockKey> keys(first.size(), gpu::BlockKey{~0ull, ~0ull});
    for (size_t b = 0; b < first.size(); ++b)
      if (first[b] >= 0) {
        if (first_keys[b].is_none()) throw py::value_error("block_round_plan: a block that starts a record needs its key");
        keys[b] = block_key_of(first_keys[b].cast<std::string>());
      }
    py::dict d;
    py::list fl;
    for (int32_t f : first) fl.append((int)f);
    d["first"] = fl;
    gpu::BlockIndex index;
    const bool sorted = gpu::build_block_index(g, first, keys, &index);
    d["sorted"] = sorted;
    if (!sorted) return d;
    gpu::RoundPlan rp;
    gpu::plan_rounds(g, index, round_bytes, &rp);
    d["Q"] = rp.Q;
    py::list bounds, spans, ib, ir;
    for (const auto& b : rp.bounds) bounds.append(block_key_bytes(b));
    for (int q = 0; q < rp.Q; ++q) {
      py::list row;
      for (const auto& sp : rp.spans[(size_t)q]) {
        py::dict e;
        e["b0"] = sp.b0;
        e["b1"] = sp.b1;
        e["rec0"] = sp.rec0;
        e["rec1"] = sp.rec1;
        e["in_off"] = sp.in_off;
        row.append(e);
      }
      spans.append(row);
      ib.append(rp.in_bytes[(size_t)q]);
      ir.append(rp.in_recs[(size_t)q]);
    }
    d["bounds"] = bounds;
    d["spans"] = spans;
    d["in_bytes"] = ib;
    d["in_recs"] = ir;
    return d;
  }, py::arg("nrec"), py::arg("blocks"), py::arg("first_keys"), py::arg("round_bytes"));
  m.def("gpu_crc32_chunk_bytes", [] { return gpu::crc32_chunk_bytes(); });
  // zlib.crc32 of every input by one launch of the device kernels (crc32.hip): the inputs lie in one device
  // buffer, each at an address that is `misalign` modulo 16
  // (states: launch_crc32_states, the raw register after every input from a zero register)
  auto gpu_crc32 = [](const std::vector<std::string>& inputs, int misalign, int device, bool states) {
    if (misalign < 0 || misalign > 15) throw py::value_error("misalign must be 0..15");
    const int n = (int)inputs.size();
    std::vector<uint32_t> out((size_t)n, 0);
    if (n == 0) return out;
    py::gil_scoped_release rel;
    HIP_CHECK(hipSetDevice(device));
    std::vector<int64_t> at((size_t)n);
    int64_t total = 16;
    for (int i = 0; i < n; ++i) {
      at[(size_t)i] = total + misalign;
      total = (total + misalign + (int64_t)inputs[(size_t)i].size() + 15) & ~(int64_t)15;
    }
    gpu::DeviceBuffer data((size_t)total + 16);
    uint8_t* base = data.as<uint8_t>();
    if ((uintptr_t)base & 15) throw UdaError("device allocation is not 16-byte aligned");
    hipStream_t s;
    HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    std::vector<gpu::CrcDesc> descs((size_t)n);
    std::vector<int64_t> first((size_t)n + 1);
    for (int i = 0; i < n; ++i) {
      const std::string& in = inputs[(size_t)i];
      descs[(size_t)i] = gpu::CrcDesc{base + at[(size_t)i], (int64_t)in.size()};
      if (!in.empty()) HIP_CHECK(hipMemcpyAsync(base + at[(size_t)i], in.data(), in.size(), hipMemcpyHostToDevice, s));
    }
    const int64_t chunks = gpu::crc32_chunk_plan(descs.data(), n, first.data());
    gpu::DeviceBuffer d_descs((size_t)n * sizeof(gpu::CrcDesc)), d_first(((size_t)n + 1) * 8), d_out((size_t)n * 4),
        ws(gpu::crc32_ws_bytes(chunks));
    HIP_CHECK(hipMemcpyAsync(d_descs.as(), descs.data(), (size_t)n * sizeof(gpu::CrcDesc), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_first.as(), first.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
    (states ? gpu::launch_crc32_states : gpu::launch_crc32)(d_descs.as<gpu::CrcDesc>(), n, d_first.as<int64_t>(), chunks,
                                                            ws.as(), d_out.as<uint32_t>(), s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out.data(), d_out.as(), (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipStreamDestroy(s));
    return out;
  };
  m.def("gpu_crc32", [gpu_crc32](const std::vector<std::string>& inputs, int misalign, int device) {
    return gpu_crc32(inputs, misalign, device, false);
  }, py::arg("inputs"), py::arg("misalign") = 0, py::arg("device") = 0);
  // zlib.crc32(input, 0xFFFFFFFF) ^ 0xFFFFFFFF of every input: what crc32_fold_state chains
  m.def("gpu_crc32_states", [gpu_crc32](const std::vector<std::string>& inputs, int misalign, int device) {
    return gpu_crc32(inputs, misalign, device, true);
  }, py::arg("inputs"), py::arg("misalign") = 0, py::arg("device") = 0);
  // benchmarks/run_configs.py checksum: `parts` ranges of `part_bytes` random bytes; per repetition the
  // milliseconds (hipEvents) of the CRC launch and of launch_batched_copy of the same bytes
  m.def("gpu_crc32_bench", [](int parts, int64_t part_bytes, int warmup, int reps, int device) {
    std::vector<double> crc_ms, copy_ms;
    bool ok = true;
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      const int64_t stride = (part_bytes + 255) & ~(int64_t)255;
      gpu::DeviceBuffer src((size_t)(stride * parts) + 16), dst((size_t)(stride * parts) + 16);
      hipStream_t s;
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      {  // random bytes (a pattern repeated: the kernel's speed does not depend on the values)
        std::vector<uint8_t> pat(64 << 20);
        std::mt19937_64 rng(7);
        for (size_t i = 0; i + 8 <= pat.size(); i += 8) {
          const uint64_t v = rng();
          std::memcpy(&pat[i], &v, 8);
        }
        for (int64_t o = 0; o < stride * parts; o += (int64_t)pat.size())
          HIP_CHECK(hipMemcpyAsync(src.as<uint8_t>() + o, pat.data(), (size_t)std::min<int64_t>((int64_t)pat.size(), stride * parts - o),
                                   hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));
      }
      std::vector<gpu::CrcDesc> descs((size_t)parts);
      std::vector<gpu::CopyDesc> copies((size_t)parts);
      std::vector<int64_t> first((size_t)parts + 1);
      for (int i = 0; i < parts; ++i) {
        descs[(size_t)i] = gpu::CrcDesc{src.as<uint8_t>() + stride * i, part_bytes};
        copies[(size_t)i] = gpu::CopyDesc{src.as<uint8_t>() + stride * i, dst.as<uint8_t>() + stride * i, part_bytes};
      }
      const int64_t chunks = gpu::crc32_chunk_plan(descs.data(), parts, first.data());
      gpu::DeviceBuffer d_descs((size_t)parts * sizeof(gpu::CrcDesc)), d_first(((size_t)parts + 1) * 8),
          d_out((size_t)parts * 4), ws(gpu::crc32_ws_bytes(chunks)), d_copies((size_t)parts * sizeof(gpu::CopyDesc));
      HIP_CHECK(hipMemcpyAsync(d_descs.as(), descs.data(), (size_t)parts * sizeof(gpu::CrcDesc), hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(d_first.as(), first.data(), ((size_t)parts + 1) * 8, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(d_copies.as(), copies.data(), (size_t)parts * sizeof(gpu::CopyDesc), hipMemcpyHostToDevice, s));
      hipEvent_t e0, e1;
      HIP_CHECK(hipEventCreate(&e0));
      HIP_CHECK(hipEventCreate(&e1));
      std::vector<uint32_t> got((size_t)parts), ref;
      for (int which = 0; which < 2; ++which)
        for (int r = 0; r < warmup + reps; ++r) {
          HIP_CHECK(hipEventRecord(e0, s));
          if (which == 0)
            gpu::launch_crc32(d_descs.as<gpu::CrcDesc>(), parts, d_first.as<int64_t>(), chunks, ws.as(), d_out.as<uint32_t>(), s);
          else
            gpu::launch_batched_copy(d_copies.as<gpu::CopyDesc>(), parts, part_bytes, s);
          HIP_CHECK(hipEventRecord(e1, s));
          HIP_CHECK(hipEventSynchronize(e1));
          float ms = 0;
          HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
          if (r >= warmup) (which == 0 ? crc_ms : copy_ms).push_back((double)ms);
          if (which == 0) {  // every repetition gives the same values
            HIP_CHECK(hipMemcpy(got.data(), d_out.as(), (size_t)parts * 4, hipMemcpyDeviceToHost));
            if (ref.empty()) ref = got;
            ok = ok && got == ref;
          }
        }
      (void)hipEventDestroy(e0);
      (void)hipEventDestroy(e1);
      HIP_CHECK(hipStreamDestroy(s));
    }
    py::dict d;
    d["crc_ms"] = crc_ms;
    d["copy_ms"] = copy_ms;
    d["bytes"] = (int64_t)parts * part_bytes;
    d["repeatable"] = ok;
    return d;
  }, py::arg("parts"), py::arg("part_bytes"), py::arg("warmup") = 3, py::arg("reps") = 10, py::arg("device") = 0);

  m.def("generate_runs", [](const std::string& kind, int maps, int reducers, int64_t rows, uint64_t seed) {
    std::vector<std::vector<std::vector<uint8_t>>> r;
    {
      py::gil_scoped_release g;
      r = generate_runs(kind, maps, reducers, rows, seed);
    }
    py::list out;
    for (auto& m : r) {
      py::list parts;
      for (auto& p : m) parts.append(py::bytes((const char*)p.data(), p.size()));
      out.append(parts);
    }
    return out;
  });

  // ---------------------------------------------------------------- CPU engine
  m.def("cpu_merge", [](const std::vector<std::string>& runs, const std::string& key_class, int64_t buf,
                        const std::string& combine, const std::string& key_order) {
    std::vector<int64_t> lens;
    py::bytes out = cpu_merge_impl(runs, key_class, buf, &lens, combine_op_arg(combine), key_order);
    return py::make_tuple(out, lens);
  }, py::arg("runs"), py::arg("key_class"), py::arg("buf"), py::arg("combine") = "none",
        py::arg("key_order") = "reference");
  // Host reference of the reduce-side combiner (uda/combine.h) over a stream already in merged order.
  m.def("combine_stream", [](const std::string& stream, const std::string& key_class, const std::string& op,
                             const std::string& key_order) {
    KeyKind kind = key_kind_arg(key_class, key_order);
    const std::vector<uint8_t> out =
        combine_stream(reinterpret_cast<const uint8_t*>(stream.data()), stream.size(), kind, combine_op_arg(op));
    return py::bytes(reinterpret_cast<const char*>(out.data()), out.size());
  }, py::arg("stream"), py::arg("key_class"), py::arg("op"), py::arg("key_order") = "reference");
  // merged elements per workgroup of the device combiner's segmented sum (tests build groups around it)
  m.def("combine_tile", [] { return (int)gpu::kCombineTile; });

  // teravalidate: framing + order + checksum of a delivered stream, fed buffer by buffer
  py::class_<StreamValidator, std::shared_ptr<StreamValidator>>(m, "StreamValidator")
      .def(py::init([](const std::string& key_class, const std::string& key_order) {
        return std::make_shared<StreamValidator>(key_kind_arg(key_class, key_order));
      }), py::arg("key_class"), py::arg("key_order") = "reference")
      .def("feed", [](StreamValidator& v, py::buffer b) {
        py::buffer_info bi = b.request();
        v.feed(static_cast<const uint8_t*>(bi.ptr), (size_t)(bi.size * bi.itemsize));
      })
      .def_readonly("records", &StreamValidator::records)
      .def_readonly("bytes", &StreamValidator::bytes)
      .def_readonly("buffers", &StreamValidator::buffers)
      .def_readonly("order_errors", &StreamValidator::order_errors)
      .def_readonly("framing_errors", &StreamValidator::framing_errors)
      .def_readonly("checksum", &StreamValidator::checksum)
      .def_readonly("eof", &StreamValidator::eof);
  // True iff the whole-record buffer's last record is the EOF marker (-1, -1): walks the VInt framing
  // from the buffer's start (a dataFromUda buffer begins on a record boundary), so record bytes that
  // happen to end in 0xFF 0xFF are not taken for the marker. -1 on broken framing.
  m.def("buffer_ends_with_eof", [](py::buffer b) {
    py::buffer_info bi = b.request();
    const uint8_t* p = static_cast<const uint8_t*>(bi.ptr);
    const int64_t n = (int64_t)(bi.size * bi.itemsize);
    int64_t off = 0;
    while (off < n) {
      int64_t kl = 0, vl = 0;
      const int a = vint_decode(p + off, (size_t)(n - off), &kl);
      if (a <= 0) return -1;
      const int c = vint_decode(p + off + a, (size_t)(n - off - a), &vl);
      if (c <= 0) return -1;
      if (kl == -1 && vl == -1) return off + a + c == n ? 1 : -1;
      if (kl < 0 || vl < 0 || off + a + c + kl + vl > n) return -1;
      off += a + c + kl + vl;
    }
    return 0;
  });
  m.def("ifile_checksum", [](py::buffer b) {
    py::buffer_info bi = b.request();
    int64_t recs = 0, bytes = 0;
    uint64_t ck;
    {
      py::gil_scoped_release r;
      ck = ifile_checksum(static_cast<const uint8_t*>(bi.ptr), (size_t)(bi.size * bi.itemsize), &recs, &bytes);
    }
    return py::make_tuple(recs, bytes, ck);
  });

  // ---------------------------------------------------------------- async IO
  m.def("aio_selftest", [](const std::string& path, int64_t size, const std::string& backend) {
    // write `size` bytes in 64 KiB pieces then read them back through the same backend
    if (!backend.empty()) setenv("UDA_AIO_BACKEND", backend.c_str(), 1);
    auto io = AsyncIO::create(AsyncIO::Options());
    unsetenv("UDA_AIO_BACKEND");
    int fd = ::open(path.c_str(), O_CREAT | O_TRUNC | O_RDWR | O_CLOEXEC, 0600);
    if (fd < 0) throw std::runtime_error("open failed");
    std::vector<uint8_t> src((size_t)size), dst((size_t)size, 0);
    for (int64_t i = 0; i < size; ++i) src[(size_t)i] = (uint8_t)(i * 131 + (i >> 9));
    std::atomic<int64_t> bad{0};
    const int64_t piece = 64 << 10;
    for (int64_t off = 0; off < size; off += piece) {
      int64_t len = std::min(piece, size - off);
      io->write(fd, off, len, src.data() + off, [&bad, len](int64_t r) { if (r != len) bad++; });
    }
    io->drain();
    for (int64_t off = 0; off < size; off += piece) {
      int64_t len = std::min(piece, size - off);
      io->read(fd, off, len, dst.data() + off, [&bad, len](int64_t r) { if (r != len) bad++; });
    }
    io->drain();
    ::close(fd);
    return py::make_tuple(std::string(io->backend()), bad.load() == 0 && src == dst);
  });

  // AIO microbenchmark (AIOHandler_test parity, src/tests/AIOHandler_test.cc:244-249): read `size`
  // bytes of `path` in `block` pieces with up to `depth` in flight through AsyncIO (O_DIRECT when
  // `direct`), then with a sequential pread loop; returns MB/s of both.
  m.def("aio_bench", [](const std::string& path, int64_t size, int64_t block, int depth, bool direct,
                        const std::string& backend) {
    py::gil_scoped_release rel;
    {
      int fd = ::open(path.c_str(), O_CREAT | O_TRUNC | O_WRONLY | O_CLOEXEC, 0600);
      if (fd < 0) throw std::runtime_error("open for write failed");
      std::vector<uint8_t> buf((size_t)(8 << 20));
      for (size_t i = 0; i < buf.size(); ++i) buf[i] = (uint8_t)(i * 2654435761u >> 13);
      for (int64_t off = 0; off < size; off += (int64_t)buf.size()) {
        const size_t n = (size_t)std::min<int64_t>((int64_t)buf.size(), size - off);
        if (::pwrite(fd, buf.data(), n, off) != (ssize_t)n) throw std::runtime_error("pwrite failed");
      }
      ::fsync(fd);
      ::close(fd);
    }
    if (!backend.empty()) setenv("UDA_AIO_BACKEND", backend.c_str(), 1);
    AsyncIO::Options o;
    o.queue_depth = std::max(depth, 1);
    auto io = AsyncIO::create(o);
    unsetenv("UDA_AIO_BACKEND");
    int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC | (direct ? O_DIRECT : 0));
    if (fd < 0 && direct) fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);  // tmpfs: no O_DIRECT
    if (fd < 0) throw std::runtime_error("open for read failed");
    const int nbuf = std::max(depth, 1);
    std::vector<void*> bufs;
    for (int i = 0; i < nbuf; ++i) bufs.push_back(aligned_alloc_io((size_t)block));
    std::atomic<int64_t> bad{0}, got{0};
    auto t0 = std::chrono::steady_clock::now();
    int64_t off = 0;
    while (off < size) {
      for (int i = 0; i < nbuf && off < size; ++i, off += block)
        io->read(fd, off, std::min(block, size - off), bufs[(size_t)i], [&](int64_t r) {
          if (r < 0) bad++;
          else got += r;
        });
      io->drain();
    }
    const double aio_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    // the same reads with `depth` kept in flight throughout (a new read as each one lands), the way a
    // store loader streams a file; the batch loop above idles the device at every batch's tail
    double cont_s = 0;
    {
      std::mutex m;
      std::condition_variable cv;
      std::vector<int> free_bufs;
      for (int i = 0; i < nbuf; ++i) free_bufs.push_back(i);
      const auto c0 = std::chrono::steady_clock::now();
      for (int64_t o3 = 0; o3 < size; o3 += block) {
        int bi;
        {
          std::unique_lock<std::mutex> lk(m);
          cv.wait(lk, [&] { return !free_bufs.empty(); });
          bi = free_bufs.back();
          free_bufs.pop_back();
        }
        io->read(fd, o3, std::min(block, size - o3), bufs[(size_t)bi], [&, bi](int64_t r) {
          if (r < 0) bad++;
          std::lock_guard<std::mutex> g(m);
          free_bufs.push_back(bi);
          cv.notify_all();
        });
      }
      io->drain();
      cont_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count();
    }
    t0 = std::chrono::steady_clock::now();
    int64_t seq = 0;
    for (int64_t o2 = 0; o2 < size; o2 += block) {
      const ssize_t r = ::pread(fd, bufs[0], (size_t)std::min(block, size - o2), o2);
      if (r <= 0) break;
      seq += r;
    }
    const double seq_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ::close(fd);
    for (void* b : bufs) aligned_free_io(b);
    ::unlink(path.c_str());
    py::gil_scoped_acquire acq;
    py::dict d;
    d["backend"] = std::string(io->backend());
    d["ok"] = bad.load() == 0 && got.load() == size && seq == size;
    d["aio_mbps"] = size / aio_s / 1e6;
    d["aio_streaming_mbps"] = size / cont_s / 1e6;
    d["sequential_mbps"] = size / seq_s / 1e6;
    return d;
  }, py::arg("path"), py::arg("size"), py::arg("block") = 1 << 20, py::arg("depth") = 16, py::arg("direct") = true,
     py::arg("backend") = "");

  // The provider store's read pattern without the store: `files` files of `file_bytes` written and synced,
  // then read round-robin in `chunk` pieces with `depth` reads kept in flight (O_DIRECT), as a loader
  // streams a job's MOF files. Returns GB/s; the files are removed.
  m.def("device_guard_violations", [] { return uda::gpu::device_guard_violations(); });
  // tests / tools: n idle streams on `device` kept alive until release_idle_streams() (mimics a process
  // whose pooled streams are alive: they change how new streams map onto the hardware queues)
  // tests / tools: a thread keeping `streams` extra streams of this process busy with device copies (and
  // optionally a small kernel) until stop_gpu_noise(): other streams' work sharing the hardware queues
  m.def("start_gpu_noise", [](int device, int streams, int64_t bytes) {
    if (g_noise) return;
    g_noise = new GpuNoise();
    GpuNoise* nz = g_noise;
    nz->thr = std::thread([nz, device, streams, bytes] {
      try {
        HIP_CHECK(hipSetDevice(device));
        std::vector<hipStream_t> ss(streams);
        for (auto& st : ss) HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        gpu::DeviceBuffer a((size_t)bytes * streams), b((size_t)bytes * streams);
        while (!nz->stop.load()) {
          for (int i = 0; i < streams; ++i)
            HIP_CHECK(hipMemcpyAsync(b.as<uint8_t>() + (size_t)i * bytes, a.as<uint8_t>() + (size_t)i * bytes,
                                     (size_t)bytes, hipMemcpyDeviceToDevice, ss[i]));
          for (auto& st : ss) HIP_CHECK(hipStreamSynchronize(st));
          nz->ops.fetch_add(streams);
        }
        for (auto& st : ss) (void)hipStreamDestroy(st);
      } catch (const std::exception& e) {
        UDA_LOG(kError, "gpu noise: %s", e.what());
      }
    });
  });
  m.def("stop_gpu_noise", [] {
    if (!g_noise) return (int64_t)0;
    g_noise->stop = true;
    {
      py::gil_scoped_release rel;
      if (g_noise->thr.joinable()) g_noise->thr.join();
    }
    const int64_t n = g_noise->ops.load();
    delete g_noise;
    g_noise = nullptr;
    return n;
  });
  // node topology (uda/topology.h): every GPU of the node with its NUMA node and consumer CPU slice
  // (UDA_SYSFS_ROOT lets a test describe any node); `allowed` empty = no affinity restriction
  m.def("topology_plan", [](const std::vector<int>& allowed) {
    py::list out;
    const auto gpus = node_gpus();
    for (const auto& g : gpus) {
      py::dict d;
      d["bdf"] = g.bdf();
      d["numa_node"] = g.numa_node;
      d["cpus"] = consumer_cpus(g, gpus, allowed);
      out.append(d);
    }
    return out;
  }, py::arg("allowed") = std::vector<int>());
  m.def("lzo_lane_decode_host", [](py::bytes stream, int64_t raw_cap) {
    const std::string in = stream;
    std::string out((size_t)std::max<int64_t>(raw_cap, 1), '\0');
    int64_t n = 0;
    if (!gpu::lzo_lane_decode_host(reinterpret_cast<const uint8_t*>(in.data()), (int64_t)in.size(),
                                   reinterpret_cast<uint8_t*>(&out[0]), raw_cap, &n))
      throw std::runtime_error("lzo lane decode: corrupt block");
    out.resize((size_t)n);
    return py::bytes(out);
  });
  m.def("usable_gpu_bdfs", [] {
    std::vector<std::string> v;
    for (const auto& g : usable_gpus()) v.push_back(g.bdf());
    return v;
  });
  m.def("format_cpulist", &format_cpulist);
  m.def("parse_cpulist", &parse_cpulist);
  // a rank's placement record (bench.py JSON): PCI address, NUMA node, consumer CPU slice
  m.def("device_placement", [](int device) {
    py::dict d;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) == hipSuccess) d["pci"] = std::string(bus);
    d["numa_node"] = gpu::device_numa_node(device);
    d["consumer_cpus"] = format_cpulist(gpu::device_consumer_cpus(device));
    return d;
  });
  // hipDeviceCanAccessPeer over the visible devices: m[i][j] (diagonal 1)
  m.def("peer_access_matrix", [] {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    std::vector<std::vector<int>> m2((size_t)n, std::vector<int>((size_t)n, 0));
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        int can = i == j ? 1 : 0;
        if (i != j && hipDeviceCanAccessPeer(&can, i, j) != hipSuccess) can = -1;
        m2[(size_t)i][(size_t)j] = can;
      }
    return m2;
  });
  m.def("hold_idle_streams", [](int device, int n, int priority) {
    static std::vector<hipStream_t>& held = *new std::vector<hipStream_t>();
    HIP_CHECK(hipSetDevice(device));
    for (int i = 0; i < n; ++i) {
      hipStream_t s = nullptr;
      HIP_CHECK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority));
      held.push_back(s);
    }
    return (int)held.size();
  }, py::arg("device"), py::arg("n"), py::arg("priority") = 0);

  m.def("aio_interleave_bench", [](const std::string& dir, int files, int64_t file_bytes, int64_t chunk, int depth) {
    py::gil_scoped_release rel;
    file_bytes = file_bytes / chunk * chunk;
    std::vector<std::string> paths;
    std::vector<int> fds;
    {
      std::vector<uint8_t> buf((size_t)(8 << 20));
      for (size_t i = 0; i < buf.size(); ++i) buf[i] = (uint8_t)(i * 2654435761u >> 13);
      for (int f = 0; f < files; ++f) {
        paths.push_back(dir + "/uda_interleave." + std::to_string(getpid()) + "." + std::to_string(f));
        const int fd = ::open(paths.back().c_str(), O_CREAT | O_TRUNC | O_WRONLY | O_CLOEXEC, 0600);
        if (fd < 0) throw std::runtime_error("open for write failed");
        for (int64_t off = 0; off < file_bytes; off += (int64_t)buf.size())
          if (::pwrite(fd, buf.data(), (size_t)std::min<int64_t>((int64_t)buf.size(), file_bytes - off), off) <= 0)
            throw std::runtime_error("pwrite failed");
        ::fdatasync(fd);
        ::close(fd);
      }
    }
    for (const auto& p : paths) {
      int fd = ::open(p.c_str(), O_RDONLY | O_CLOEXEC | O_DIRECT);
      if (fd < 0) fd = ::open(p.c_str(), O_RDONLY | O_CLOEXEC);
      if (fd < 0) throw std::runtime_error("open for read failed");
      fds.push_back(fd);
    }
    AsyncIO::Options o;
    o.queue_depth = std::max(depth, 1) * 2;
    auto io = AsyncIO::create(o);
    std::vector<void*> bufs;
    for (int i = 0; i < depth; ++i) bufs.push_back(aligned_alloc_io((size_t)chunk));
    std::mutex m;
    std::condition_variable cv;
    std::vector<int> free_bufs;
    for (int i = 0; i < depth; ++i) free_bufs.push_back(i);
    std::atomic<int64_t> bad{0};
    const auto t0 = std::chrono::steady_clock::now();
    for (int64_t off = 0; off < file_bytes; off += chunk)
      for (int f = 0; f < files; ++f) {
        int bi;
        {
          std::unique_lock<std::mutex> lk(m);
          cv.wait(lk, [&] { return !free_bufs.empty(); });
          bi = free_bufs.back();
          free_bufs.pop_back();
        }
        io->read(fds[(size_t)f], off, chunk, bufs[(size_t)bi], [&, bi](int64_t r) {
          if (r < 0) bad++;
          std::lock_guard<std::mutex> g(m);
          free_bufs.push_back(bi);
          cv.notify_all();
        });
      }
    io->drain();
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int fd : fds) ::close(fd);
    for (void* b : bufs) aligned_free_io(b);
    for (const auto& p : paths) ::unlink(p.c_str());
    if (bad.load()) throw std::runtime_error("interleaved read failed");
    return (double)file_bytes * files / secs / 1e9;
  }, py::arg("dir"), py::arg("files"), py::arg("file_bytes"), py::arg("chunk") = 16 << 20, py::arg("depth") = 16);

  // ---------------------------------------------------------------- bridge (C ABI)
  py::class_<PyBridge, std::shared_ptr<PyBridge>>(m, "Bridge")
      .def(py::init([](bool is_net_merger, const std::vector<std::string>& args, int log_level, py::object fetch_over,
                       py::object data_from_uda, py::object get_path, py::object get_conf, py::object log,
                       py::object failure) {
             auto b = std::make_shared<PyBridge>();
             b->fetch_over = fetch_over;
             b->data_from_uda = data_from_uda;
             b->get_path = get_path;
             b->get_conf = get_conf;
             b->log = log;
             b->failure = failure;
             uda_callbacks cb;
             std::memset(&cb, 0, sizeof(cb));
             cb.ctx = b.get();
             cb.fetch_over = &PyBridge::t_fetch_over;
             cb.data_from_uda = &PyBridge::t_data;
             cb.get_path = &PyBridge::t_get_path;
             cb.get_conf = &PyBridge::t_get_conf;
             cb.log = log.is_none() ? nullptr : &PyBridge::t_log;
             cb.failure = &PyBridge::t_failure;
             std::vector<const char*> argv;
             for (auto& a : args) argv.push_back(a.c_str());
             {
               py::gil_scoped_release r;
               b->h = uda_start(is_net_merger ? 1 : 0, (int)argv.size(), argv.data(), log_level, 0, &cb);
             }
             if (!b->h) throw std::runtime_error("uda_start failed");
             return b;
           }),
           py::arg("is_net_merger"), py::arg("args"), py::arg("log_level") = 3, py::arg("fetch_over") = py::none(),
           py::arg("data_from_uda") = py::none(), py::arg("get_path") = py::none(), py::arg("get_conf") = py::none(),
           py::arg("log") = py::none(), py::arg("failure") = py::none())
      .def("do_command",
           [](PyBridge& b, const std::string& cmd) {
             int r;
             {
               py::gil_scoped_release g;
               r = uda_do_command(b.h, cmd.c_str());
             }
             if (r != 0) throw std::runtime_error(std::string("UdaRuntimeException: ") + uda_last_error(b.h));
           })
      .def("reduce_exit",
           [](PyBridge& b) {
             py::gil_scoped_release g;
             return uda_reduce_exit(b.h);
           })
      .def("register_mof",
           [](PyBridge& b, const std::string& job, const std::string& map, py::bytes data,
              const std::vector<int64_t>& index) {
             // the bridge keeps a reference: the data must outlive the provider
             auto keep = std::make_shared<std::string>(data);
             b.keep.push_back(keep);
             return uda_provider_register_mof(b.h, job.c_str(), map.c_str(), keep->data(), (int64_t)keep->size(),
                                              index.data(), (int32_t)(index.size() / 3));
           })
      .def("register_mof_device",
           [](PyBridge& b, const std::string& job, const std::string& map, uintptr_t dev_ptr, int64_t len,
              const std::vector<int64_t>& index, int device) {
             return uda_provider_register_mof_device(b.h, job.c_str(), map.c_str(), reinterpret_cast<const void*>(dev_ptr),
                                                     len, index.data(), (int32_t)(index.size() / 3), device);
           })
      .def("stats", [](PyBridge& b) { return uda_stats_string(b.h); });
  // node-local shared-memory control plane of the IPC exchange (CPU-testable, no HIP)
  py::class_<ShmGroup>(m, "ShmGroup")
      .def(py::init<const std::string&, int, int, size_t, size_t, double>(), py::arg("name"), py::arg("rank"),
           py::arg("world"), py::arg("mailbox_bytes") = 1 << 16, py::arg("outbox_bytes") = 1 << 16,
           py::arg("timeout_s") = 60.0, py::call_guard<py::gil_scoped_release>())
      .def("barrier", [](ShmGroup& g) { g.barrier("python"); }, py::call_guard<py::gil_scoped_release>())
      .def("try_barrier", &ShmGroup::try_barrier, py::call_guard<py::gil_scoped_release>())
      .def("abort", &ShmGroup::abort)
      .def("aborted", &ShmGroup::aborted)
      .def("abort_reason", &ShmGroup::abort_reason)
      .def("publish", [](ShmGroup& g, int c, int64_t v) { g.publish((ShmGroup::Counter)c, v); })
      .def("read", [](ShmGroup& g, int c, int peer) { return g.read((ShmGroup::Counter)c, peer); })
      .def("wait_at_least",
           [](ShmGroup& g, int c, int peer, int64_t v) { g.wait_at_least((ShmGroup::Counter)c, peer, v, "python"); },
           py::call_guard<py::gil_scoped_release>())
      .def("alltoall",
           [](ShmGroup& g, const std::vector<int64_t>& send) {
             if (send.size() % (size_t)g.world()) throw std::runtime_error("alltoall: size not a multiple of world");
             std::vector<int64_t> recv(send.size());
             {
               py::gil_scoped_release nogil;
               g.alltoall_i64(send.data(), recv.data(), send.size() / (size_t)g.world());
             }
             return recv;
           })
      .def("publish_alloc",
           [](ShmGroup& g, py::bytes b, int64_t size) {
             const std::string s = b;
             return g.publish_alloc(s.data(), s.size(), size);
           })
      .def("read_alloc", [](ShmGroup& g, int peer, int id) -> py::object {
        char blob[ShmGroup::kAllocBlob];
        int64_t size = 0;
        if (!g.read_alloc(peer, id, blob, sizeof(blob), &size)) return py::none();
        return py::make_tuple(py::bytes(blob, sizeof(blob)), size);
      });

  // node-local registry of reduce tasks / HBM bytes per GPU (CPU-testable, no HIP)
  py::class_<NodeRegistry>(m, "NodeRegistry")
      .def(py::init<const std::string&>(), py::arg("name") = std::string())
      .def_property_readonly("name", &NodeRegistry::name)
      .def("place_task",
           [](NodeRegistry& r, const std::vector<std::string>& keys, const std::string& tag) {
             const NodeRegistry::Placement p = r.place_task(keys, tag);
             return py::make_tuple(p.index, p.slot);
           })
      .def("add_task", &NodeRegistry::add_task)
      .def("release", &NodeRegistry::release)
      .def("set_bytes", &NodeRegistry::set_bytes, py::arg("key"), py::arg("bytes"), py::arg("resident") = 0)
      .def("usage",
           [](NodeRegistry& r, const std::string& key) {
             const NodeRegistry::Use u = r.usage(key);
             py::dict d;
             d["tasks"] = u.tasks;
             d["bytes"] = u.bytes;
             d["resident"] = u.resident;
             return d;
           })
      .def_property_readonly("reclaimed", &NodeRegistry::reclaimed)
      .def("unlink", &NodeRegistry::unlink);
  m.def("process_running", &process_running, py::arg("pid"), py::arg("start") = 0);
  m.def("process_start_ticks", &process_start_ticks);
  // HBM budget ledger on fake devices (no HIP): tests of admission, trimming and the node-wide total
  m.def("hbm_fake_device", [](int d, int64_t total, const std::string& key) {
    gpu::HbmLedger::get().set_fake_device(d, total, key);
  });
  m.def("hbm_fake_untracked", [](int d, int64_t b) { gpu::HbmLedger::get().set_fake_untracked(d, b); });
  m.def("hbm_configure", [](int d, double conf) { gpu::HbmLedger::get().configure(d, conf); });
  m.def("hbm_alloc", [](int d, int64_t b, bool resident) { gpu::HbmLedger::get().on_alloc(d, b, resident); },
        py::arg("device"), py::arg("bytes"), py::arg("resident") = false);
  m.def("hbm_free", [](int d, int64_t b, bool resident) { gpu::HbmLedger::get().on_free(d, b, resident); },
        py::arg("device"), py::arg("bytes"), py::arg("resident") = false);
  m.def("hbm_headroom", [](int d) { return gpu::HbmLedger::get().headroom(d); });
  m.def("hbm_stats", [](int d) {
    const gpu::HbmLedger::Stats s = gpu::HbmLedger::get().stats(d);
    py::dict o;
    o["budget"] = s.budget;
    o["used"] = s.used;
    o["reserved"] = s.reserved;
    o["peak"] = s.peak;
    o["resident"] = s.resident;
    o["node_bytes"] = s.node_bytes;
    o["trimmed"] = s.trimmed;
    o["over"] = s.over;
    o["waits"] = s.waits;
    o["wait_ms"] = s.wait_ms;
    o["device_peak"] = s.device_peak;
    return o;
  });
  // an idle pool of fake objects: trimmed by the ledger under pressure (returns the pool's id)
  m.def("hbm_fake_pool", [](int d, std::vector<int64_t> sizes) {
    auto objs = std::make_shared<std::vector<int64_t>>(std::move(sizes));
    auto mu = std::make_shared<std::mutex>();
    for (int64_t b : *objs) gpu::HbmLedger::get().on_alloc(d, b);
    gpu::HbmLedger::get().add_pool(
        {[objs, mu, d](int dev, int64_t want) -> int64_t {
           if (dev != d) return 0;
           std::vector<int64_t> drop;
           {
             std::lock_guard<std::mutex> g(*mu);
             std::sort(objs->begin(), objs->end());
             int64_t got = 0;
             while (!objs->empty() && got < want) {
               got += objs->back();
               drop.push_back(objs->back());
               objs->pop_back();
             }
           }
           int64_t freed = 0;
           for (int64_t b : drop) {
             gpu::HbmLedger::get().on_free(d, b);
             freed += b;
           }
           return freed;
         },
         [objs, mu, d](int dev) -> int64_t {
           if (dev != d) return 0;
           std::lock_guard<std::mutex> g(*mu);
           int64_t n = 0;
           for (int64_t b : *objs) n += b;
           return n;
         }});
  });
  struct PyReservation {
    std::unique_ptr<gpu::HbmLedger::Reservation> r;
  };
  py::class_<PyReservation, std::shared_ptr<PyReservation>>(m, "HbmReservation")
      .def_property_readonly("granted", [](PyReservation& p) { return p.r ? p.r->granted() : 0; })
      .def_property_readonly("wait_ms", [](PyReservation& p) { return p.r ? p.r->wait_ms() : 0.0; })
      .def("alloc", [](PyReservation& p, int64_t b) {  // an allocation drawing from the reservation
        if (!p.r) throw std::runtime_error("reservation released");
        auto scope = p.r->bind();
        gpu::HbmLedger::get().on_alloc(p.r->device(), b);
      })
      .def("release", [](PyReservation& p) { p.r.reset(); });
  m.def("hbm_reserve",
        [](int d, int64_t bytes, double timeout_s) {
          auto p = std::make_shared<PyReservation>();
          {
            py::gil_scoped_release nogil;
            p->r = gpu::HbmLedger::get().reserve(d, bytes, nullptr, timeout_s);
            // the Python thread is not where the allocations happen: unbind (alloc() binds per call)
            p->r->unbind();
          }
          return p;
        },
        py::arg("device"), py::arg("bytes"), py::arg("timeout_s") = 30.0);

  m.def("set_log_level", &uda_set_log_level);

  // ---------------------------------------------------------------- GPU engine
  // the provider's HBM store of MOF files on its own (gpu/mof_cache.h): loads, holders, eviction
  py::class_<gpu::MofCache>(m, "MofStore")
      .def(py::init([](int64_t capacity, std::vector<int> devices, double lease_s, int64_t chunk_bytes,
                       double idle_evict_s, bool cached_read) {
             gpu::MofCache::Options o;
             o.capacity = capacity;
             o.devices = devices;
             o.lease_s = lease_s;
             o.chunk_bytes = chunk_bytes;
             o.idle_evict_s = idle_evict_s;
             o.cached_read = cached_read;
             return new gpu::MofCache(o);
           }),
           py::arg("capacity"), py::arg("devices") = std::vector<int>{0}, py::arg("lease_s") = 600.0,
           py::arg("chunk_bytes") = 16 << 20, py::arg("idle_evict_s") = 0.0, py::arg("cached_read") = true)
      .def("acquire",
           [](gpu::MofCache& c, const std::string& job, const std::string& path, const std::string& holder) {
             gpu::MofCache::Ref r;
             std::string why;
             bool ok;
             {
               py::gil_scoped_release nogil;
               ok = c.acquire(job, path, holder, &r, &why);
             }
             return py::make_tuple(ok, why, (uint64_t)(uintptr_t)r.data, r.len, r.device);
           })
      .def("release", &gpu::MofCache::release)
      .def("release_holder", &gpu::MofCache::release_holder)
      .def("job_over", &gpu::MofCache::job_over)
      .def("stats", [](gpu::MofCache& c) {
        const gpu::MofCache::Stats s = c.stats();
        py::dict d;
        d["loads"] = s.loads;
        d["hits"] = s.hits;
        d["declined"] = s.declined;
        d["evictions"] = s.evictions;
        d["bytes_loaded"] = s.bytes_loaded;
        d["resident_bytes"] = s.resident_bytes;
        d["holders"] = s.holders;
        d["holders_reaped"] = s.holders_reaped;
        d["releases"] = s.releases;
        d["cached_reads"] = s.cached_reads;
        return d;
      });
  m.def("reducer_holder_id", &gpu::reducer_holder_id);
  // the merge service's peer-credential rule (mapred.uda.gpu.merge.service.users)
  m.def("merge_service_user_allowed", [](const std::string& users, int uid) {
    return MergeService::user_allowed(users, (uid_t)uid);
  });
  m.def("merge_service_default_path", &MergeService::default_path);
  // fetch throughput of the TCP transport alone: every listed partition fetched whole into one buffer,
  // `maps_at_once` partitions at a time with `depth` requests of `chunk` bytes in flight each
  m.def("tcp_fetch_probe", [](const std::string& host, int port, const std::string& job,
                              const std::vector<std::string>& maps, int reduce, const std::vector<int64_t>& sizes,
                              int64_t chunk, int depth, int connections, int maps_at_once) {
    auto nogil = std::make_unique<py::gil_scoped_release>();
    auto cl = make_tcp_client(port, 256, connections);
    int64_t total = 0;
    std::vector<int64_t> base(maps.size() + 1, 0);
    for (size_t i = 0; i < maps.size(); ++i) base[i + 1] = base[i] + sizes[i];
    total = base.back();
    std::unique_ptr<uint8_t[]> buf(new uint8_t[(size_t)std::max<int64_t>(total, 1)]);
    std::mutex m;
    std::condition_variable cv;
    std::string err;
    const auto t0 = std::chrono::steady_clock::now();
    std::atomic<size_t> next_map{0};
    std::vector<std::thread> ts;
    for (int w = 0; w < std::max(1, maps_at_once); ++w)
      ts.emplace_back([&] {
        for (size_t i; (i = next_map++) < maps.size();) {
          int inflight = 0;
          int64_t at = 0;
          std::unique_lock<std::mutex> lk(m);
          while (at < sizes[i] || inflight > 0) {
            while (at < sizes[i] && inflight < depth && err.empty()) {
              FetchRequest rq;
              rq.job_id = job;
              rq.map_id = maps[i];
              rq.reduce_id = reduce;
              rq.fetched = at;
              rq.buf_len = std::min(chunk, sizes[i] - at);
              at += rq.buf_len;
              ++inflight;
              lk.unlock();
              cl->fetch(host, rq, buf.get() + base[i] + rq.fetched, [&](const FetchAck& a) {
                std::lock_guard<std::mutex> g(m);
                if (a.status != 0 && err.empty()) err = a.error;
                --inflight;
                cv.notify_all();
              });
              lk.lock();
            }
            if (!err.empty() && inflight == 0) break;
            cv.wait(lk, [&] { return inflight == 0 || (at < sizes[i] && inflight < depth && err.empty()); });
            if (!err.empty() && inflight == 0) break;
          }
        }
      });
    for (auto& t : ts) t.join();
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    cl->close();
    uint64_t sum = 0;
    for (int64_t k = 0; k < total; k += 4096) sum += buf[(size_t)k];
    nogil.reset();  // the GIL again before any Python object is made
    if (!err.empty()) throw std::runtime_error("tcp_fetch_probe: " + err);
    return py::make_tuple(total, s, sum);
  });
  // one TCP client, a fetch to an unreachable host on one thread and, while it is still trying, one to a
  // live host: returns (live fetch ms, dead host error, dead host ms, second dead fetch ms)
  m.def("mof_host_is_local", &uda::mof_host_is_local);
  m.def("local_mof_readable", [](const std::string& path, int64_t off, int64_t len) {
    const int fd = uda::open_local_mof(path, off, len);
    if (fd >= 0) ::close(fd);
    return fd >= 0;
  });
  // ACK string codec (transport.h): format then parse, as a TCP reducer sees the provider's answer
  m.def("ack_roundtrip", [](int status, int64_t raw_len, int64_t part_len, int64_t sent, int64_t mof_offset,
                            const std::string& path, const std::string& error) {
    uda::FetchAck a;
    a.status = status;
    a.raw_len = raw_len;
    a.part_len = part_len;
    a.sent = sent;
    a.mof_offset = mof_offset;
    a.path = path;
    a.error = error;
    uda::FetchAck b;
    if (!uda::parse_ack(uda::format_ack(a), &b)) throw std::runtime_error("ack does not parse");
    py::dict d;
    d["status"] = b.status;
    d["raw_len"] = b.raw_len;
    d["part_len"] = b.part_len;
    d["sent"] = b.sent;
    d["mof_offset"] = b.mof_offset;
    d["path"] = b.path;
    d["error"] = b.error;
    return d;
  });
  m.def("tcp_dead_host_probe", [](const std::string& live, const std::string& dead, int port, const std::string& job,
                                  const std::string& map, int reduce, int64_t size) {
    py::gil_scoped_release rel;
    auto cl = make_tcp_client(port, 256, 4);
    std::unique_ptr<uint8_t[]> a(new uint8_t[(size_t)std::max<int64_t>(size, 1)]), b(new uint8_t[64]);
    auto fetch = [&](const std::string& host, uint8_t* dst, int64_t len, std::string* err) {
      std::mutex m;
      std::condition_variable cv;
      bool done = false;
      FetchRequest rq;
      rq.job_id = job;
      rq.map_id = map;
      rq.reduce_id = reduce;
      rq.buf_len = len;
      const auto t0 = std::chrono::steady_clock::now();
      cl->fetch(host, rq, dst, [&](const FetchAck& k) {
        std::lock_guard<std::mutex> g(m);
        if (k.status != 0) *err = k.error.empty() ? "status " + std::to_string(k.status) : k.error;
        done = true;
        cv.notify_all();
      });
      std::unique_lock<std::mutex> lk(m);
      cv.wait(lk, [&] { return done; });
      return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    std::string dead_err, live_err, dead2_err;
    double dead_ms = 0;
    std::thread t([&] { dead_ms = fetch(dead, b.get(), 64, &dead_err); });
    std::this_thread::sleep_for(std::chrono::milliseconds(100));
    const double live_ms = fetch(live, a.get(), size, &live_err);
    t.join();
    const double dead2_ms = fetch(dead, b.get(), 64, &dead2_err);
    cl->close();
    if (!live_err.empty()) throw std::runtime_error("live host fetch failed: " + live_err);
    return std::make_tuple(live_ms, dead_err, dead_ms, dead2_ms);
  });
  m.def("open_ipc_mappings", &gpu::open_ipc_mappings);
  m.def("device_read", [](uint64_t addr, int64_t len) {  // device bytes back to the host (tests)
    std::string out((size_t)len, '\0');
    if (len > 0) HIP_CHECK(hipMemcpy(out.data(), reinterpret_cast<const void*>((uintptr_t)addr), (size_t)len,
                                     hipMemcpyDeviceToHost));
    return py::bytes(out);
  });
  m.def("device_count", &gpu::device_count);
  m.def("ipc_safe_bytes", [](uint64_t b) { return (uint64_t)gpu::ipc_safe_bytes((size_t)b); });
  m.def("ipc_size_ok", [](uint64_t b) { return gpu::ipc_size_ok((size_t)b); });
  m.def("node_id", []() { return gpu::node_id(); });
  // (address or None, reason): what a reducer does with a provider's descriptor
  m.def("descriptor_resolve", [](const std::string& desc, int device) -> py::tuple {
    std::string why;
    const uint8_t* p = gpu::try_resolve_device_descriptor(desc, device, &why);
    if (!p) return py::make_tuple(py::none(), why);
    return py::make_tuple((uint64_t)(uintptr_t)p, why);
  });
  m.def("descriptor_make", [](int device, uint64_t addr, const std::string& handle_hex, uint64_t base) {
    gpu::IpcExport ex;
    ex.handle_hex = handle_hex;
    ex.base = reinterpret_cast<const uint8_t*>((uintptr_t)base);
    return gpu::make_device_descriptor(device, reinterpret_cast<const uint8_t*>((uintptr_t)addr), ex);
  });
  // N8 device discovery: per-pair P2P reachability, link type (HSA_AMD_LINK_INFO_TYPE_*: 2 = xGMI) and
  // hop count, and the runtime's relative performance rank.
  m.def("device_topology", []() {
    py::dict d;
    int n = gpu::device_count();
    d["devices"] = n;
    py::list props, links;
    for (int i = 0; i < n; ++i) {
      hipDeviceProp_t p;
      if (hipGetDeviceProperties(&p, i) != hipSuccess) continue;
      py::dict e;
      e["name"] = std::string(p.name);
      e["arch"] = std::string(p.gcnArchName);
      e["cus"] = p.multiProcessorCount;
      e["hbm_bytes"] = (int64_t)p.totalGlobalMem;
      e["lds_bytes"] = (int64_t)p.sharedMemPerBlock;
      e["l2_bytes"] = p.l2CacheSize;
      e["pci_bus"] = p.pciBusID;
      props.append(e);
      for (int j = 0; j < n; ++j) {
        if (i == j) continue;
        int can = 0, rank = -1;
        uint32_t type = 0, hops = 0;
        (void)hipDeviceCanAccessPeer(&can, i, j);
        (void)hipDeviceGetP2PAttribute(&rank, hipDevP2PAttrPerformanceRank, i, j);
        (void)hipExtGetLinkTypeAndHopCount(i, j, &type, &hops);
        py::dict l;
        l["src"] = i;
        l["dst"] = j;
        l["p2p"] = can != 0;
        l["link_type"] = type;
        l["hops"] = hops;
        l["perf_rank"] = rank;
        links.append(l);
      }
    }
    d["props"] = props;
    d["links"] = links;
    return d;
  });
  // The constants of the generic merge kernels (F1 index, K-way cells, pairwise tiles, key compare), for
  // tests that place their inputs on those boundaries. Plain numbers: callable without a device.
  m.def("gpu_generic_geometry", [] {
    py::dict d;
    d["f1_chunk"] = gpu::f1_chunk_bytes();
    d["f1_halo"] = gpu::f1_halo_bytes();
    d["f1_entries"] = gpu::f1_entries();
    d["f1_super_chunks"] = gpu::f1_super_chunks();
    d["f1_chase"] = gpu::f1_chase_survivors();
    d["gk_cap"] = gpu::generic_kway_cap();
    d["gk_max_runs"] = gpu::kGkMaxRuns;
    d["generic_tile"] = gpu::kGenericMergeTile;
    d["staged_key_bytes"] = gpu::generic_staged_key_bytes();
    d["len_cap"] = gpu::generic_len_cap();
    return d;
  });
  // The constants of the key-range round planner (generic_rounds.h). Callable without a device.
  m.def("gpu_rounds_geometry", [] {
    py::dict d;
    d["sample_key"] = gpu::kSampleKey;
    d["samples_per_round"] = gpu::kSamplesPerRound;
    return d;
  });
  // The two planners of generic_rounds.h on their own (tests). Every run lies in a device allocation of its
  // own and starts `misalign` bytes past that allocation's 256-byte-aligned base: partitions sit at any
  // offset of a MOF, progressive windows start at any byte.
  struct RoundRuns {
    std::vector<gpu::DeviceBuffer> bufs;
    std::vector<const uint8_t*> ptrs;
    std::vector<int64_t> bytes;
    hipStream_t s = nullptr;
    ~RoundRuns() {
      if (s) (void)hipStreamDestroy(s);
    }
    void upload(const std::vector<std::string>& runs, int misalign, int device) {
      if (misalign < 0 || misalign > 255) throw py::value_error("misalign must be 0..255");
      HIP_CHECK(hipSetDevice(device));
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      bufs.resize(runs.size());
      for (size_t i = 0; i < runs.size(); ++i) {
        bufs[i].alloc_local(runs[i].size() + (size_t)misalign + 256);
        uint8_t* base = bufs[i].as<uint8_t>();
        if ((uintptr_t)base & 255) throw UdaError("device allocation is not 256-byte aligned");
        if (!runs[i].empty())
          HIP_CHECK(hipMemcpyAsync(base + misalign, runs[i].data(), runs[i].size(), hipMemcpyHostToDevice, s));
        ptrs.push_back(base + misalign);
        bytes.push_back((int64_t)runs[i].size());
      }
      HIP_CHECK(hipStreamSynchronize(s));
    }
  };
  // plan_generic_rounds over whole runs: {"rounds", "pos": [run][0..rounds], "bounds", "max_round_bytes"}
  m.def("gpu_plan_generic_rounds", [](const std::vector<std::string>& streams, int kind, int64_t round_bytes,
                                      int misalign, int device) {
    gpu::GenericRoundsPlan plan;
    {
      py::gil_scoped_release rel;
      RoundRuns rr;
      rr.upload(streams, misalign, device);
      gpu::GenericRoundsWs ws;
      plan = gpu::plan_generic_rounds(rr.ptrs, rr.bytes, kind, round_bytes, ws, rr.s);
    }
    py::list pos, bounds;
    for (size_t k = 0; k < streams.size(); ++k) {
      py::list row;
      for (int q = 0; q <= plan.rounds; ++q) row.append(plan.at((int)k, q));
      pos.append(row);
    }
    for (const std::string& b : plan.bounds) bounds.append(py::bytes(b));
    py::dict d;
    d["rounds"] = plan.rounds;
    d["pos"] = pos;
    d["bounds"] = bounds;
    d["max_round_bytes"] = plan.max_round_bytes;
    return d;
  }, py::arg("streams"), py::arg("kind"), py::arg("round_bytes"), py::arg("misalign") = 0, py::arg("device") = 0);
  // plan_progressive_split: windows[k] is uploaded whole, its first avail[k] bytes count as landed.
  // {"complete", "split", "bounded", "bound"}
  m.def("gpu_plan_progressive_split", [](const std::vector<std::string>& windows, const std::vector<int64_t>& avail,
                                         const std::vector<bool>& final_run, int kind, int misalign, int device) {
    if (avail.size() != windows.size() || final_run.size() != windows.size())
      throw py::value_error("windows, avail and final differ in length");
    for (size_t k = 0; k < windows.size(); ++k)
      if (avail[k] < 0 || avail[k] > (int64_t)windows[k].size()) throw py::value_error("avail outside its window");
    gpu::ProgressiveSplit ps;
    {
      py::gil_scoped_release rel;
      RoundRuns rr;
      rr.upload(windows, misalign, device);
      gpu::GenericRoundsWs ws;
      const std::vector<char> fin(final_run.begin(), final_run.end());
      ps = gpu::plan_progressive_split(rr.ptrs, avail, fin, kind, ws, rr.s);
    }
    py::dict d;
    d["complete"] = ps.complete;
    d["split"] = ps.split;
    d["bounded"] = ps.bounded;
    d["bound"] = py::bytes(ps.bound);
    return d;
  }, py::arg("windows"), py::arg("avail"), py::arg("final"), py::arg("kind"), py::arg("misalign") = 0,
        py::arg("device") = 0);
  // Merge IFile runs (any bytes-like objects, read in place) on the device. Returns
  // (merged bytes, buffer cuts, records, merge passes, device merge ms, runs indexed serially, records merged).
  // combine: "none" or an op of uda/combine.h (sum.int, sum.long, min.int, max.int, min.long, max.long,
  // sum.vint, sum.vlong): records then counts the groups delivered.
  m.def("gpu_merge_runs", [](const py::list& runs, const std::string& key_class, int64_t kv_buf, int device,
                             const std::string& combine, const std::string& key_order) {
    KeyKind kind = key_kind_arg(key_class, key_order);
    const CombineOp cop = combine_op_arg(combine);
    std::vector<py::buffer_info> views;
    std::vector<const uint8_t*> host;
    std::vector<int64_t> bytes;
    int64_t total = 0;
    for (auto h : runs) {
      views.push_back(py::reinterpret_borrow<py::buffer>(h).request());
      host.push_back(static_cast<const uint8_t*>(views.back().ptr));
      bytes.push_back((int64_t)(views.back().size * views.back().itemsize));
      total += bytes.back();
    }
    std::vector<int64_t> cuts;
    int64_t records = 0, records_in = 0, out_bytes = 0;
    int passes = 0, serial_runs = 0;
    double merge_ms = 0;
    gpu::DeviceBuffer in, dout;
    hipStream_t s = nullptr;
    struct StreamDrop {  // a merge that throws (a value the combiner cannot sum) leaves no stream behind
      hipStream_t& s;
      ~StreamDrop() {
        if (s) (void)hipStreamDestroy(s);
      }
    } stream_drop{s};
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      in.alloc((size_t)std::max<int64_t>(total, 16));
      dout.alloc((size_t)std::max<int64_t>(total, 16));
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      std::vector<const uint8_t*> ptrs;
      int64_t off = 0;
      for (size_t i = 0; i < host.size(); ++i) {
        if (bytes[i]) HIP_CHECK(hipMemcpyAsync(in.as<uint8_t>() + off, host[i], (size_t)bytes[i], hipMemcpyHostToDevice, s));
        ptrs.push_back(in.as<uint8_t>() + off);
        off += bytes[i];
      }
      // one merger (and its HBM workspace) per device for the process, like the NetMerger's pooled
      // DeviceWorkspace: a reducer process merges many times, so only the first call allocates
      static std::mutex gm_mu;
      static auto* gm_cache = new std::map<int, std::unique_ptr<gpu::GenericMerger>>();  // outlives HIP at exit
      std::unique_lock<std::mutex> gm_lock(gm_mu);
      auto& gm_slot = (*gm_cache)[device];
      if (!gm_slot) gm_slot.reset(new gpu::GenericMerger());
      gpu::GenericMerger& gm = *gm_slot;
      HIP_CHECK(hipStreamSynchronize(s));
      auto t0 = std::chrono::steady_clock::now();
      auto res = gm.merge(ptrs, bytes, (int)kind, dout.as<uint8_t>(), total, kv_buf, s, nullptr, 256ll << 20, cop);
      HIP_CHECK(hipStreamSynchronize(s));
      merge_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      cuts = res.cuts;
      records = res.records;
      records_in = res.records_in;
      passes = res.passes;
      out_bytes = res.bytes;
      serial_runs = gm.f1_serial_runs();
    }
    views.clear();
    // the result is copied D2H straight into the bytes object's storage
    PyObject* o = PyBytes_FromStringAndSize(nullptr, (Py_ssize_t)out_bytes);
    if (!o) throw py::error_already_set();
    py::bytes out = py::reinterpret_steal<py::bytes>(o);
    {
      py::gil_scoped_release rel;
      if (out_bytes) HIP_CHECK(hipMemcpyAsync(PyBytes_AS_STRING(o), dout.as(), (size_t)out_bytes, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      HIP_CHECK(hipStreamDestroy(s));
      s = nullptr;
      in.reset();
      dout.reset();
    }
    return py::make_tuple(out, cuts, records, passes, merge_ms, serial_runs, records_in);
  }, py::arg("runs"), py::arg("key_class"), py::arg("kv_buf") = 1 << 20, py::arg("device") = 0,
        py::arg("combine") = "none", py::arg("key_order") = "reference");
  // The same merge handed over in key-range rounds of about round_bytes (GenericMerger::merge's on_round,
  // recorded here). Returns (merged bytes, cuts, records, records merged, rounds, held records), rounds a
  // list of (records, absolute cuts) per on_round call. gpu_merge_streamed_last_rounds(): the on_round
  // calls of the most recent call, also of one that raised.
  static std::atomic<int> streamed_last_rounds{0};
  m.def("gpu_merge_streamed_last_rounds", [] { return streamed_last_rounds.load(); });
  m.def("gpu_merge_runs_streamed", [](const py::list& runs, const std::string& key_class, int64_t kv_buf,
                                      int64_t round_bytes, int device, const std::string& combine,
                                      const std::string& key_order) {
    KeyKind kind = key_kind_arg(key_class, key_order);
    if (round_bytes <= 0) throw py::value_error("round_bytes must be positive");
    const CombineOp cop = combine_op_arg(combine);
    std::vector<py::buffer_info> views;
    std::vector<const uint8_t*> host;
    std::vector<int64_t> bytes;
    int64_t total = 0;
    for (auto h : runs) {
      views.push_back(py::reinterpret_borrow<py::buffer>(h).request());
      host.push_back(static_cast<const uint8_t*>(views.back().ptr));
      bytes.push_back((int64_t)(views.back().size * views.back().itemsize));
      total += bytes.back();
    }
    gpu::GenericMergeResult res;
    std::vector<std::pair<int64_t, std::vector<int64_t>>> calls;
    std::vector<uint8_t> merged;
    streamed_last_rounds = 0;
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      gpu::DeviceBuffer in, dout;
      in.alloc((size_t)std::max<int64_t>(total, 16));
      dout.alloc((size_t)std::max<int64_t>(total, 16));
      gpu::GenericMerger gm;  // before the stream: its workspace outlives whatever a failed merge left queued
      hipStream_t s = nullptr;
      struct StreamDrop {
        hipStream_t& s;
        ~StreamDrop() {
          if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
          }
        }
      } stream_drop{s};
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      std::vector<const uint8_t*> ptrs;
      int64_t off = 0;
      for (size_t i = 0; i < host.size(); ++i) {
        if (bytes[i]) HIP_CHECK(hipMemcpyAsync(in.as<uint8_t>() + off, host[i], (size_t)bytes[i], hipMemcpyHostToDevice, s));
        ptrs.push_back(in.as<uint8_t>() + off);
        off += bytes[i];
      }
      HIP_CHECK(hipStreamSynchronize(s));
      bool closed = false;
      res = gm.merge(ptrs, bytes, (int)kind, dout.as<uint8_t>(), total, kv_buf, s,
                     [&](const std::vector<int64_t>& cuts, int64_t records, bool last) {
                       if (closed) throw std::runtime_error("on_round after the last round");
                       closed = last;
                       calls.emplace_back(records, cuts);
                       ++streamed_last_rounds;
                     },
                     round_bytes, cop);
      HIP_CHECK(hipStreamSynchronize(s));
      if (!calls.empty() && !closed) throw std::runtime_error("the final on_round call did not say last");
      merged.resize((size_t)res.bytes);
      if (res.bytes) HIP_CHECK(hipMemcpy(merged.data(), dout.as(), (size_t)res.bytes, hipMemcpyDeviceToHost));
    }
    py::list rounds;
    for (auto& c : calls) rounds.append(py::make_tuple(c.first, c.second));
    return py::make_tuple(py::bytes(reinterpret_cast<const char*>(merged.data()), merged.size()), res.cuts, res.records,
                          res.records_in, rounds, res.held_records);
  }, py::arg("runs"), py::arg("key_class"), py::arg("kv_buf"), py::arg("round_bytes"), py::arg("device") = 0,
        py::arg("combine") = "none", py::arg("key_order") = "reference");
  // F8: sort TeraSort records (104-byte IFile records, no EOF marker) by their 10-byte key on the
  // device; returns (sorted bytes, device ms of the sort).
  m.def("gpu_sort_fixed", [](py::buffer b, int device, bool staged) {
    py::buffer_info v = b.request();
    const int64_t bytes = (int64_t)(v.size * v.itemsize);
    if (bytes % gpu::kTeraRecordBytes) throw py::value_error("not a whole number of 104-byte records");
    const int64_t n = bytes / gpu::kTeraRecordBytes;
    if (n >= (int64_t)UINT32_MAX) throw py::value_error("too many records");
    PyObject* o = PyBytes_FromStringAndSize(nullptr, (Py_ssize_t)bytes);
    if (!o) throw py::error_already_set();
    py::bytes out = py::reinterpret_steal<py::bytes>(o);
    float ms = 0;
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      gpu::DeviceBuffer d, ws;
      d.alloc((size_t)std::max<int64_t>(bytes + 2, 16));
      ws.alloc((size_t)gpu::sort_fixed_ws_bytes(std::max<int64_t>(n, 1)));
      hipStream_t s = nullptr;
      hipEvent_t e0 = nullptr, e1 = nullptr;
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      HIP_CHECK(hipEventCreate(&e0));
      HIP_CHECK(hipEventCreate(&e1));
      // staged: input in the workspace's record area, sorted run gathered into d (+ EOF marker)
      uint8_t* in = staged ? gpu::sort_fixed_ws_records(ws.as(), std::max<int64_t>(n, 1)) : d.as<uint8_t>();
      if (bytes) HIP_CHECK(hipMemcpyAsync(in, v.ptr, (size_t)bytes, hipMemcpyHostToDevice, s));
      gpu::launch_sort_fixed_run(d.as<uint8_t>(), n, ws.as(), s, staged);  // warm-up (first launch loads code)
      if (bytes) HIP_CHECK(hipMemcpyAsync(in, v.ptr, (size_t)bytes, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipEventRecord(e0, s));
      gpu::launch_sort_fixed_run(d.as<uint8_t>(), n, ws.as(), s, staged);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipEventRecord(e1, s));
      if (bytes) HIP_CHECK(hipMemcpyAsync(PyBytes_AS_STRING(o), d.as(), (size_t)bytes, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
      (void)hipEventDestroy(e0);
      (void)hipEventDestroy(e1);
      (void)hipStreamDestroy(s);
    }
    return py::make_tuple(out, (double)ms);
  }, py::arg("records"), py::arg("device") = 0, py::arg("staged") = false);

  // Test hooks of the device validators and of the TeraGen kernel (tests/test_gpu_validate.py): each runs the
  // launcher on a stream of its own, synchronises and returns what the device wrote.
  struct TestStream {
    hipStream_t s = nullptr;
    TestStream() { HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    ~TestStream() {
      (void)hipStreamSynchronize(s);
      (void)hipStreamDestroy(s);
    }
  };
  // FIXED10 slices laid end to end in one device buffer (a record is 104 bytes, so every slice is 8-byte aligned)
  struct DeviceSlices {
    gpu::DeviceBuffer data, descs;
    int64_t largest = 0;
    DeviceSlices(const std::vector<std::string>& slices, hipStream_t s) {
      size_t total = 0;
      for (const auto& b : slices) {
        if (b.size() % (size_t)gpu::kTeraRecordBytes) throw py::value_error("need whole 104-byte records");
        total += b.size();
      }
      data.alloc(std::max<size_t>(total, 16));
      std::vector<gpu::RunDesc> rd(slices.size());
      size_t at = 0;
      for (size_t i = 0; i < slices.size(); ++i) {
        rd[i].base = data.as<uint8_t>() + at;
        rd[i].nbytes = (int64_t)slices[i].size();
        rd[i].nrec = rd[i].nbytes / gpu::kTeraRecordBytes;
        rd[i].offsets = nullptr;
        largest = std::max(largest, rd[i].nrec);
        if (!slices[i].empty())
          HIP_CHECK(hipMemcpyAsync(data.as<uint8_t>() + at, slices[i].data(), slices[i].size(), hipMemcpyHostToDevice, s));
        at += slices[i].size();
      }
      descs.alloc(std::max<size_t>(rd.size() * sizeof(gpu::RunDesc), 16));
      if (!rd.empty())
        HIP_CHECK(hipMemcpyAsync(descs.as(), rd.data(), rd.size() * sizeof(gpu::RunDesc), hipMemcpyHostToDevice, s));
      HIP_CHECK(hipStreamSynchronize(s));  // rd goes out of scope
    }
  };
  // Order errors, checksum and last key of the chunks taken as one stream: one launch_validate_fixed per
  // non-empty chunk, chained as ShuffleJob::run_step chains a reducer's rounds.
  m.def("gpu_validate_fixed", [](const std::vector<std::string>& chunks, int device) {
    for (const auto& c : chunks)
      if (c.size() % (size_t)gpu::kTeraRecordBytes) throw py::value_error("need whole 104-byte records");
    unsigned long long host[8] = {0};  // stats[2], group_ck, pad, prev key, last key
    bool any = false;
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      gpu::DeviceBuffer state(sizeof(host));
      std::vector<gpu::DeviceBuffer> bufs;
      TestStream ts;
      unsigned long long* stats = state.as<unsigned long long>();
      gpu::Elem* prev = reinterpret_cast<gpu::Elem*>(stats + 4);
      gpu::Elem* last = prev + 1;
      HIP_CHECK(hipMemsetAsync(state.as(), 0, sizeof(host), ts.s));
      for (const auto& c : chunks) {
        if (c.empty()) continue;
        bufs.emplace_back(std::max<size_t>(c.size(), 16));
        HIP_CHECK(hipMemcpyAsync(bufs.back().as(), c.data(), c.size(), hipMemcpyHostToDevice, ts.s));
        gpu::launch_validate_fixed(bufs.back().as<uint8_t>(), (int64_t)c.size() / gpu::kTeraRecordBytes, prev,
                                   any ? 1 : 0, last, stats, ts.s, stats + 2);
        HIP_CHECK(hipMemcpyAsync(prev, last, sizeof(gpu::Elem), hipMemcpyDeviceToDevice, ts.s));
        any = true;
      }
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(host, state.as(), sizeof(host), hipMemcpyDeviceToHost, ts.s));
      HIP_CHECK(hipStreamSynchronize(ts.s));
    }
    char key[10];
    for (int b = 0; b < 8; ++b) key[b] = (char)(host[6] >> (56 - 8 * b));
    key[8] = (char)(host[7] >> 56);
    key[9] = (char)(host[7] >> 48);
    py::dict d;
    d["order_errors"] = host[0];
    d["checksum"] = host[1];
    d["group_ck"] = host[2];
    d["last_key"] = py::bytes(key, any ? sizeof(key) : 0);
    return d;
  }, py::arg("chunks"), py::arg("device") = 0);
  // launch_slice_checksums over the slices; max_nrec (default: the largest slice) sizes the grid as the
  // engine does, so 1 gives one block per slice. The output starts as ff bytes: the launcher zeroes it.
  m.def("gpu_slice_checksums", [](const std::vector<std::string>& slices, const py::object& max_nrec, int device) {
    const int64_t forced = max_nrec.is_none() ? -1 : max_nrec.cast<int64_t>();
    const int n = (int)slices.size();
    if (n > 65535) throw py::value_error("more slices than one launch takes (65535)");
    std::vector<uint64_t> out((size_t)n);
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      TestStream ts;
      DeviceSlices in(slices, ts.s);
      gpu::DeviceBuffer ck(std::max<size_t>((size_t)n * 8, 16));
      HIP_CHECK(hipMemsetAsync(ck.as(), 0xFF, ck.size(), ts.s));
      gpu::launch_slice_checksums(in.descs.as<gpu::RunDesc>(), n, forced >= 0 ? forced : in.largest,
                                  ck.as<unsigned long long>(), ts.s);
      HIP_CHECK(hipGetLastError());
      if (n) HIP_CHECK(hipMemcpyAsync(out.data(), ck.as(), (size_t)n * 8, hipMemcpyDeviceToHost, ts.s));
      HIP_CHECK(hipStreamSynchronize(ts.s));
    }
    return out;
  }, py::arg("slices"), py::arg("max_nrec") = py::none(), py::arg("device") = 0);
  // launch_check_fixed over the slices: True when every record has the TeraSort layout.
  m.def("gpu_check_fixed", [](const std::vector<std::string>& slices, const py::object& max_nrec, int device) {
    const int64_t forced = max_nrec.is_none() ? -1 : max_nrec.cast<int64_t>();
    const int n = (int)slices.size();
    if (n > 65535) throw py::value_error("more slices than one launch takes (65535)");
    int bad = 0;
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      TestStream ts;
      DeviceSlices in(slices, ts.s);
      gpu::DeviceBuffer flag(16);
      HIP_CHECK(hipMemsetAsync(flag.as(), 0, 16, ts.s));
      gpu::launch_check_fixed(in.descs.as<gpu::RunDesc>(), n, forced >= 0 ? forced : in.largest, flag.as<int>(), ts.s);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(&bad, flag.as(), sizeof(bad), hipMemcpyDeviceToHost, ts.s));
      HIP_CHECK(hipStreamSynchronize(ts.s));
    }
    return bad == 0;
  }, py::arg("slices"), py::arg("max_nrec") = py::none(), py::arg("device") = 0);
  // launch_count_mismatch: `start` plus the number of positions where the two word lists differ.
  m.def("gpu_count_mismatch", [](const std::vector<uint64_t>& a, const std::vector<uint64_t>& b, uint64_t start,
                                 int device) {
    if (a.size() != b.size()) throw py::value_error("gpu_count_mismatch: the lists differ in length");
    if (a.size() > (size_t)INT32_MAX) throw py::value_error("gpu_count_mismatch: too long");
    unsigned long long errors = start;
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      TestStream ts;
      const size_t bytes = a.size() * 8;
      gpu::DeviceBuffer da(std::max<size_t>(bytes, 16)), db(std::max<size_t>(bytes, 16)), de(16);
      if (bytes) {
        HIP_CHECK(hipMemcpyAsync(da.as(), a.data(), bytes, hipMemcpyHostToDevice, ts.s));
        HIP_CHECK(hipMemcpyAsync(db.as(), b.data(), bytes, hipMemcpyHostToDevice, ts.s));
      }
      HIP_CHECK(hipMemcpyAsync(de.as(), &errors, 8, hipMemcpyHostToDevice, ts.s));
      gpu::launch_count_mismatch(da.as<unsigned long long>(), db.as<unsigned long long>(), (int)a.size(),
                                 de.as<unsigned long long>(), ts.s);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(&errors, de.as(), 8, hipMemcpyDeviceToHost, ts.s));
      HIP_CHECK(hipStreamSynchronize(ts.s));
    }
    return (uint64_t)errors;
  }, py::arg("a"), py::arg("b"), py::arg("start") = 0, py::arg("device") = 0);
  // The contract of sorted generation (kernels.h): raises ValueError when a run's key span is below its
  // record count. No device needed.
  m.def("teragen_require_spans", [](const std::vector<int64_t>& nrec, const std::vector<uint64_t>& key_span) {
    if (nrec.size() != key_span.size()) throw py::value_error("teragen_require_spans: one span per run");
    gpu::require_teragen_spans(nrec.data(), key_span.data(), (int)nrec.size());
  }, py::arg("nrec"), py::arg("key_span"));
  // launch_teragen of all the runs in one launch. Every run's buffer is 104 * n + 2 bytes and 16 guard bytes
  // behind them, all a5 before the launch; returns the buffers whole (guards included) and the checksums.
  m.def("gpu_teragen", [](const std::vector<int64_t>& nrec, const std::vector<uint64_t>& key_lo,
                          const std::vector<uint64_t>& key_span, const std::vector<uint64_t>& seeds, bool unsorted,
                          int device) {
    const size_t R = nrec.size();
    if (key_lo.size() != R || key_span.size() != R || seeds.size() != R)
      throw py::value_error("gpu_teragen: one key_lo, key_span and seed per run");
    if (R > 65535) throw py::value_error("gpu_teragen: more runs than one launch takes (65535)");
    constexpr size_t kGuard = 16;
    std::vector<size_t> at(R), len(R);
    size_t total = 0;
    int64_t max_n = 0;
    for (size_t r = 0; r < R; ++r) {
      if (nrec[r] < 0 || nrec[r] > (1 << 24)) throw py::value_error("gpu_teragen: nrec out of range");
      at[r] = total;  // 16-byte aligned
      len[r] = (size_t)nrec[r] * gpu::kTeraRecordBytes + 2 + kGuard;
      total = (total + len[r] + 15) & ~(size_t)15;
      max_n = std::max(max_n, nrec[r]);
    }
    if (!unsorted) gpu::require_teragen_spans(nrec.data(), key_span.data(), (int)R);
    std::vector<uint8_t> host(total);
    std::vector<uint64_t> ck(R);
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      TestStream ts;
      gpu::DeviceBuffer data(std::max<size_t>(total, 16)), args(std::max<size_t>(R * 48, 16));
      std::vector<uint8_t*> bases(R);
      for (size_t r = 0; r < R; ++r) bases[r] = data.as<uint8_t>() + at[r];
      // args: bases, nrec, key_lo, key_span, seeds, checksums (R words each)
      uint64_t* a = args.as<uint64_t>();
      HIP_CHECK(hipMemsetAsync(data.as(), 0xA5, data.size(), ts.s));
      if (R) {
        HIP_CHECK(hipMemcpyAsync(a, bases.data(), R * 8, hipMemcpyHostToDevice, ts.s));
        HIP_CHECK(hipMemcpyAsync(a + R, nrec.data(), R * 8, hipMemcpyHostToDevice, ts.s));
        HIP_CHECK(hipMemcpyAsync(a + 2 * R, key_lo.data(), R * 8, hipMemcpyHostToDevice, ts.s));
        HIP_CHECK(hipMemcpyAsync(a + 3 * R, key_span.data(), R * 8, hipMemcpyHostToDevice, ts.s));
        HIP_CHECK(hipMemcpyAsync(a + 4 * R, seeds.data(), R * 8, hipMemcpyHostToDevice, ts.s));
        HIP_CHECK(hipMemsetAsync(a + 5 * R, 0, R * 8, ts.s));
      }
      gpu::launch_teragen(reinterpret_cast<uint8_t* const*>(a), reinterpret_cast<const int64_t*>(a + R), a + 2 * R,
                          a + 3 * R, a + 4 * R, (int)R, max_n, reinterpret_cast<unsigned long long*>(a + 5 * R), ts.s,
                          unsorted ? 1 : 0);
      HIP_CHECK(hipGetLastError());
      if (total) HIP_CHECK(hipMemcpyAsync(host.data(), data.as(), total, hipMemcpyDeviceToHost, ts.s));
      if (R) HIP_CHECK(hipMemcpyAsync(ck.data(), a + 5 * R, R * 8, hipMemcpyDeviceToHost, ts.s));
      HIP_CHECK(hipStreamSynchronize(ts.s));
    }
    py::list runs;
    for (size_t r = 0; r < R; ++r) runs.append(py::bytes(reinterpret_cast<const char*>(host.data()) + at[r], len[r]));
    return py::make_tuple(runs, ck);
  }, py::arg("nrec"), py::arg("key_lo"), py::arg("key_span"), py::arg("seeds"), py::arg("unsorted") = false,
        py::arg("device") = 0);
  // The constants of the block decode kernels (kernels.h: DecodeGeometry), for tests that place tokens on
  // their boundaries. Plain numbers: callable without a device.
  m.def("gpu_decode_geometry", [] {
    const gpu::DecodeGeometry g = gpu::decode_geometry();
    py::dict d;
    d["reg_window"] = g.reg_window;
    d["reg_align"] = g.reg_align;
    d["lds_window"] = g.lds_window;
    d["lds_align"] = g.lds_align;
    d["short_copy"] = g.short_copy;
    d["vec_bytes"] = g.vec_bytes;
    d["wave_step"] = g.wave_step;
    d["lane_word"] = g.lane_word;
    d["waves_per_block"] = g.waves_per_block;
    d["prefix_slot"] = g.prefix_slot;
    return d;
  });
  // F6: decode Hadoop block-compressed streams on the device; returns (raw streams, blocks, decode_ms).
  // clip > 0: the prefix decode as device_reduce.cc lays it out, block b's first min(clip, raw) bytes at
  // b * clip of a buffer of blocks * clip bytes plus a 256-byte guard, every byte 0xA5 before the launch;
  // returns (the whole buffer, blocks, decode_ms). The full decode's output buffer is filled the same way, so
  // a byte a kernel failed to write never shows what an earlier launch left at that address.
  m.def("gpu_block_decode", [](const std::string& codec_cls, const std::vector<std::string>& streams, int device,
                               int64_t clip) {
    bool unsup = false;
    Codec c = codec_from_class(codec_cls, &unsup);
    if (c == Codec::kNone)
      c = codec_cls == "snappy" ? Codec::kSnappy
          : codec_cls == "lzo"  ? Codec::kLzo
          : codec_cls == "lz4"  ? Codec::kLz4
                                : Codec::kNone;
    if (c == Codec::kNone) throw py::value_error("unknown codec " + codec_cls);
    if (clip < 0) throw py::value_error("clip < 0");
    constexpr int64_t kGuard = 256;
    std::vector<std::string> outs;
    std::string whole;
    int64_t blocks = 0;
    double ms = 0;
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      std::vector<const uint8_t*> ptrs;
      std::vector<int64_t> lens;
      int64_t staged = 0;
      for (auto& st : streams) {
        ptrs.push_back(reinterpret_cast<const uint8_t*>(st.data()));
        lens.push_back((int64_t)st.size());
        staged += (int64_t)st.size();
      }
      gpu::BlockPlan plan;
      if (!gpu::plan_block_streams(c, ptrs, lens, &plan)) throw UdaError("block framing not resolvable on device");
      const int64_t nb = (int64_t)plan.descs.size();
      const int64_t out_bytes = clip > 0 ? nb * clip + kGuard : plan.raw_total;
      gpu::DeviceBuffer din((size_t)std::max<int64_t>(staged, 16)), dout((size_t)std::max<int64_t>(out_bytes, 16));
      hipStream_t s;
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      int64_t off = 0;
      for (auto& st : streams) {
        if (!st.empty()) HIP_CHECK(hipMemcpyAsync(din.as<uint8_t>() + off, st.data(), st.size(), hipMemcpyHostToDevice, s));
        off += (int64_t)st.size();
      }
      if (out_bytes) HIP_CHECK(hipMemsetAsync(dout.as(), 0xA5, (size_t)out_bytes, s));
      HIP_CHECK(hipStreamSynchronize(s));
      if (clip > 0) {
        std::vector<gpu::DecodeDesc> pd(plan.descs);
        for (int64_t b = 0; b < nb; ++b) pd[(size_t)b].dst = b * clip;
        gpu::DeviceBuffer ddesc((size_t)std::max<int64_t>(nb, 1) * sizeof(gpu::DecodeDesc)), dstat(sizeof(int));
        int st = 0;
        const size_t desc_bytes = (size_t)nb * sizeof(gpu::DecodeDesc);
        if (nb) HIP_CHECK(hipMemcpyAsync(ddesc.as(), pd.data(), desc_bytes, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(dstat.as(), 0, sizeof(int), s));
        HIP_CHECK(hipStreamSynchronize(s));
        auto t0 = std::chrono::steady_clock::now();
        gpu::launch_block_decode((int)c, din.as<uint8_t>(), dout.as<uint8_t>(), ddesc.as<gpu::DecodeDesc>(), (int)nb,
                                 dstat.as<int>(), s, clip);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(&st, dstat.as(), sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        whole.assign((size_t)out_bytes, '\0');
        HIP_CHECK(hipMemcpyAsync(&whole[0], dout.as(), whole.size(), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipStreamDestroy(s));
        if (st) throw UdaError(std::string("corrupt ") + codec_name(c) + " block (device prefix decode)");
        blocks = nb;
      } else {
        gpu::DeviceBlockDecoder dec;
        auto t0 = std::chrono::steady_clock::now();
        dec.decode(c, plan, din.as<uint8_t>(), dout.as<uint8_t>(), s);
        ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::string all((size_t)plan.raw_total, '\0');
        if (plan.raw_total) HIP_CHECK(hipMemcpyAsync(&all[0], dout.as(), all.size(), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipStreamDestroy(s));
        for (size_t i = 0; i < streams.size(); ++i)
          outs.push_back(all.substr((size_t)plan.raw_offset[i], (size_t)(plan.raw_offset[i + 1] - plan.raw_offset[i])));
        blocks = (int64_t)plan.descs.size();
      }
    }
    if (clip > 0) return py::make_tuple(py::object(py::bytes(whole)), blocks, ms);
    py::list l;
    for (auto& o : outs) l.append(py::bytes(o));
    return py::make_tuple(py::object(l), blocks, ms);
  }, py::arg("codec"), py::arg("streams"), py::arg("device") = 0, py::arg("clip") = 0);
  // zlib streams inflated on the device in one launch (gpu/stream_decoder.h): (raw streams, bytes each stream
  // took, ms). Output i is raw_lens[i] bytes followed by 256 guard bytes of 0xA5, the whole buffer 0xA5 before
  // the launch; a guard byte that changed is an error here whatever the decode said.
  // container: "zlib" (default) or "gzip", one gzip member per stream.
  m.def("gpu_inflate_streams", [](const std::vector<std::string>& streams, const std::vector<int64_t>& raw_lens, int device,
                                  const std::string& container) {
    if (streams.size() != raw_lens.size()) throw py::value_error("one raw length per stream");
    if (container != "zlib" && container != "gzip") throw py::value_error("container: zlib or gzip");
    const Codec cont = container == "gzip" ? Codec::kGzip : Codec::kZlib;
    constexpr int64_t kGuard = 256;
    std::vector<std::string> outs;
    std::vector<int64_t> consumed;
    double ms = 0;
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      gpu::StreamPlan plan;
      plan.raw_offset.assign(1, 0);
      int64_t staged = 0, out_bytes = 0;
      for (size_t i = 0; i < streams.size(); ++i) {
        if (raw_lens[i] < 0) throw UdaError("raw length < 0");
        plan.descs.push_back(gpu::InflateDesc{staged, (int64_t)streams[i].size(), out_bytes, raw_lens[i]});
        staged += (int64_t)streams[i].size();
        out_bytes += raw_lens[i] + kGuard;
        plan.raw_offset.push_back(out_bytes);
      }
      plan.raw_total = out_bytes;
      gpu::DeviceBuffer din((size_t)std::max<int64_t>(staged, 16)), dout((size_t)std::max<int64_t>(out_bytes, 16));
      hipStream_t s;
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      for (size_t i = 0; i < streams.size(); ++i)
        if (!streams[i].empty())
          HIP_CHECK(hipMemcpyAsync(din.as<uint8_t>() + plan.descs[i].src, streams[i].data(), streams[i].size(),
                                   hipMemcpyHostToDevice, s));
      if (out_bytes) HIP_CHECK(hipMemsetAsync(dout.as(), 0xA5, (size_t)out_bytes, s));
      HIP_CHECK(hipStreamSynchronize(s));
      gpu::DeviceStreamDecoder dec;
      std::string err;
      auto t0 = std::chrono::steady_clock::now();
      try {
        dec.decode(plan, din.as<uint8_t>(), dout.as<uint8_t>(), {}, s, nullptr, nullptr, nullptr, cont);
      } catch (const UdaError& e) {
        err = e.what();
      }
      ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      std::string all((size_t)out_bytes, '\0');
      if (out_bytes) HIP_CHECK(hipMemcpyAsync(&all[0], dout.as(), all.size(), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      HIP_CHECK(hipStreamDestroy(s));
      for (size_t i = 0; i < streams.size(); ++i) {
        const size_t g0 = (size_t)(plan.descs[i].dst + raw_lens[i]);
        for (size_t k = 0; k < (size_t)kGuard; ++k)
          if ((uint8_t)all[g0 + k] != 0xA5)
            throw UdaError("device inflate wrote past the output of stream " + std::to_string(i) + " (guard byte " +
                           std::to_string(k) + ")");
      }
      if (!err.empty()) throw UdaError(err);
      for (size_t i = 0; i < streams.size(); ++i) {
        outs.push_back(all.substr((size_t)plan.descs[i].dst, (size_t)raw_lens[i]));
        consumed.push_back(dec.results()[i].consumed);
      }
    }
    py::list l;
    for (auto& o : outs) l.append(py::bytes(o));
    return py::make_tuple(py::object(l), consumed, ms);
  }, py::arg("streams"), py::arg("raw_lens"), py::arg("device") = 0, py::arg("container") = "zlib");
  // zstd frames decoded on the device in one launch (gpu/zstd.hip), laid out as gpu_inflate_streams lays its
  // streams: 256 guard bytes of 0xA5 behind every output, checked before anything is returned or raised.
  // Returns (outputs, consumed, frames that carried a content checksum, ms, launches of the XXH64 kernel).
  m.def("gpu_zstd_streams", [](const std::vector<std::string>& streams, const std::vector<int64_t>& raw_lens, int device) {
    if (streams.size() != raw_lens.size()) throw py::value_error("one raw length per stream");
    constexpr int64_t kGuard = 256;
    std::vector<std::string> outs;
    std::vector<int64_t> consumed;
    int64_t with_sum = 0, xxh_launches = 0;
    double ms = 0;
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      gpu::StreamPlan plan;
      plan.raw_offset.assign(1, 0);
      int64_t staged = 0, out_bytes = 0;
      for (size_t i = 0; i < streams.size(); ++i) {
        if (raw_lens[i] < 0) throw UdaError("raw length < 0");
        plan.descs.push_back(gpu::InflateDesc{staged, (int64_t)streams[i].size(), out_bytes, raw_lens[i]});
        staged += (int64_t)streams[i].size();
        out_bytes += raw_lens[i] + kGuard;
        plan.raw_offset.push_back(out_bytes);
      }
      plan.raw_total = out_bytes;
      gpu::DeviceBuffer din((size_t)std::max<int64_t>(staged, 16)), dout((size_t)std::max<int64_t>(out_bytes, 16));
      hipStream_t s;
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      for (size_t i = 0; i < streams.size(); ++i)
        if (!streams[i].empty())
          HIP_CHECK(hipMemcpyAsync(din.as<uint8_t>() + plan.descs[i].src, streams[i].data(), streams[i].size(),
                                   hipMemcpyHostToDevice, s));
      if (out_bytes) HIP_CHECK(hipMemsetAsync(dout.as(), 0xA5, (size_t)out_bytes, s));
      HIP_CHECK(hipStreamSynchronize(s));
      gpu::DeviceStreamDecoder dec;
      std::string err;
      auto t0 = std::chrono::steady_clock::now();
      try {
        dec.decode(plan, din.as<uint8_t>(), dout.as<uint8_t>(), {}, s, nullptr, nullptr, nullptr, Codec::kZstd);
      } catch (const UdaError& e) {
        err = e.what();
      }
      ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      std::string all((size_t)out_bytes, '\0');
      if (out_bytes) HIP_CHECK(hipMemcpyAsync(&all[0], dout.as(), all.size(), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      HIP_CHECK(hipStreamDestroy(s));
      for (size_t i = 0; i < streams.size(); ++i) {
        const size_t g0 = (size_t)(plan.descs[i].dst + raw_lens[i]);
        for (size_t k = 0; k < (size_t)kGuard; ++k)
          if ((uint8_t)all[g0 + k] != 0xA5)
            throw UdaError("device zstd decode wrote past the output of stream " + std::to_string(i) + " (guard byte " +
                           std::to_string(k) + ")");
      }
      if (!err.empty()) throw UdaError(err);
      for (size_t i = 0; i < streams.size(); ++i) {
        outs.push_back(all.substr((size_t)plan.descs[i].dst, (size_t)raw_lens[i]));
        consumed.push_back(dec.zstd_results()[i].consumed);
        with_sum += dec.zstd_results()[i].has_checksum ? 1 : 0;
      }
      xxh_launches = dec.xxh64_launches();
    }
    py::list l;
    for (auto& o : outs) l.append(py::bytes(o));
    return py::make_tuple(py::object(l), consumed, with_sum, ms, xxh_launches);
  }, py::arg("streams"), py::arg("raw_lens"), py::arg("device") = 0);
  m.def("gpu_zstd_geometry", [] {
    const gpu::ZstdGeometry g = gpu::zstd_geometry();
    py::dict d;
    d["waves_per_block"] = g.waves_per_block;
    d["lds_per_wave"] = g.lds_per_wave;
    d["literal_scratch"] = g.literal_scratch;
    return d;
  });
  // XXH64 (seed 0) of every buffer in one launch (gpu/xxh64.hip).
  m.def("gpu_xxh64", [](const std::vector<std::string>& buffers, int device) {
    std::vector<uint64_t> out(buffers.size());
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      const int n = (int)buffers.size();
      if (n == 0) return out;
      std::vector<int64_t> offs, lens;
      int64_t total = 16;
      for (auto& b : buffers) {
        offs.push_back(total);
        lens.push_back((int64_t)b.size());
        total += (int64_t)b.size();
      }
      gpu::DeviceBuffer data((size_t)total), meta((size_t)n * 24);
      std::vector<const uint8_t*> ptrs;
      for (int i = 0; i < n; ++i) ptrs.push_back(data.as<uint8_t>() + offs[(size_t)i]);
      hipStream_t s;
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      for (int i = 0; i < n; ++i)
        if (!buffers[(size_t)i].empty())
          HIP_CHECK(hipMemcpyAsync(data.as<uint8_t>() + offs[(size_t)i], buffers[(size_t)i].data(), buffers[(size_t)i].size(),
                                   hipMemcpyHostToDevice, s));
      uint8_t* const mb = meta.as<uint8_t>();
      HIP_CHECK(hipMemcpyAsync(mb, ptrs.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(mb + (size_t)n * 8, lens.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
      gpu::launch_xxh64(reinterpret_cast<const uint8_t* const*>(mb), reinterpret_cast<const int64_t*>(mb + (size_t)n * 8), n,
                        reinterpret_cast<uint64_t*>(mb + (size_t)n * 16), s);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(out.data(), mb + (size_t)n * 16, (size_t)n * 8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      HIP_CHECK(hipStreamDestroy(s));
    }
    return out;
  }, py::arg("buffers"), py::arg("device") = 0);
  // zlib.adler32 of every item in one batched launch (gpu/adler32.hip); item i starts `misalign` bytes past a
  // 16-byte boundary of the device buffer.
  // timed: returns (values, ms of the launch alone, from its queueing to its result) instead.
  m.def("gpu_adler32", [](const std::vector<std::string>& items, int misalign, int device, bool timed) -> py::object {
    if (misalign < 0 || misalign > 15) throw py::value_error("misalign 0..15");
    std::vector<uint32_t> out(items.size());
    double ms = 0;
    {
      py::gil_scoped_release rel;
      HIP_CHECK(hipSetDevice(device));
      const int n = (int)items.size();
      std::vector<int64_t> offs, lens;
      int64_t total = 16;
      for (auto& it : items) {
        offs.push_back(total + misalign);
        lens.push_back((int64_t)it.size());
        total = (total + misalign + (int64_t)it.size() + 15) / 16 * 16;
      }
      gpu::DeviceBuffer data((size_t)total + 16), meta((size_t)std::max(n, 1) * 48);
      std::vector<const uint8_t*> ptrs;
      for (auto o : offs) ptrs.push_back(data.as<uint8_t>() + o);
      hipStream_t s;
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      for (int i = 0; i < n; ++i)
        if (!items[(size_t)i].empty())
          HIP_CHECK(hipMemcpyAsync(data.as<uint8_t>() + offs[(size_t)i], items[(size_t)i].data(), items[(size_t)i].size(),
                                   hipMemcpyHostToDevice, s));
      uint8_t* mb = meta.as<uint8_t>();
      if (n) {
        HIP_CHECK(hipMemcpyAsync(mb, ptrs.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(mb + (size_t)n * 8, lens.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));
        const auto t0 = std::chrono::steady_clock::now();
        gpu::launch_adler32(reinterpret_cast<const uint8_t* const*>(mb), reinterpret_cast<const int64_t*>(mb + (size_t)n * 8), n,
                            reinterpret_cast<uint32_t*>(mb + (size_t)n * 16), reinterpret_cast<uint64_t*>(mb + (size_t)n * 32), s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(out.data(), mb + (size_t)n * 16, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      }
      HIP_CHECK(hipStreamSynchronize(s));
      HIP_CHECK(hipStreamDestroy(s));
    }
    if (timed) return py::make_tuple(out, ms);
    return py::cast(out);
  }, py::arg("items"), py::arg("misalign") = 0, py::arg("device") = 0, py::arg("timed") = false);
  // The inflate kernel's constants (needs no GPU), for tests that lay codes on its boundaries.
  m.def("gpu_inflate_geometry", []() {
    const gpu::InflateGeometry g = gpu::inflate_geometry();
    py::dict d;
    d["window"] = g.window;
    d["window_align"] = g.window_align;
    d["literal_stage"] = g.literal_stage;
    d["waves_per_block"] = g.waves_per_block;
    d["lds_per_wave"] = g.lds_per_wave;
    return d;
  });
  m.def("nccl_unique_id", []() { return py::bytes(gpu::nccl_unique_id()); });
  // RCCL data-plane self test on one GPU: communicator bootstrap from an ncclUniqueId and the grouped
  // send/recv counts exchange the shuffle plan uses (world 1: the rank exchanges with itself).
  m.def("rccl_selftest", [](int device, int n) {
    py::gil_scoped_release rel;
    HIP_CHECK(hipSetDevice(device));
    auto ex = gpu::make_rccl_exchange(0, 1, gpu::nccl_unique_id());
    hipStream_t s;
    HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    std::vector<int64_t> send((size_t)n), recv((size_t)n, -1);
    for (int i = 0; i < n; ++i) send[(size_t)i] = (int64_t)i * 1000003 - 7;
    ex->alltoall_i64(send.data(), recv.data(), (size_t)n, s);
    HIP_CHECK(hipStreamDestroy(s));
    return std::string(ex->name()) + (send == recv ? ":ok" : ":mismatch");
  }, py::arg("device") = 0, py::arg("n") = 4096);

  // Exchange backends with hand-made plans (tests): the local group runs its ranks as threads here;
  // the IPC probe is one rank (call it from one process per rank).
  m.def("local_exchange_probe",
        [](int world, const std::vector<std::vector<std::vector<int64_t>>>& send,
           const std::vector<std::vector<std::vector<int64_t>>>& recv, bool host_source, int rounds, int device) {
          py::gil_scoped_release rel;
          static std::atomic<int> gen{0};
          const std::string name = "probe" + std::to_string(gen++);
          std::vector<std::string> out(world);
          std::vector<std::thread> ts;
          for (int r = 0; r < world; ++r)
            ts.emplace_back([&, r] {
              try {
                HIP_CHECK(hipSetDevice(device));
                auto ex = gpu::make_local_exchange(name, r, world);
                out[r] = gpu::exchange_probe(*ex, device, send.at(r), recv.at(r), host_source, rounds);
              } catch (const std::exception& e) {
                out[r] = e.what();
              }
            });
          for (auto& t : ts) t.join();
          return out;
        },
        py::arg("world"), py::arg("send"), py::arg("recv"), py::arg("host_source") = false, py::arg("rounds") = 1,
        py::arg("device") = 0);
  m.def("ipc_exchange_probe",
        [](const std::string& name, int rank, int world, const std::vector<std::vector<int64_t>>& send,
           const std::vector<std::vector<int64_t>>& recv, bool host_source, int rounds, int device,
           int64_t export_bytes) {
          py::gil_scoped_release rel;
          try {
            HIP_CHECK(hipSetDevice(device));
            auto ex = gpu::make_ipc_exchange(name, rank, world, device);
            return gpu::exchange_probe(*ex, device, send, recv, host_source, rounds, export_bytes);
          } catch (const std::exception& e) {
            return std::string(e.what());
          }
        },
        py::arg("name"), py::arg("rank"), py::arg("world"), py::arg("send"), py::arg("recv"),
        py::arg("host_source") = false, py::arg("rounds") = 1, py::arg("device") = 0, py::arg("export_bytes") = 0);

  py::class_<gpu::J2CSink, std::shared_ptr<gpu::J2CSink>>(m, "J2CSink")
      .def(py::init([](int r, int64_t kv, py::object threaded) {
             return std::make_shared<gpu::J2CSink>(r, kv, threaded.is_none() ? gpu::J2CSink::default_threaded()
                                                                               : threaded.cast<bool>());
           }),
           py::arg("reducers"), py::arg("kv_buf_bytes") = 1 << 20, py::arg("threaded") = py::none())
      .def_property_readonly("reducers", &gpu::J2CSink::reducers)
      .def_property_readonly("threaded", &gpu::J2CSink::threaded)
      .def("flush", &gpu::J2CSink::flush, py::call_guard<py::gil_scoped_release>())
      .def("records", &gpu::J2CSink::records)
      .def("bytes", &gpu::J2CSink::bytes)
      .def("buffers", &gpu::J2CSink::buffers)
      .def("eof", &gpu::J2CSink::eof)
      .def("error", &gpu::J2CSink::error)
      .def("order_errors", &gpu::J2CSink::order_errors)
      .def("set_check_order", &gpu::J2CSink::set_check_order)
      .def("reset", &gpu::J2CSink::reset, py::call_guard<py::gil_scoped_release>())
      // one dataFromUda buffer for reducer r (returns the sink's status code, 0 = ok); reps > 1
      // consumes the same buffer again (micro-benchmarks; EOF buffers only once)
      .def("consume", [](gpu::J2CSink& s, int r, py::buffer b, int reps) {
        py::buffer_info bi = b.request();
        const auto* p = static_cast<const uint8_t*>(bi.ptr);
        const int64_t n = (int64_t)(bi.size * bi.itemsize);
        if (r < 0 || r >= s.reducers()) throw py::index_error("reducer out of range");
        py::gil_scoped_release rel;
        int rc = 0;
        for (int i = 0; i < std::max(1, reps) && rc == 0; ++i) rc = s.consume(r, p, n);
        return rc;
      }, py::arg("reducer"), py::arg("data"), py::arg("reps") = 1);

  // fixed windows of every reducer's delivered stream, kept beside the J2C sink (set_j2c_sink)
  py::class_<gpu::StreamSampler, std::shared_ptr<gpu::StreamSampler>>(m, "StreamSampler")
      .def(py::init<std::vector<std::vector<int64_t>>, int64_t>(), py::arg("starts"), py::arg("window"))
      .def_property_readonly("reducers", &gpu::StreamSampler::reducers)
      .def_property_readonly("window", &gpu::StreamSampler::window)
      .def("reset", &gpu::StreamSampler::reset)
      .def("observe", [](gpu::StreamSampler& s, int r, py::buffer b) {
        py::buffer_info bi = b.request();
        if (r < 0 || r >= s.reducers()) throw py::index_error("reducer out of range");
        s.observe(r, static_cast<const uint8_t*>(bi.ptr), (int64_t)(bi.size * bi.itemsize));
      }, py::arg("reducer"), py::arg("data"))
      .def("stream_bytes", &gpu::StreamSampler::stream_bytes)
      .def("captured_bytes", &gpu::StreamSampler::captured_bytes)
      // reducer r's windows as a (windows, window) uint8 array (a copy)
      .def("data", [](gpu::StreamSampler& s, int r) {
        if (r < 0 || r >= s.reducers()) throw py::index_error("reducer out of range");
        py::array_t<uint8_t> a({(py::ssize_t)s.windows(r), (py::ssize_t)s.window()});
        const auto& d = s.data(r);
        if (!d.empty()) std::memcpy(a.mutable_data(), d.data(), d.size());
        return a;
      });

  py::class_<gpu::ApiTeraSortBench>(m, "ApiTeraSortBench")
      .def(py::init([](const py::dict& d) {
        gpu::ApiBenchConfig c;
        auto get = [&](const char* k, auto& field) {
          if (d.contains(k)) field = d[k].cast<std::decay_t<decltype(field)>>();
        };
        get("device", c.device);
        get("maps", c.maps);
        get("reducers", c.reducers);
        get("records_per_map", c.records_per_map);
        get("seed", c.seed);
        get("kv_buf_bytes", c.kv_buf_bytes);
        get("round_bytes", c.round_bytes);
        get("rank", c.rank);
        get("world", c.world);
        get("port", c.port);
        get("transport", c.transport);
        get("bind_addr", c.bind_addr);
        get("host_mofs", c.host_mofs);
        get("fetch", c.fetch);
        get("max_concurrent_merges", c.max_concurrent_merges);
        get("provider_workers", c.provider_workers);
        get("mof_dir", c.mof_dir);
        get("provider_hbm_bytes", c.provider_hbm_bytes);
        get("workload", c.workload);
        get("skew", c.skew);
        get("codec", c.codec);
        return new gpu::ApiTeraSortBench(c);
      }))
      .def("setup", &gpu::ApiTeraSortBench::setup, py::call_guard<py::gil_scoped_release>())
      .def("step",
           [](gpu::ApiTeraSortBench& b, bool validate) {
             std::string info;
             std::map<std::string, double> r;
             {
               py::gil_scoped_release g;
               r = b.step(validate, &info);
             }
             py::dict d;
             for (auto& kv : r) d[kv.first.c_str()] = kv.second;
             d["task0_stats"] = info;
             return d;
           },
           py::arg("validate") = false)
      .def("expected_records", &gpu::ApiTeraSortBench::expected_records)
      .def("provider_stats", &gpu::ApiTeraSortBench::provider_stats)
      .def_property_readonly("compressed_bytes", &gpu::ApiTeraSortBench::compressed_bytes)
      .def("local_partition_records", &gpu::ApiTeraSortBench::local_partition_records)
      .def("set_expected", &gpu::ApiTeraSortBench::set_expected)
      .def("set_peers", &gpu::ApiTeraSortBench::set_peers)
      .def("task_commands", &gpu::ApiTeraSortBench::task_commands)
      .def("provider_port", &gpu::ApiTeraSortBench::provider_port)
      .def_property_readonly("store_bytes", &gpu::ApiTeraSortBench::store_bytes);

  py::class_<gpu::ShuffleJob>(m, "ShuffleJob")
      .def(py::init([](const py::dict& cfg) { return new gpu::ShuffleJob(config_from_dict(cfg)); }))
      // std::string, not py::bytes: the argument is converted while the GIL is held (a py::bytes would
      // be read and released inside the GIL-free call)
      .def("init_comm", [](gpu::ShuffleJob& j, const std::string& uid) { j.init_comm(uid); },
           py::call_guard<py::gil_scoped_release>())
      .def("init_local", &gpu::ShuffleJob::init_local, py::call_guard<py::gil_scoped_release>())
      .def("init_ipc", &gpu::ShuffleJob::init_ipc, py::call_guard<py::gil_scoped_release>())
      .def("generate", &gpu::ShuffleJob::generate, py::call_guard<py::gil_scoped_release>())
      .def("sample_keys",
           [](gpu::ShuffleJob& j, int64_t every) {
             auto v = j.sample_keys(every);
             py::list out;
             for (auto& d : v) {
               py::array_t<uint64_t> a({(py::ssize_t)(d.size() / 2), (py::ssize_t)2});
               if (!d.empty()) std::memcpy(a.mutable_data(), d.data(), d.size() * 8);
               out.append(a);
             }
             return out;
           })
      .def("set_bounds",
           [](gpu::ShuffleJob& j, py::array_t<uint64_t, py::array::c_style> b) {
             std::vector<uint64_t> v(b.data(), b.data() + b.size());
             j.set_bounds(v);
           })
      .def("plan", &gpu::ShuffleJob::plan, py::call_guard<py::gil_scoped_release>())
      .def("set_j2c_sink",
           [](gpu::ShuffleJob& j, std::shared_ptr<gpu::J2CSink> s, std::shared_ptr<gpu::StreamSampler> sampler) {
             if (s->reducers() != j.config().reducers) throw py::value_error("J2CSink reducer count mismatch");
             if (!sampler) {
               j.set_sink([s](int r, const uint8_t* buf, int64_t len) { return s->consume(r, buf, len); });
               return;
             }
             if (sampler->reducers() != s->reducers()) throw py::value_error("StreamSampler reducer count mismatch");
             j.set_sink([s, sampler](int r, const uint8_t* buf, int64_t len) {
               sampler->observe(r, buf, len);
               return s->consume(r, buf, len);
             });
           },
           py::arg("sink"), py::arg("sampler") = std::shared_ptr<gpu::StreamSampler>())
      .def("set_python_sink",
           [](gpu::ShuffleJob& j, py::function fn, bool with_reducer) {
             auto holder = std::make_shared<py::function>(fn);
             j.set_sink([holder, with_reducer](int r, const uint8_t* buf, int64_t len) {
               py::gil_scoped_acquire g;
               try {
                 py::bytes b(reinterpret_cast<const char*>(buf), (size_t)len);
                 py::object res = with_reducer ? (*holder)(r, b) : (*holder)(b);
                 return res.is_none() ? 0 : res.cast<int>();
               } catch (py::error_already_set& e) {
                 e.discard_as_unraisable("ShuffleJob python sink");
                 return -1;
               }
             });
           },
           py::arg("fn"), py::arg("with_reducer") = false)
      .def("clear_sink", [](gpu::ShuffleJob& j) { j.set_sink(nullptr); })
      .def("run_step",
           [](gpu::ShuffleJob& j, bool validate) {
             gpu::StepStats st;
             {
               py::gil_scoped_release r;
               st = j.run_step(validate);
             }
             return stats_to_dict(st);
           },
           py::arg("validate") = false)
      .def("reducer_records", &gpu::ShuffleJob::reducer_records)
      .def_property_readonly("comm_ranks", &gpu::ShuffleJob::comm_ranks)
      .def_property_readonly("exchange_name", &gpu::ShuffleJob::exchange_name)
      .def_property_readonly("delivery_name", &gpu::ShuffleJob::delivery_name)
      .def_property_readonly("store_name", &gpu::ShuffleJob::store_name)
      .def("local_dest_checksums", &gpu::ShuffleJob::local_dest_checksums)
      .def("local_dest_records", &gpu::ShuffleJob::local_dest_records)
      .def("index_record", &gpu::ShuffleJob::index_record)
      .def("read_partition",
           [](gpu::ShuffleJob& j, int mp, int d) {
             auto v = j.read_partition(mp, d);
             return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
           })
      .def("mof_device_ptr", [](gpu::ShuffleJob& j, int m) { return (uintptr_t)j.mof_device_ptr(m); })
      .def("mof_bytes", &gpu::ShuffleJob::mof_bytes)
      .def_property_readonly("store_bytes", &gpu::ShuffleJob::store_bytes)
      .def_property_readonly("map_sort_ms", &gpu::ShuffleJob::map_sort_ms)
      .def_property_readonly("max_round_records", &gpu::ShuffleJob::max_round_records)
      .def("peer_send_bytes", &gpu::ShuffleJob::peer_send_bytes);
}
