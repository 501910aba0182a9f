#include "rpq_plan.h"

#include <algorithm>

#include "uda/error.h"

namespace uda {

std::string key_at(const uint8_t* p, int64_t avail) {
  RecordView rv;
  if (ifile_parse(p, (size_t)avail, &rv) != Parse::kRecord) throw UdaError("spill index: bad record boundary");
  return std::string(reinterpret_cast<const char*>(rv.key), (size_t)rv.klen);
}

int cmp_key(KeyKind kind, const std::string& a, const std::string& b) {
  return key_compare(kind, reinterpret_cast<const uint8_t*>(a.data()), (int)a.size(),
                     reinterpret_cast<const uint8_t*>(b.data()), (int)b.size());
}

void RunCursor::advance(const uint8_t* p, int64_t limit, int64_t spacing, std::vector<int64_t>* cut,
                        std::vector<std::string>* key) {
  while (!eof && pos < limit) {
    // between cuts: skip records with one-byte VInt headers (lengths < 128) without parsing them
    while (pos < next_cut && pos + 2 <= limit) {
      const int8_t k1 = (int8_t)p[pos], v1 = (int8_t)p[pos + 1];
      if ((k1 | v1) < 0) break;  // multi-byte header or the EOF marker: the parser below
      const int64_t nx = pos + 2 + k1 + v1;
      if (nx > limit) break;  // cut by the limit: the parser below reports it
      last = pos;
      pos = nx;
    }
    if (pos >= limit) break;
    RecordView rv;
    const Parse ps = ifile_parse(p + pos, (size_t)(limit - pos), &rv);
    if (ps == Parse::kEof) {
      eof = true;
      break;
    }
    if (ps == Parse::kPartial) break;  // the rest of it lands with a later phase
    if (ps != Parse::kRecord) throw UdaError("hybrid index: bad record in a fetched partition");
    if (pos >= next_cut) {
      cut->push_back(pos);
      key->emplace_back(reinterpret_cast<const char*>(rv.key), (size_t)rv.klen);
      next_cut = pos + spacing;
    }
    last = pos;
    pos += rv.size();
  }
}

std::string RunCursor::last_key(const uint8_t* p) const {
  RecordView rv;
  if (last < 0 || ifile_parse(p + last, (size_t)(pos - last), &rv) != Parse::kRecord) return std::string();
  return std::string(reinterpret_cast<const char*>(rv.key), (size_t)rv.klen);
}

SpillRun index_host_run(uint8_t* p, int64_t len, int64_t spacing) {
  SpillRun run;
  run.mem = p;
  RunCursor c;
  c.advance(p, len, spacing, &run.cut, &run.key);
  // a whole partition: a record that its end cuts is a bad record, not one still to land
  if (!c.eof && c.pos < len) throw UdaError("hybrid index: bad record in a fetched partition");
  run.bytes = c.pos;
  return run;
}

int64_t boundary(const SpillRun& run, const std::string& key, KeyKind kind, const ReadWindow& read_window) {
  // last cut with key < `key` (cut keys ascend within a run)
  int lo = -1, hi = (int)run.cut.size();
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (cmp_key(kind, run.key[(size_t)mid], key) < 0)
      lo = mid;
    else
      hi = mid;
  }
  if (lo < 0) return 0;
  const int64_t b = run.cut[(size_t)lo];
  const int64_t e = (size_t)lo + 1 < run.cut.size() ? run.cut[(size_t)lo + 1] : run.bytes;
  std::vector<uint8_t> win;
  const uint8_t* w = run.mem ? run.mem + b : nullptr;  // DRAM runs are scanned in place
  if (!w) {
    if (!read_window) throw UdaError("spill scan: the run is not in memory");
    win.resize((size_t)(e - b));
    read_window(run, b, e - b, win.data());
    w = win.data();
  }
  int64_t p = 0;
  while (b + p < e) {
    RecordView rv;
    if (ifile_parse(w + p, (size_t)(e - b - p), &rv) != Parse::kRecord) throw UdaError("spill scan: bad record");
    if (key_compare(kind, rv.key, rv.klen, reinterpret_cast<const uint8_t*>(key.data()), (int)key.size()) >= 0) break;
    p += rv.size();
  }
  return b + p;
}

std::vector<std::string> plan_splitters(const std::vector<SpillRun>& runs, const std::vector<int64_t>& at,
                                        const std::vector<int64_t>& end, int64_t target, KeyKind kind) {
  struct Sample {
    int run;
    int idx;
  };
  std::vector<Sample> samples;
  for (int k = 0; k < (int)runs.size(); ++k) {
    const SpillRun& r = runs[(size_t)k];
    for (int j = 0; j < (int)r.cut.size(); ++j)
      if (r.cut[(size_t)j] >= at[(size_t)k] && r.cut[(size_t)j] < end[(size_t)k]) samples.push_back({k, j});
  }
  std::stable_sort(samples.begin(), samples.end(), [&](const Sample& a, const Sample& b) {
    const int c = cmp_key(kind, runs[(size_t)a.run].key[(size_t)a.idx], runs[(size_t)b.run].key[(size_t)b.idx]);
    return c != 0 ? c < 0 : (a.run != b.run ? a.run < b.run : a.idx < b.idx);
  });
  std::vector<std::string> split;
  int64_t acc = 0;
  for (const Sample& sm : samples) {
    const SpillRun& r = runs[(size_t)sm.run];
    const int64_t next = std::min(end[(size_t)sm.run], (size_t)sm.idx + 1 < r.cut.size() ? r.cut[(size_t)sm.idx + 1] : r.bytes);
    if (acc >= target) {
      const std::string& k = r.key[(size_t)sm.idx];
      if (split.empty() || cmp_key(kind, split.back(), k) < 0) {
        split.push_back(k);
        acc = 0;
      }
    }
    acc += next - r.cut[(size_t)sm.idx];
  }
  return split;
}

std::vector<RoundSlices> slice_rounds(const std::vector<std::vector<int64_t>>& bnd, const std::vector<int64_t>& at,
                                      const std::vector<int64_t>& end, bool drop_empty, bool keep_last) {
  const size_t K = bnd.size();
  const size_t nr = K ? bnd[0].size() + 1 : 0;
  std::vector<std::vector<int64_t>> b(K);
  for (size_t k = 0; k < K; ++k) {
    b[k].push_back(at[k]);
    for (int64_t x : bnd[k]) b[k].push_back(std::min(end[k], std::max(b[k].back(), x)));
    b[k].push_back(end[k]);
  }
  std::vector<RoundSlices> rounds;
  for (size_t q = 0; q < nr; ++q) {
    RoundSlices rr(K);
    int64_t bytes = 0;
    for (size_t k = 0; k < K; ++k) {
      rr[k] = {b[k][q], b[k][q + 1]};
      bytes += rr[k].second - rr[k].first;
    }
    if (!drop_empty || bytes > 0 || (keep_last && q + 1 == nr)) rounds.push_back(std::move(rr));
  }
  return rounds;
}

}  // namespace uda
