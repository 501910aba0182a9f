// Stand-alone self-test of the host-only RPQ planner (csrc/consumer/rpq_plan.cc), built with ASan + UBSan
// by tests/test_rpq_plan_cpu.py. IFile runs are built in memory from a fixed-seed generator and the
// planner is checked against a brute-force oracle: parse every record, std::stable_sort by key_compare
// with the run index as tie-break. Every run handed to the planner is an exact-size heap copy, so a read
// past a run's end (or past the landed prefix of a partition) is an ASan error.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "rpq_plan.h"
#include "uda/error.h"
#include "uda/ifile.h"

using namespace uda;

static long checks = 0, failures = 0;
#define EXPECT(c)                                               \
  do {                                                          \
    ++checks;                                                   \
    if (!(c)) {                                                 \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      ++failures;                                               \
    }                                                           \
  } while (0)

struct Rec {
  std::string key, val;
};

static std::string make_key(KeyKind kind, const std::string& content) {
  if (kind == KeyKind::kText) {
    uint8_t b[9];
    const int n = vint_encode((int64_t)content.size(), b);
    return std::string(reinterpret_cast<char*>(b), (size_t)n) + content;
  }
  std::string s(4, '\0');  // BytesWritable: 4-byte big-endian length
  for (int i = 0; i < 4; ++i) s[(size_t)i] = (char)(uint8_t)(content.size() >> (8 * (3 - i)));
  return s + content;
}

static int cmp(KeyKind kind, const std::string& a, const std::string& b) { return cmp_key(kind, a, b); }

// A run: its records (sorted), the IFile bytes with the EOF marker, the offset of every record.
struct Run {
  std::vector<Rec> recs;
  std::vector<uint8_t> bytes;  // records + EOF marker
  std::vector<int64_t> off;    // off[i]: start of record i; off.back(): end of the records
  std::unique_ptr<uint8_t[]> heap;  // exact-size copy of `bytes` (what the planner reads)
  int64_t len() const { return (int64_t)bytes.size(); }
  int64_t body() const { return off.back(); }
};

static void seal(Run* r, KeyKind kind, bool eof = true) {
  std::stable_sort(r->recs.begin(), r->recs.end(), [&](const Rec& a, const Rec& b) { return cmp(kind, a.key, b.key) < 0; });
  r->bytes.clear();
  r->off.clear();
  for (const Rec& x : r->recs) {
    r->off.push_back((int64_t)r->bytes.size());
    ifile_append(&r->bytes, reinterpret_cast<const uint8_t*>(x.key.data()), (int32_t)x.key.size(),
                 reinterpret_cast<const uint8_t*>(x.val.data()), (int32_t)x.val.size());
  }
  r->off.push_back((int64_t)r->bytes.size());
  if (eof) ifile_append_eof(&r->bytes);
  r->heap.reset(new uint8_t[r->bytes.size() ? r->bytes.size() : 1]);
  if (!r->bytes.empty()) std::memcpy(r->heap.get(), r->bytes.data(), r->bytes.size());
}

// `n` records over `distinct` key contents; about one key and one value in eight is >= 128 bytes long
// (multi-byte VInt headers, which break out of the walker's one-byte fast skip)
static Run make_run(std::mt19937& g, KeyKind kind, int n, int distinct, int salt) {
  Run r;
  for (int i = 0; i < n; ++i) {
    const int id = (int)(g() % (unsigned)distinct);
    std::string content = "k" + std::to_string(1000 + id * 7);
    if (id % 8 == 3) content += std::string(130 + (size_t)(id % 5), 'x');
    std::string val((g() % 8 == 0) ? 128 + g() % 90 : g() % 40, (char)('a' + salt));
    val += std::to_string(i);  // distinguishes equal keys: a wrong tie order shows in the bytes
    r.recs.push_back({make_key(kind, content), val});
  }
  seal(&r, kind);
  return r;
}

static std::string raw_of(const Rec& x) {
  std::vector<uint8_t> b;
  ifile_append(&b, reinterpret_cast<const uint8_t*>(x.key.data()), (int32_t)x.key.size(),
               reinterpret_cast<const uint8_t*>(x.val.data()), (int32_t)x.val.size());
  return std::string(b.begin(), b.end());
}

// the oracle: every record of every run, stable-sorted by key (runs in order, so ties keep run order)
static std::string oracle_merge(const std::vector<Run>& runs, KeyKind kind) {
  std::vector<const Rec*> all;
  for (const Run& r : runs)
    for (const Rec& x : r.recs) all.push_back(&x);
  std::stable_sort(all.begin(), all.end(), [&](const Rec* a, const Rec* b) { return cmp(kind, a->key, b->key) < 0; });
  std::string out;
  for (const Rec* x : all) out += raw_of(*x);
  return out;
}

// records of [b, e) of a run; *ok false unless both ends are record boundaries
static std::vector<Rec> slice_records(const Run& r, int64_t b, int64_t e, bool* ok) {
  std::vector<Rec> out;
  const auto ib = std::lower_bound(r.off.begin(), r.off.end(), b), ie = std::lower_bound(r.off.begin(), r.off.end(), e);
  if (ib == r.off.end() || *ib != b || ie == r.off.end() || *ie != e || b > e) {
    *ok = false;
    return out;
  }
  for (auto it = ib; it != ie; ++it) out.push_back(r.recs[(size_t)(it - r.off.begin())]);
  return out;
}

// stable merge of one round's slices, appended to *out; *seen: its records (for the bound check)
static bool merge_round(const std::vector<Run>& runs, const RoundSlices& rr, KeyKind kind, std::string* out,
                        std::vector<Rec>* seen = nullptr) {
  bool ok = rr.size() == runs.size();
  std::vector<Rec> all;
  for (size_t k = 0; ok && k < runs.size(); ++k)
    for (Rec& x : slice_records(runs[k], rr[k].first, rr[k].second, &ok)) all.push_back(std::move(x));
  std::stable_sort(all.begin(), all.end(), [&](const Rec& a, const Rec& b) { return cmp(kind, a.key, b.key) < 0; });
  for (const Rec& x : all) *out += raw_of(x);
  if (seen) *seen = all;
  return ok;
}

static int64_t oracle_boundary(const Run& r, const std::string& key, KeyKind kind) {
  for (size_t i = 0; i < r.recs.size(); ++i)
    if (cmp(kind, r.recs[i].key, key) >= 0) return r.off[i];
  return r.body();
}

// ------------------------------------------------------------------------------ walker equivalence
static void check_walker(const Run& r, int64_t spacing) {
  const SpillRun whole = index_host_run(r.heap.get(), r.len(), spacing);
  EXPECT(whole.bytes == r.body());
  EXPECT(whole.cut.size() == whole.key.size());
  RunCursor c;
  std::vector<int64_t> cut;
  std::vector<std::string> key;
  for (int64_t limit = 1; limit <= r.len(); ++limit) {
    std::unique_ptr<uint8_t[]> prefix(new uint8_t[(size_t)limit]);  // exactly the landed bytes
    std::memcpy(prefix.get(), r.bytes.data(), (size_t)limit);
    c.advance(prefix.get(), limit, spacing, &cut, &key);
    // the last complete record inside the limit, and its key
    const size_t done = (size_t)(std::upper_bound(r.off.begin(), r.off.end(), limit) - r.off.begin()) - 1;
    const bool ok = c.pos == r.off[done] && c.last_key(prefix.get()) == (done ? r.recs[done - 1].key : std::string()) &&
                    c.eof == (limit == r.len() && r.len() > r.body());
    if (!ok) {
      EXPECT(ok);
      return;
    }
  }
  EXPECT(true);
  EXPECT(cut == whole.cut);
  EXPECT(key == whole.key);
  EXPECT(c.pos == whole.bytes);
  for (size_t j = 0; j < whole.cut.size(); ++j) {
    const auto it = std::lower_bound(r.off.begin(), r.off.end(), whole.cut[j]);
    const bool at_record = it != r.off.end() && *it == whole.cut[j] && whole.cut[j] < r.body();
    EXPECT(at_record && whole.key[j] == r.recs[(size_t)(it - r.off.begin())].key);
    if (j) EXPECT(whole.cut[j] >= whole.cut[j - 1] + spacing);
  }
  EXPECT(whole.cut.empty() == r.recs.empty());
  if (!whole.cut.empty()) EXPECT(whole.cut[0] == 0);
}

static void test_walker(KeyKind kind) {
  std::mt19937 g(11);
  Run mixed = make_run(g, kind, 40, 16, 0);
  for (int64_t spacing : {int64_t(1), int64_t(64), int64_t(300), mixed.len() + 100}) check_walker(mixed, spacing);
  Run none;  // EOF marker only
  seal(&none, kind);
  check_walker(none, 64);
  Run zero;  // zero bytes
  seal(&zero, kind, false);
  check_walker(zero, 64);
  Run one = make_run(g, kind, 1, 1, 1);
  check_walker(one, 1);
  check_walker(one, 1 << 20);
  Run no_eof = make_run(g, kind, 12, 4, 2);  // a stream that ends with its last record
  seal(&no_eof, kind, false);
  check_walker(no_eof, 50);
  // a partition whose end cuts a record is a bad partition for the whole-run walk
  bool threw = false;
  try {
    (void)index_host_run(mixed.heap.get(), mixed.body() - 1, 64);
  } catch (const UdaError& e) {
    threw = std::string(e.what()) == "hybrid index: bad record in a fetched partition";
  }
  EXPECT(threw);
}

// ----------------------------------------------------------------------------------------- boundary
static std::vector<std::string> probe_keys(const std::vector<Run>& runs, KeyKind kind) {
  std::vector<std::string> keys{make_key(kind, ""), make_key(kind, std::string(200, '\xff'))};  // below all, above all
  for (const Run& r : runs)
    for (const Rec& x : r.recs) keys.push_back(x.key);
  return keys;
}

static void test_boundary(KeyKind kind) {
  std::mt19937 g(23);
  std::vector<Run> runs;
  runs.push_back(make_run(g, kind, 50, 12, 0));
  runs.push_back(make_run(g, kind, 30, 3, 1));
  runs.emplace_back();  // no records: no samples
  seal(&runs.back(), kind);
  {  // a block of equal keys much longer than the sample spacing, between two other keys
    Run r;
    r.recs.push_back({make_key(kind, "k1000"), "first"});
    for (int i = 0; i < 40; ++i) r.recs.push_back({make_key(kind, "k1014"), "dup" + std::to_string(i)});
    r.recs.push_back({make_key(kind, "k1099"), "last"});
    seal(&r, kind);
    runs.push_back(std::move(r));
  }
  const std::vector<std::string> keys = probe_keys(runs, kind);
  for (const Run& r : runs) {
    const SpillRun idx = index_host_run(r.heap.get(), r.len(), 48);
    EXPECT(idx.cut.empty() == r.recs.empty());
    SpillRun spilled = idx;  // the same run as a spill file: windows come through read_window
    spilled.mem = nullptr;
    int64_t window_bytes = 0;
    const ReadWindow window = [&](const SpillRun& run, int64_t off, int64_t len, uint8_t* dst) {
      if (&run != &spilled || off < 0 || len < 0 || off + len > r.body()) {
        EXPECT(false);
        return;
      }
      std::memcpy(dst, r.bytes.data() + off, (size_t)len);
      window_bytes += len;
    };
    bool all = true;
    for (const std::string& k : keys) {
      const int64_t want = oracle_boundary(r, k, kind);
      all = all && boundary(idx, k, kind) == want && boundary(spilled, k, kind, window) == want;
      ++checks;
    }
    EXPECT(all);
    EXPECT(r.recs.empty() || window_bytes > 0);
    // a key equal to a sample's key: the boundary is at or before that sample (equal keys may precede it)
    for (size_t j = 0; j < idx.cut.size(); ++j) EXPECT(boundary(idx, idx.key[j], kind) <= idx.cut[j]);
  }
  // the duplicate block: every sample inside it carries the block's key, and the boundary is its first record
  const Run& d = runs.back();
  const SpillRun idx = index_host_run(d.heap.get(), d.len(), 48);
  int inside = 0;
  for (const std::string& k : idx.key) inside += k == make_key(kind, "k1014");
  EXPECT(inside >= 3);
  EXPECT(boundary(idx, make_key(kind, "k1014"), kind) == d.off[1]);
  EXPECT(boundary(idx, make_key(kind, "k1015"), kind) == d.off[41]);
}

// --------------------------------------------------------------------- splitters and rounds: hybrid
static std::vector<Run> dup_runs(std::mt19937& g, KeyKind kind, int K, int distinct) {
  std::vector<Run> runs;
  for (int k = 0; k < K; ++k) runs.push_back(make_run(g, kind, 25 + 9 * k, distinct, k));
  return runs;
}

static void test_hybrid(KeyKind kind) {
  std::mt19937 g(37);
  const int64_t spacing = 96;
  for (int K : {1, 2, 5})
    for (int distinct : {3, 20}) {
      const std::vector<Run> runs = dup_runs(g, kind, K, distinct);
      const std::string want = oracle_merge(runs, kind);
      std::vector<SpillRun> idx;
      std::vector<int64_t> at((size_t)K, 0), end;
      for (const Run& r : runs) {
        idx.push_back(index_host_run(r.heap.get(), r.len(), spacing));
        end.push_back(idx.back().bytes);
      }
      for (int64_t target : {int64_t(1), spacing, (int64_t)want.size() + 1000}) {
        const std::vector<std::string> split = plan_splitters(idx, at, end, target, kind);
        for (size_t i = 1; i < split.size(); ++i) EXPECT(cmp(kind, split[i - 1], split[i]) < 0);
        if (target > (int64_t)want.size()) EXPECT(split.empty());
        if (target == 1 && K * distinct > 3) EXPECT(!split.empty());
        std::vector<std::vector<int64_t>> bnd((size_t)K);
        for (int k = 0; k < K; ++k)
          for (const std::string& s : split) bnd[(size_t)k].push_back(boundary(idx[(size_t)k], s, kind));
        const std::vector<RoundSlices> rounds = slice_rounds(bnd, at, end, false, false);
        EXPECT(rounds.size() == split.size() + 1);  // empty rounds are kept: the count is rpq_rounds
        std::string got;
        bool shape = !rounds.empty();
        for (size_t q = 0; shape && q < rounds.size(); ++q) {
          shape = merge_round(runs, rounds[q], kind, &got);
          for (int k = 0; shape && k < K; ++k) {
            const auto& sl = rounds[q][(size_t)k];
            shape = sl.first <= sl.second && sl.first == (q ? rounds[q - 1][(size_t)k].second : 0) &&
                    (q + 1 < rounds.size() || sl.second == runs[(size_t)k].body());
          }
        }
        EXPECT(shape);
        EXPECT(got == want);  // byte for byte: records equal to a splitter all went to the later round
      }
    }
}

// ---------------------------------------------------------------- splitters and rounds: progressive
static void test_progressive(KeyKind kind) {
  std::mt19937 g(53);
  const int64_t spacing = 80;
  for (int K : {1, 2, 5})
    for (int P : {2, 3, 7})
      for (int64_t target : {int64_t(1), spacing, int64_t(1) << 30}) {
        std::vector<Run> runs = dup_runs(g, kind, K, K == 2 ? 3 : 15);
        if (K == 5) {  // one partition without records among them
          runs[3] = Run();
          seal(&runs[3], kind);
        }
        const std::string want = oracle_merge(runs, kind);
        std::vector<SpillRun> idx((size_t)K);
        std::vector<RunCursor> cur((size_t)K);
        std::vector<int64_t> at((size_t)K, 0), had((size_t)K, 0);  // merged so far; bytes landed so far
        std::string got;
        bool shape = true, below_bound = true, no_empty = true, final_kept = false;
        for (int p = 0; p < P; ++p) {
          const bool final_phase = p + 1 == P;
          bool all_eof = true, blocked = false, have_bound = false;
          std::string bound;
          std::vector<std::unique_ptr<uint8_t[]>> landed((size_t)K);
          for (int k = 0; k < K; ++k) {
            const Run& r = runs[(size_t)k];
            // an arbitrary byte limit (any byte of a header, key, value or the marker); the last phase lands all
            const int64_t limit = final_phase ? r.len() : std::max<int64_t>(had[(size_t)k], (int64_t)(g() % (uint64_t)(r.len() + 1)));
            had[(size_t)k] = limit;
            landed[(size_t)k].reset(new uint8_t[(size_t)std::max<int64_t>(limit, 1)]);
            std::memcpy(landed[(size_t)k].get(), r.bytes.data(), (size_t)limit);
            SpillRun& v = idx[(size_t)k];
            v.mem = landed[(size_t)k].get();
            cur[(size_t)k].advance(v.mem, limit, spacing, &v.cut, &v.key);
            v.bytes = cur[(size_t)k].pos;
            if (cur[(size_t)k].eof || final_phase) continue;
            all_eof = false;
            const std::string lk = cur[(size_t)k].last_key(v.mem);
            if (lk.empty()) {
              blocked = true;
              continue;
            }
            if (!have_bound || cmp(kind, lk, bound) < 0) {
              bound = lk;
              have_bound = true;
            }
          }
          if (!all_eof && (blocked || !have_bound)) continue;  // nothing below any bound is known yet
          std::vector<int64_t> end((size_t)K);
          for (int k = 0; k < K; ++k)
            end[(size_t)k] = all_eof ? idx[(size_t)k].bytes : std::max(at[(size_t)k], boundary(idx[(size_t)k], bound, kind));
          const std::vector<std::string> split = plan_splitters(idx, at, end, target, kind);
          for (size_t i = 1; i < split.size(); ++i) EXPECT(cmp(kind, split[i - 1], split[i]) < 0);
          std::vector<std::vector<int64_t>> bnd((size_t)K);
          for (int k = 0; k < K; ++k)
            for (const std::string& s : split) bnd[(size_t)k].push_back(boundary(idx[(size_t)k], s, kind));
          const std::vector<RoundSlices> rounds = slice_rounds(bnd, at, end, true, all_eof);
          std::vector<int64_t> pos = at;
          for (size_t q = 0; q < rounds.size(); ++q) {
            std::vector<Rec> seen;
            shape = shape && merge_round(runs, rounds[q], kind, &got, &seen);
            int64_t bytes = 0;
            for (int k = 0; shape && k < K; ++k) {
              shape = rounds[q][(size_t)k].first == pos[(size_t)k];  // slices follow one another in every run
              pos[(size_t)k] = rounds[q][(size_t)k].second;
              bytes += rounds[q][(size_t)k].second - rounds[q][(size_t)k].first;
            }
            if (bytes == 0 && !(all_eof && q + 1 == rounds.size())) no_empty = false;
            if (!all_eof)
              for (const Rec& x : seen) below_bound = below_bound && cmp(kind, x.key, bound) < 0;
          }
          shape = shape && (rounds.empty() || pos == end);
          if (all_eof) final_kept = !rounds.empty();
          at = end;
          if (all_eof) break;
        }
        EXPECT(shape);
        EXPECT(below_bound);  // a record at or above the bound waits for a later call
        EXPECT(no_empty);     // rounds of zero bytes are dropped ...
        EXPECT(final_kept);   // ... except the last one of the final call, which carries the EOF
        EXPECT(got == want);
      }
}

// partitions without a record: the final call still plans one (empty) round, which carries the EOF
static void test_progressive_empty(KeyKind kind) {
  std::vector<Run> runs(2);
  for (Run& r : runs) seal(&r, kind);
  std::vector<SpillRun> idx;
  for (const Run& r : runs) idx.push_back(index_host_run(r.heap.get(), r.len(), 64));
  const std::vector<int64_t> at(2, 0), end(2, 0);
  EXPECT(plan_splitters(idx, at, end, 1, kind).empty());
  const std::vector<std::vector<int64_t>> bnd(2);
  EXPECT(slice_rounds(bnd, at, end, true, true).size() == 1);
  EXPECT(slice_rounds(bnd, at, end, true, false).empty());
  EXPECT(slice_rounds(bnd, at, end, false, false).size() == 1);
}

int main() {
  for (KeyKind kind : {KeyKind::kText, KeyKind::kBytes}) {
    test_walker(kind);
    test_boundary(kind);
    test_hybrid(kind);
    test_progressive(kind);
    test_progressive_empty(kind);
  }
  std::printf("%ld checks, %ld failures\n", checks, failures);
  return failures ? 1 : 0;
}
