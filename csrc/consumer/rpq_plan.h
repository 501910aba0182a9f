// RPQ planning on the host: sorted runs with a sparse index (the key at a record boundary every
// `spacing` bytes), the key-range rounds cut from those indices, and each run's byte slice per round.
// Records equal to a splitter all fall in the later round, in every run, so ties keep run order.
// No device, task or tracing state: the GPU merge (gpu_merge_staged.cc) owns those.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "uda/compare.h"
#include "uda/ifile.h"

namespace uda {

// A sorted run of whole records with its sparse index: one merged LPQ output resident in host memory
// or in a spill file, or (direct RPQ) a fetched partition where the fetch put it.
struct SpillRun {
  uint8_t* mem = nullptr;         // host tier: pinned (spill arena)
  std::string path;
  int fd = -1;
  int64_t bytes = 0;
  std::vector<int64_t> cut;       // record-boundary offsets (first 0)
  std::vector<std::string> key;   // key bytes of the record at each cut
};

std::string key_at(const uint8_t* p, int64_t avail);
int cmp_key(KeyKind kind, const std::string& a, const std::string& b);

// The sparse-index walk of a run that lands in byte phases: walks the complete records of [pos, limit)
// (the bytes landed so far), a sample every `spacing` bytes; a record the landed bytes cut is left for
// the next call. Samples go to the caller's vectors; the cursor and the last complete record stay here.
struct RunCursor {
  int64_t pos = 0, next_cut = 0;
  int64_t last = -1;  // start of the last complete record walked
  bool eof = false;
  void advance(const uint8_t* p, int64_t limit, int64_t spacing, std::vector<int64_t>* cut, std::vector<std::string>* key);
  std::string last_key(const uint8_t* p) const;
};

// Direct RPQ: a fetched partition, already a sorted run in pinned DRAM, becomes an RPQ input as it is:
// the record boundary at or after every `spacing` bytes and its key, by one walk of the VInt headers
// (RunCursor through `len`). bytes = the records (an EOF marker ends the walk and is left out).
SpillRun index_host_run(uint8_t* p, int64_t len, int64_t spacing);

// read [off, off + len) of a run that is not in memory into dst
using ReadWindow = std::function<void(const SpillRun& run, int64_t off, int64_t len, uint8_t* dst)>;

// First record of `run` whose key is >= `key`: the last sample below the key, then a record scan of that
// sample's window (in place for a run in memory; through read_window for a spilled one).
int64_t boundary(const SpillRun& run, const std::string& key, KeyKind kind, const ReadWindow& read_window = nullptr);

// Splitters every ~target bytes of the runs' windows [at[k], end[k]): the samples inside the windows in
// (key, run, index) order, each standing for the bytes up to its run's next cut (or the window's end);
// strictly ascending.
std::vector<std::string> plan_splitters(const std::vector<SpillRun>& runs, const std::vector<int64_t>& at,
                                        const std::vector<int64_t>& end, int64_t target, KeyKind kind);

// A round: one [b, e) slice per run.
using RoundSlices = std::vector<std::pair<int64_t, int64_t>>;

// The rounds of the windows [at[k], end[k]) cut at bnd[k][i] = boundary(run k, splitter i), clamped
// monotone within the window. drop_empty: rounds of zero bytes are left out, except the last one when
// keep_last is set (a progressive plan's final call delivers the EOF with it).
std::vector<RoundSlices> slice_rounds(const std::vector<std::vector<int64_t>>& bnd, const std::vector<int64_t>& at,
                                      const std::vector<int64_t>& end, bool drop_empty, bool keep_last);

}  // namespace uda
