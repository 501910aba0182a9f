// See block_rounds.h.
#include "block_rounds.h"

#include <algorithm>
#include <iterator>

namespace uda {
namespace gpu {

namespace {
int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
}  // namespace

std::vector<int32_t> block_first_offsets(const BlockGeometry& g) {
  const int K = (int)g.nrec.size();
  std::vector<int32_t> first(g.rel.size(), -1);
  for (int k = 0; k < K; ++k)
    for (int64_t b = g.blk0[(size_t)k]; b < g.blk0[(size_t)k + 1]; ++b) {
      const int64_t rel = g.rel[(size_t)b];
      const int64_t f = (kBlockRecordBytes - rel % kBlockRecordBytes) % kBlockRecordBytes;
      if (rel + f + kBlockRecordBytes <= g.nrec[(size_t)k] * kBlockRecordBytes && f + kBlockKeyEnd <= g.raw[(size_t)b])
        first[(size_t)b] = (int32_t)f;
    }
  return first;
}

bool build_block_index(const BlockGeometry& g, const std::vector<int32_t>& first, const std::vector<BlockKey>& keys,
                       BlockIndex* out) {
  const int K = (int)g.nrec.size();
  out->idx.assign((size_t)K, {});
  out->samp.clear();
  for (int k = 0; k < K; ++k)
    for (int64_t b = g.blk0[(size_t)k]; b < g.blk0[(size_t)k + 1]; ++b)
      if (first[(size_t)b] >= 0) {
        auto& ix = out->idx[(size_t)k];
        if (!ix.empty() && block_key_less(keys[(size_t)b], ix.back().second)) return false;  // not a sorted run
        ix.emplace_back(b, keys[(size_t)b]);
        out->samp.push_back(keys[(size_t)b]);
      }
  std::sort(out->samp.begin(), out->samp.end(), block_key_less);
  return true;
}

void plan_rounds(const BlockGeometry& g, const BlockIndex& index, int64_t round_bytes, RoundPlan* out) {
  const int K = (int)g.nrec.size();
  const int64_t rb = std::max<int64_t>(round_bytes, kBlockRecordBytes);
  int64_t N = 0;
  for (int k = 0; k < K; ++k) N += g.nrec[(size_t)k];
  const std::vector<BlockKey>& samp = index.samp;
  const int Q = (int)std::max<int64_t>(1, (N * kBlockRecordBytes + rb - 1) / rb);
  out->Q = Q;
  out->bounds.assign((size_t)std::max(0, Q - 1), BlockKey{0, 0});
  for (int q = 1; q < Q; ++q)
    out->bounds[(size_t)q - 1] = samp.empty() ? BlockKey{~0ull, ~0ull} : samp[samp.size() * (size_t)q / (size_t)Q];
  out->spans.assign((size_t)Q, std::vector<RoundSpan>((size_t)K));
  out->in_bytes.assign((size_t)Q, 0);
  out->in_recs.assign((size_t)Q, 0);
  auto key_below = [](const std::pair<int64_t, BlockKey>& a, const BlockKey& v) { return block_key_less(a.second, v); };
  for (int q = 0; q < Q; ++q) {
    int64_t cur = 0;
    for (int k = 0; k < K; ++k) {
      RoundSpan& sp = out->spans[(size_t)q][(size_t)k];
      const int64_t nrec = g.nrec[(size_t)k], blk0 = g.blk0[(size_t)k], blk1 = g.blk0[(size_t)k + 1];
      if (nrec == 0 || blk0 == blk1) continue;
      const auto& ix = index.idx[(size_t)k];
      // b0: the last block starting a record with a key below the low bound (round 0: the first block)
      sp.b0 = blk0;
      if (q > 0) {
        auto it = std::lower_bound(ix.begin(), ix.end(), out->bounds[(size_t)q - 1], key_below);
        if (it != ix.begin()) sp.b0 = std::prev(it)->first;
      }
      // b1: the first block starting a record with a key at or above the high bound (last round: the last block)
      sp.b1 = blk1 - 1;
      if (q + 1 < Q) {
        auto it = std::lower_bound(ix.begin(), ix.end(), out->bounds[(size_t)q], key_below);
        if (it != ix.end()) sp.b1 = it->first;
      }
      if (sp.b1 < sp.b0) sp.b1 = sp.b0;
      const int64_t r0 = g.rel[(size_t)sp.b0], r1 = g.rel[(size_t)sp.b1] + g.raw[(size_t)sp.b1];
      sp.rec0 = (r0 + kBlockRecordBytes - 1) / kBlockRecordBytes;
      sp.rec1 = std::min(r1 / kBlockRecordBytes, nrec);
      if (sp.rec1 < sp.rec0) sp.rec1 = sp.rec0;
      const int64_t lead = sp.rec0 * kBlockRecordBytes - r0;  // partial record before the first whole one
      sp.in_off = align_up(cur + lead, 16) - lead;             // record starts 16-byte aligned
      cur = sp.in_off + (r1 - r0);
      out->in_recs[(size_t)q] += sp.rec1 - sp.rec0;
    }
    out->in_bytes[(size_t)q] = align_up(cur, 256);
  }
}

}  // namespace gpu
}  // namespace uda
