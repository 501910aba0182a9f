#include "delivery_schedule.h"

#include <algorithm>
#include <stdexcept>

namespace uda {
namespace gpu {

void check_delivery_order(const std::string& order) {
  if (order != "wave" && order != "reducer") throw std::runtime_error("delivery_order must be wave or reducer");
}

std::vector<DeliveryPiece> delivery_schedule(const std::vector<int64_t>& group_recs, int64_t piece_bytes,
                                             const std::string& order, int64_t record_bytes) {
  check_delivery_order(order);
  if (record_bytes < 1) throw std::runtime_error("delivery_schedule: record_bytes < 1");
  const int64_t piece = std::max<int64_t>(1, piece_bytes / record_bytes) * record_bytes;
  // reducer-major: today's order, and the numbering of pack_index
  std::vector<DeliveryPiece> v;
  std::vector<size_t> first(group_recs.size() + 1, 0);  // reducer i's pieces are v[first[i] .. first[i + 1])
  int64_t goff = 0;
  size_t waves = 0;
  for (size_t i = 0; i < group_recs.size(); ++i) {
    if (group_recs[i] < 0) throw std::runtime_error("delivery_schedule: negative record count");
    const int64_t bytes = group_recs[i] * record_bytes;
    for (int64_t off = 0; off < bytes;) {
      const int64_t len = std::min(piece, bytes - off);
      off += len;
      v.push_back(DeliveryPiece{(int)i, goff + off - len, len, (int)v.size(), off >= bytes});
    }
    goff += bytes;
    first[i + 1] = v.size();
    waves = std::max(waves, first[i + 1] - first[i]);
  }
  if (order == "reducer") return v;
  std::vector<DeliveryPiece> w;
  w.reserve(v.size());
  for (size_t k = 0; k < waves; ++k)
    for (size_t i = 0; i < group_recs.size(); ++i)
      if (first[i] + k < first[i + 1]) w.push_back(v[first[i] + k]);
  return w;
}

}  // namespace gpu
}  // namespace uda
