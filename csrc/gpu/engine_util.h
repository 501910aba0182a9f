// Small helpers shared by the device engine's translation units (device_engine.h).
#pragma once
#include <chrono>
#include <cstdint>

namespace uda {
namespace gpu {

constexpr int kSlots = 2;  // recv/out double buffering across rounds

inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

}  // namespace gpu
}  // namespace uda
