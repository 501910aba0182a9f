// Keeps fixed windows of every reducer's delivered stream: a delivery sink wrapped with a sampler sees
// the same buffers, and the sampler copies the bytes that fall into its windows. The windows are byte
// ranges of a reducer's stream (the concatenation of its dataFromUda buffers), so what is kept does not
// depend on where the buffers were cut. One delivering thread per reducer, as for the sink itself.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

namespace uda {
namespace gpu {

class StreamSampler {
 public:
  // starts[r]: ascending stream offsets of reducer r's windows, each `window` bytes, not overlapping
  StreamSampler(std::vector<std::vector<int64_t>> starts, int64_t window) : window_(window) {
    if (window <= 0) throw std::invalid_argument("StreamSampler: window must be positive");
    for (auto& v : starts) {
      for (size_t i = 0; i < v.size(); ++i)
        if (v[i] < 0 || (i > 0 && v[i] < v[i - 1] + window))
          throw std::invalid_argument("StreamSampler: window starts must ascend without overlap");
      st_.emplace_back(new State);
      st_.back()->data.assign(v.size() * (size_t)window, 0);
      st_.back()->starts = std::move(v);
    }
  }

  int reducers() const { return (int)st_.size(); }
  int64_t window() const { return window_; }
  int64_t windows(int r) const { return (int64_t)st_[(size_t)r]->starts.size(); }

  void reset() {
    for (auto& sp : st_) {
      sp->pos = 0;
      sp->next = 0;
      sp->captured = 0;
      std::fill(sp->data.begin(), sp->data.end(), 0);
    }
  }

  // The next `len` bytes of reducer r's stream.
  void observe(int r, const uint8_t* buf, int64_t len) {
    State& s = *st_[(size_t)r];
    const int64_t b0 = s.pos, b1 = b0 + len;
    s.pos = b1;
    while (s.next < s.starts.size()) {
      const int64_t w0 = s.starts[s.next], w1 = w0 + window_;
      if (w0 >= b1) break;
      const int64_t lo = std::max(w0, b0), hi = std::min(w1, b1);
      if (lo < hi) {
        std::memcpy(s.data.data() + s.next * (size_t)window_ + (size_t)(lo - w0), buf + (lo - b0), (size_t)(hi - lo));
        s.captured += hi - lo;
      }
      if (w1 > b1) break;  // the window goes on in the next buffer
      ++s.next;
    }
  }

  int64_t stream_bytes(int r) const { return st_[(size_t)r]->pos; }
  int64_t captured_bytes(int r) const { return st_[(size_t)r]->captured; }
  const std::vector<uint8_t>& data(int r) const { return st_[(size_t)r]->data; }

 private:
  struct alignas(64) State {
    std::vector<int64_t> starts;
    std::vector<uint8_t> data;
    int64_t pos = 0, captured = 0;
    size_t next = 0;
  };
  int64_t window_;
  std::vector<std::unique_ptr<State>> st_;
};

}  // namespace gpu
}  // namespace uda
