#include "gpu_phase_fetch.h"

#include <algorithm>

namespace uda {

void ProgFetch::work() {
  ProgFetch& pf = *this;
  for (int64_t i; (i = pf.next++) < (int64_t)pf.P * pf.K;) {
    {
      std::lock_guard<std::mutex> g(pf.mu);
      if (*stop || pf.err) break;  // a stopped or failed task fetches no further phases
    }
    const int p = (int)(i / pf.K), k = (int)(i % pf.K);
    int64_t e = 0;
    try {
      MofFetcher& f = *pf.f[(size_t)k];
      const int64_t cap = pf.cap[(size_t)k];
      const int64_t b = cap * p / pf.P;
      e = cap * (p + 1) / pf.P;
      if (p == 0) {
        const int64_t off = f.take_first(pf.dst[(size_t)k], cap);
        if (off < e) task->fetch_direct(f.params(), pf.dst[(size_t)k], off, e, depth, nullptr, 0);
        e = std::max(e, off);
        st->copy(pf.dst[(size_t)k], pf.dev[(size_t)k], e, 0);
      } else if (b < e) {  // (may refetch bytes the first chunk already brought: same bytes)
        task->fetch_direct(f.params(), pf.dst[(size_t)k], b, e, depth, nullptr, 0);
        st->copy(pf.dst[(size_t)k] + b, pf.dev[(size_t)k] + b, e - b, p);
      }
    } catch (...) {
      std::lock_guard<std::mutex> g(pf.mu);
      if (!pf.err) pf.err = std::current_exception();
    }
    std::lock_guard<std::mutex> g(pf.mu);
    pf.landed[(size_t)p][(size_t)k] = e;
    if (++pf.done[(size_t)p] == pf.K && p + 1 == pf.P) pf.t_end = std::chrono::steady_clock::now();
    pf.cv.notify_all();
  }
}

void DirectProg::work() {
  DirectProg& dp = *this;
  for (int64_t i; (i = dp.next++) < (int64_t)dp.P * dp.K;) {
    {
      std::lock_guard<std::mutex> g(dp.mu);
      if (*stop || dp.err) break;
    }
    const int p = (int)(i / dp.K), k = (int)(i % dp.K);
    try {
      MofFetcher& f = *dp.f[(size_t)k];
      const int64_t cap = dp.cap[(size_t)k];
      const int64_t b = cap * p / dp.P, e = cap * (p + 1) / dp.P;
      if (p == 0) {
        const gpu::PinnedPool::Block blk = gpu::PinnedPool::instance().acquire((size_t)std::max<int64_t>(cap, 256));
        {
          std::lock_guard<std::mutex> g(dp.mu);
          dp.blocks[(size_t)k] = blk;
          dp.dst[(size_t)k] = blk.p;
          dp.cv.notify_all();
        }
        const int64_t off = f.take_first(dp.dst[(size_t)k], cap);
        if (off < e) task->fetch_direct(f.params(), dp.dst[(size_t)k], off, e, depth, nullptr, 0);
      } else if (b < e) {
        {  // its first phase (another thread) may still be taking the span
          std::unique_lock<std::mutex> lk(dp.mu);
          dp.cv.wait(lk, [&] { return dp.dst[(size_t)k] != nullptr || dp.err; });
          if (dp.err) break;
        }
        task->fetch_direct(f.params(), dp.dst[(size_t)k], b, e, depth, nullptr, 0);
      }
      std::unique_lock<std::mutex> lk(dp.mu);
      dp.fetched[(size_t)k][(size_t)p] = 1;
      index_landed(k, lk);
    } catch (...) {
      std::lock_guard<std::mutex> g(dp.mu);
      if (!dp.err) dp.err = std::current_exception();
      dp.cv.notify_all();
    }
  }
}

// index run k through every phase landed in order (one thread per run at a time); lk holds mu
void DirectProg::index_landed(int k, std::unique_lock<std::mutex>& lk) {
  DirectProg& dp = *this;
  const int64_t cap = dp.cap[(size_t)k];
  while (!dp.indexing[(size_t)k] && dp.indexed[(size_t)k] < dp.P &&
         dp.fetched[(size_t)k][(size_t)dp.indexed[(size_t)k]]) {
    dp.indexing[(size_t)k] = 1;
    const int q = dp.indexed[(size_t)k];
    const int64_t limit = std::min(cap * (q + 1) / dp.P, dp.body[(size_t)k]);
    lk.unlock();
    std::vector<int64_t> c;
    std::vector<std::string> kk;
    RunCursor& rc = dp.cur[(size_t)k];
    rc.advance(dp.dst[(size_t)k], limit, dp.spacing, &c, &kk);
    std::string lkey = rc.last_key(dp.dst[(size_t)k]);
    lk.lock();
    auto& vc = dp.cut[(size_t)k];
    auto& vk = dp.key[(size_t)k];
    vc.insert(vc.end(), c.begin(), c.end());
    for (auto& x : kk) vk.push_back(std::move(x));
    dp.complete[(size_t)k] = rc.pos;
    if (!lkey.empty()) dp.last_key[(size_t)k] = std::move(lkey);
    if (rc.eof || q + 1 == dp.P) dp.eof[(size_t)k] = 1;
    dp.indexed[(size_t)k] = q + 1;
    dp.indexing[(size_t)k] = 0;
    if (++dp.phase_runs[(size_t)q] == dp.K && q + 1 == dp.P) dp.t_end = std::chrono::steady_clock::now();
    dp.cv.notify_all();
  }
}

}  // namespace uda
