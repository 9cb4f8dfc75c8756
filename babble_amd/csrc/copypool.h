// copypool.h — the host entries' thread pool: parallel memcpy into / out of
// pinned staging, and the O(n) argument scans.  Host-only code.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

// ---------------------------------------------------------------------------
// host copy pool: parallel memcpy into / out of pinned staging
// ---------------------------------------------------------------------------
struct CopyPool {
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv, done_cv;
  std::vector<std::function<void()>> q;
  size_t pending = 0;
  bool stop = false;
  explicit CopyPool(int n) {
    for (int i = 0; i < n; i++)
      th.emplace_back([this]() {
        for (;;) {
          std::function<void()> f;
          {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [this]() { return stop || !q.empty(); });
            if (stop && q.empty()) return;
            f = std::move(q.back());
            q.pop_back();
          }
          f();
          std::lock_guard<std::mutex> lk(mu);
          if (--pending == 0) done_cv.notify_all();
        }
      });
  }
  ~CopyPool() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv.notify_all();
    for (auto &t : th) t.join();
  }
  // fn(lo, hi) over [0, n) in `grain`-sized ranges on the pool and the
  // caller; returns false if any range returned false.
  bool parallel_for(uint64_t n, uint64_t grain, const std::function<bool(uint64_t, uint64_t)> &fn) {
    if (n <= grain || th.empty()) return fn(0, n);
    const uint64_t parts = (n + grain - 1) / grain;
    std::atomic<bool> ok{true};
    {
      std::lock_guard<std::mutex> lk(mu);
      for (uint64_t i = 1; i < parts; i++) {
        const uint64_t lo = i * grain, hi = std::min(n, lo + grain);
        q.push_back([&fn, &ok, lo, hi]() {
          if (!fn(lo, hi)) ok = false;
        });
        pending++;
      }
    }
    cv.notify_all();
    if (!fn(0, std::min(n, grain))) ok = false;
    std::unique_lock<std::mutex> lk(mu);
    done_cv.wait(lk, [this]() { return pending == 0; });
    return ok;
  }
  // dst <- src (n bytes); returns when done.  Small copies stay on the caller.
  void copy(void *dst, const void *src, size_t n) {
    constexpr size_t kPiece = 2ull << 20;
    if (n <= kPiece || th.empty()) {
      if (n) memcpy(dst, src, n);
      return;
    }
    const size_t pieces = (n + kPiece - 1) / kPiece;
    {
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 1; i < pieces; i++) {
        const size_t o = i * kPiece, len = std::min(kPiece, n - o);
        q.push_back([=]() { memcpy((uint8_t *)dst + o, (const uint8_t *)src + o, len); });
        pending++;
      }
    }
    cv.notify_all();
    memcpy(dst, src, std::min(kPiece, n));  // the caller copies the first piece
    std::unique_lock<std::mutex> lk(mu);
    done_cv.wait(lk, [this]() { return pending == 0; });
  }
  // several copies at once (the pieces of one staging chunk), split into
  // 1 MB parts spread over the pool; returns when all are done
  struct Piece {
    void *dst;
    const void *src;
    size_t n;
  };
  void copy_many(const std::vector<Piece> &v) {
    constexpr size_t kPart = 1ull << 20;
    std::vector<Piece> parts;
    for (const Piece &p : v)
      for (size_t o = 0; o < p.n; o += kPart)
        parts.push_back({(uint8_t *)p.dst + o, (const uint8_t *)p.src + o, std::min(kPart, p.n - o)});
    if (parts.size() <= 1 || th.empty()) {
      for (const Piece &p : parts) memcpy(p.dst, p.src, p.n);
      return;
    }
    {
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 1; i < parts.size(); i++) {
        const Piece p = parts[i];
        q.push_back([p]() { memcpy(p.dst, p.src, p.n); });
        pending++;
      }
    }
    cv.notify_all();
    memcpy(parts[0].dst, parts[0].src, parts[0].n);
    std::unique_lock<std::mutex> lk(mu);
    done_cv.wait(lk, [this]() { return pending == 0; });
  }
};

// off[i] <= off[i + 1] for every i < n, scanned on the pool when there is one
inline bool monotone(CopyPool *pool, const uint64_t *off, uint64_t n, uint64_t grain = 1 << 17) {
  const auto scan = [off](uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; i++)
      if (off[i] > off[i + 1]) return false;
    return true;
  };
  return pool ? pool->parallel_for(n, grain, scan) : scan(0, n);
}
