// What one driver call borrows, returned on every way out of it.  A driver takes its vector-sized scratch from the engine's buffer cache
// (take) and its small per-call tables from the runtime (take_device); the scope's destructor -- or release(), for a driver that reads a
// copy-back afterwards -- synchronises the handle's stream ONCE, so that nothing enqueued by the call still uses a block, and gives every
// block back the way it came.  A scope that holds nothing touches neither the stream nor the runtime.  What a HANDLE keeps across calls
// (d_lz, d_wt, the staging and gather buffers, h_probe_ov) is not per-call scratch and never goes through a scope.
#pragma once
#include <utility>
#include <vector>

#include "hxv_handle.hpp"

namespace hxv {
class CallScope {
 public:
  explicit CallScope(const hxv_handle* h) : device_(h->device), stream_(h->stream) {}
  CallScope(const CallScope&) = delete;
  CallScope& operator=(const CallScope&) = delete;
  ~CallScope() { release(); }
  // *out = a block of `bytes` from pool_alloc / from hipMalloc; on failure the error and *out = nullptr
  template <typename T>
  hipError_t take(size_t bytes, T** out) {
    return keep(pool_alloc(device_, bytes, (void**)out), (void**)out, true);
  }
  template <typename T>
  hipError_t take_device(size_t bytes, T** out) {
    return keep(hipMalloc((void**)out, bytes), (void**)out, false);
  }
  void release() {
    if (held_.empty()) return;
    (void)hipStreamSynchronize(stream_);
    for (const auto& b : held_) {
      if (b.second)
        pool_free(device_, b.first);
      else
        (void)hipFree(b.first);
    }
    held_.clear();
  }

 private:
  hipError_t keep(hipError_t e, void** out, bool pooled) {
    if (e == hipSuccess)
      held_.emplace_back(*out, pooled);
    else
      *out = nullptr;
    return e;
  }
  int device_;
  hipStream_t stream_;
  std::vector<std::pair<void*, bool>> held_;  // (block, from the buffer cache?)
};

// THE scratch of a driver that takes overlaps with probes (both tridiagonalisation drivers, chebyshev_run), carved from ONE pooled block: the
// block partials of the check of the vectors' imaginary parts, the block partials of one step's sums, and those sums; with it the handle's
// page-locked staging for n_stage doubles (a copy of the sums into the caller's pageable array could make the runtime wait per step).
struct ProbeScratch {
  double *chk = nullptr, *part = nullptr, *sums = nullptr;
  int take(hxv_handle* h, CallScope& pooled, size_t n_chk, size_t n_part, size_t n_sums, int64_t n_stage) {
    HIPCHK(pooled.take((n_chk + n_part + n_sums) * sizeof(double), &chk));
    part = chk + n_chk;
    sums = part + n_part;
    return ensure_probe_stage(h, n_stage);
  }
};
}  // namespace hxv
