// TEST-ONLY: launchers for the two kernels of the Chebyshev recurrence, so that tests/test_gpu_chebyshev_kernels.py can run each of them
// alone, with a grid and sizes the driver never passes, and compare it with an exact restatement (tests/chebyshev_ref.py).  The kernels are
// the text of csrc/hxv_chebyshev_kernels.hpp, compiled with the engine's flags (build_chebyshev_kernels_check() of __graft_entry__.py);
// this library is never linked into libhxv.so.
//
// Every entry takes device pointers and the kernel's own arguments unchanged, with the grid in front; it launches on the null stream, waits,
// and returns the HIP status.  Both go through the driver's own launch functions, so the dispatch on the number of probes, on the running sum
// and on the first-step form is under test, and so is the final kernel that adds the block partials.  Arguments no launch can take (an
// empty grid, a negative length, m outside [0, HXV_MAX_PROBES], a missing probe list) are refused (hipErrorInvalidValue) before anything is
// launched.
#include "hxv_chebyshev_kernels.hpp"

namespace {

int finish() {
  hipError_t e = hipGetLastError();
  hipError_t s = hipStreamSynchronize(nullptr);
  return (int)(e != hipSuccess ? e : s);
}

constexpr int BAD = (int)hipErrorInvalidValue;

bool bad_shape(int grid, int m, int64_t n, const void* const* probes) {
  return grid < 1 || grid > RED_BLOCKS || n < 0 || m < 0 || m > HXV_MAX_PROBES || (m > 0 && !probes);
}

LzProbes probe_list(int m, const void* const* probes) {
  LzProbes pr{};
  for (int j = 0; j < m; ++j) pr.p[j] = (const double2*)probes[j];
  return pr;
}

}  // namespace

extern "C" {

// out[0..2] = RED_BLOCKS, HXV_MAX_PROBES, ch_sums(0)
void ckc_constants(int* out) {
  out[0] = RED_BLOCKS;
  out[1] = HXV_MAX_PROBES;
  out[2] = ch_sums(0);
}

// the grid the driver launches both kernels on for n elements
int ckc_grid_for(int64_t n) { return grid_for(n); }

// probes: m HOST-side entries, each a device pointer.  d_part: grid * (2m+3) doubles, d_sums: 2m+3.  out may be null.
int ckc_init(int grid, int m, int64_t n, const void* v, void* out, const void* const* probes, double c0r, double c0i, double* d_part,
             double* d_sums) {
  if (bad_shape(grid, m, n, probes)) return BAD;
  launch_ch_init(grid, nullptr, m, n, (const double2*)v, (double2*)out, probe_list(m, probes), c0r, c0i, d_part, d_sums);
  return finish();
}

// out null: no running sum; first != 0: the form without t_prev (prev_next is written, not read)
int ckc_step(int grid, int m, int first, int64_t n, const void* hv, const void* cur, void* prev_next, void* out, const void* const* probes,
             double ch, double cc, double cr, double ci, double* d_part, double* d_sums) {
  if (bad_shape(grid, m, n, probes)) return BAD;
  launch_ch_step(grid, nullptr, m, first != 0, n, (const double2*)hv, (const double2*)cur, (double2*)prev_next, (double2*)out,
                 probe_list(m, probes), ch, cc, cr, ci, d_part, d_sums);
  return finish();
}

}  // extern "C"
