// TEST-ONLY: launchers for the two kernels of the paired probe runs (lz_probe_real_pc, lz_probe_dots_pair<M> of
// csrc/hxv_lanczos_kernels.hpp) and for the single driver's complex overlap kernel they are compared with, so that
// tests/test_gpu_pair_probe_kernels.py can run each alone, with grids and sizes the driver never passes.  The kernels are the header's text,
// compiled with the engine's flags (build_pair_probe_kernels_check() of __graft_entry__.py); this library is never linked into libhxv.so.
//
// Every entry takes device pointers, launches on the null stream with 256 threads per workgroup, waits, and returns the HIP status; the
// overlaps go through launch_probe_dots_pair / launch_probe_dots, so the dispatch on m and lz_probe_final are under test.  An empty grid, a
// negative length, m outside 1 .. HXV_MAX_PROBES or a zero pitch are refused (hipErrorInvalidValue) before anything is launched.
#include "hxv_lanczos_kernels.hpp"

namespace {
int finish() {
  hipError_t e = hipGetLastError();
  hipError_t s = hipStreamSynchronize(nullptr);
  return (int)(e != hipSuccess ? e : s);
}
constexpr int BAD = (int)hipErrorInvalidValue;
bool bad_grid(int grid) { return grid < 1 || grid > RED_BLOCKS; }
}  // namespace

extern "C" {

int ppc_red_blocks() { return RED_BLOCKS; }

int ppc_probe_real_pc(int grid, int64_t n, int dimup, int pitch, const void* src, double* dst, double* partial) {
  if (bad_grid(grid) || n < 0 || pitch < 1 || dimup < 0) return BAD;
  hipLaunchKernelGGL(lz_probe_real_pc, dim3(grid), dim3(256), 0, nullptr, n, dimup, pitch, (const double2*)src, dst, partial);
  return finish();
}

// probes: m HOST-side entries, each a device pointer to n doubles.  lz_probe_dots_pair<m> on `grid` workgroups, lz_probe_final on one.
int ppc_probe_dots_pair(int grid, int m, int64_t n, const void* x, const void* const* probes, double* d_part, double* d_out) {
  if (bad_grid(grid) || n < 0 || m < 1 || m > HXV_MAX_PROBES || !probes) return BAD;
  LzRealProbes pr{};
  for (int j = 0; j < m; ++j) pr.p[j] = (const double*)probes[j];
  launch_probe_dots_pair(grid, nullptr, m, n, (const double2*)x, pr, d_part, d_out);
  return finish();
}

// the single driver's complex path: probes are m device pointers to n double2 elements
int ppc_probe_dots_complex(int grid, int m, int64_t n, const void* x, const void* const* probes, double* d_part, double* d_out) {
  if (bad_grid(grid) || n < 0 || m < 1 || m > HXV_MAX_PROBES || !probes) return BAD;
  LzProbes pr{};
  for (int j = 0; j < m; ++j) pr.p[j] = (const double2*)probes[j];
  launch_probe_dots<false>(grid, nullptr, m, n, (const double2*)x, pr, d_part, d_out);
  return finish();
}

}  // extern "C"
