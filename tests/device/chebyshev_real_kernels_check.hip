// TEST-ONLY: launchers for the two REAL-vector kernels of the Chebyshev recurrence, the conversion that opens a real run and the kernel of
// hxv_vector_random, so that tests/test_gpu_chebyshev_real_kernels.py can run each of them alone, with a grid and sizes the driver never
// passes, and compare it with an exact restatement (tests/chebyshev_real_ref.py).  The kernels are the text of
// csrc/hxv_chebyshev_real_kernels.hpp, compiled with the engine's flags (build_chebyshev_real_kernels_check() of __graft_entry__.py); this
// library is never linked into libhxv.so.  The COMPLEX launchers of csrc/hxv_chebyshev_kernels.hpp are exported beside them, so that the test
// can run both forms on the same memory and compare the stored vectors and the Re accumulators bit for bit.
//
// Every entry takes device pointers and the kernel's own arguments unchanged, with the grid in front; it launches on the null stream, waits,
// and returns the HIP status.  n counts double2 elements (two reals each).  Arguments no launch can take are refused
// (hipErrorInvalidValue) before anything is launched.
#include "hxv_chebyshev_real_kernels.hpp"

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

// out[0..3] = RED_BLOCKS, HXV_MAX_PROBES, ch_sums_real(0), ch_sums(0)
void crk_constants(int* out) {
  out[0] = RED_BLOCKS;
  out[1] = HXV_MAX_PROBES;
  out[2] = ch_sums_real(0);
  out[3] = ch_sums(0);
}

// probes: m HOST-side entries, each a device pointer.  d_part: grid * (m+2) doubles, d_sums: m+2.  out may be null.
int crk_init(int grid, int m, int64_t n, const void* v, void* out, const void* const* probes, double c0, double* d_part, double* d_sums) {
  if (bad_shape(grid, m, n, probes)) return BAD;
  launch_ch_init_real(grid, nullptr, m, n, (const double2*)v, (double2*)out, probe_list(m, probes), c0, d_part, d_sums);
  return finish();
}

// out null: no running sum; first != 0: the form without t_prev (prev_next is written, not read)
int crk_step(int grid, int m, int first, int64_t n, const void* hv, const void* cur, void* prev_next, void* out, const void* const* probes,
             double ch, double cc, double cr, double* d_part, double* d_sums) {
  if (bad_shape(grid, m, n, probes)) return BAD;
  launch_ch_step_real(grid, nullptr, m, first != 0, n, (const double2*)hv, (const double2*)cur, (double2*)prev_next, (double2*)out,
                      probe_list(m, probes), ch, cc, cr, d_part, d_sums);
  return finish();
}

// the COMPLEX kernels on the same memory (d_part: grid * (2m+3), d_sums: 2m+3)
int crk_complex_init(int grid, int m, int64_t n, const void* v, void* out, const void* const* probes, double c0r, double c0i, double* d_part,
                     double* d_sums) {
  if (bad_shape(grid, m, n, probes)) return BAD;
  launch_ch_init(grid, nullptr, m, n, (const double2*)v, (double2*)out, probe_list(m, probes), c0r, c0i, d_part, d_sums);
  return finish();
}
int crk_complex_step(int grid, int m, int first, int64_t n, const void* hv, const void* cur, void* prev_next, void* out, const void* const* probes,
                     double ch, double cc, double cr, double ci, double* d_part, double* d_sums) {
  if (bad_shape(grid, m, n, probes)) return BAD;
  launch_ch_step(grid, nullptr, m, first != 0, n, (const double2*)hv, (const double2*)cur, (double2*)prev_next, (double2*)out,
                 probe_list(m, probes), ch, cc, cr, ci, d_part, d_sums);
  return finish();
}

// src: complex [dimdw][pc], dst: real [dimdw][pr], partial: grid doubles (per-block sums of |Im| over the rows below dimup)
int crk_to_real(int grid, int dimup, int dimdw, int pc, int pr, const void* src, double* dst, double* partial) {
  if (grid < 1 || grid > RED_BLOCKS || dimup < 0 || dimdw < 0 || pc < dimup || pr < dimup || !dst || !partial) return BAD;
  hipLaunchKernelGGL(ch_to_real, dim3(grid), dim3(256), 0, nullptr, dimup, dimdw, pc, pr, (const double2*)src, dst, partial);
  return finish();
}

// q: n = ncols * pitch complex elements; iperm / sign may be null (the reference's row order); key = vr_mix(seed) is taken here
int crk_random(int grid, int64_t n, void* q, uint64_t seed, int complex_valued, int dimup, int pitch, int col0, const int32_t* iperm,
               const uint8_t* sign) {
  if (grid < 1 || grid > RED_BLOCKS || n < 0 || dimup < 1 || pitch < dimup || n % pitch != 0) return BAD;
  hipLaunchKernelGGL(vec_random, dim3(grid), dim3(256), 0, nullptr, n, (double2*)q, vr_mix(seed), complex_valued, dimup, pitch, col0, iperm, sign);
  return finish();
}

uint64_t crk_mix(uint64_t x) { return vr_mix(x); }

}  // extern "C"
