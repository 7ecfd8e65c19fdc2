// TEST-ONLY: one launcher per kernel of the single-vector Lanczos recurrence, so that tests/test_gpu_lanczos_kernels.py can run each kernel
// alone and compare it with an exact sum or an exact restatement (tests/lanczos_kernels_ref.py).  The kernels are the text of
// csrc/hxv_lanczos_kernels.hpp, compiled with the engine's flags (build_lanczos_kernels_check() of __graft_entry__.py); this library is
// never linked into libhxv.so.
//
// Every entry takes device pointers and the kernel's own arguments unchanged, with the grid in front; it launches on the null stream,
// waits, and returns the HIP status.  Streaming kernels run with 256 threads per workgroup, the scalar kernels (lz_mul, lz_sqrt, lz_next)
// with one thread of one workgroup, as the drivers launch them.  The probe overlaps go through launch_probe_dots, so the dispatch on m is
// under test.  Arguments beyond what a kernel's fixed-size tables hold, or that no launch can take (an empty grid, a negative length, a
// negative scalar slot, a zero pitch), are refused (hipErrorInvalidValue) before anything is launched.
#include "hxv_lanczos_host.hpp"
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

// out[0..6] = RED_BLOCKS, HXV_MAX_PROBES, LZ_ALPHA, LZ_BETA, LZ_S, LZ_C, LZ_STEP
void lkc_constants(int* out) {
  out[0] = RED_BLOCKS;
  out[1] = HXV_MAX_PROBES;
  out[2] = LZ_ALPHA;
  out[3] = LZ_BETA;
  out[4] = LZ_S;
  out[5] = LZ_C;
  out[6] = LZ_STEP;
}

int lkc_grid_for(int64_t n) { return grid_for(n); }

int lkc_sub_dot(int grid, int64_t n, void* w, const void* qm, const void* q, const double* scal, int ib, double* partial) {
  if (bad_grid(grid) || n < 0) return BAD;
  hipLaunchKernelGGL(lz_sub_dot, dim3(grid), dim3(256), 0, nullptr, n, (double2*)w, (const double2*)qm, (const double2*)q, scal, ib, partial);
  return finish();
}

int lkc_sub_nrm(int grid, int64_t n, void* w, const void* q, const double* scal, int ia, double* partial) {
  if (bad_grid(grid) || n < 0 || ia < 0) return BAD;
  hipLaunchKernelGGL(lz_sub_nrm, dim3(grid), dim3(256), 0, nullptr, n, (double2*)w, (const double2*)q, scal, ia, partial);
  return finish();
}

int lkc_sub_nrm_pair(int grid, int64_t n, void* w, const void* q, const double* scal, int ia, int ib, double* partial_a, double* partial_b) {
  if (bad_grid(grid) || n < 0 || ia < 0 || ib < 0) return BAD;
  hipLaunchKernelGGL(lz_sub_nrm_pair, dim3(grid), dim3(256), 0, nullptr, n, (double2*)w, (const double2*)q, scal, ia, ib, partial_a, partial_b);
  return finish();
}

int lkc_pack_pair(int grid, int64_t n, const void* a, const void* b, void* q, double* p_im, double* p_a, double* p_b) {
  if (bad_grid(grid) || n < 0) return BAD;
  hipLaunchKernelGGL(lz_pack_pair, dim3(grid), dim3(256), 0, nullptr, n, (const double2*)a, (const double2*)b, (double2*)q, p_im, p_a, p_b);
  return finish();
}

int lkc_nrm(int grid, int64_t n, const void* x, double* partial) {
  if (bad_grid(grid) || n < 0) return BAD;
  hipLaunchKernelGGL(lz_nrm, dim3(grid), dim3(256), 0, nullptr, n, (const double2*)x, partial);
  return finish();
}

int lkc_final(int grid, const double* partial, int np, double* scal, int io, int op) {
  if (bad_grid(grid) || np < 0 || io < 0) return BAD;
  hipLaunchKernelGGL(lz_final, dim3(grid), dim3(256), 0, nullptr, partial, np, scal, io, op);
  return finish();
}

// probes: m HOST-side entries, each a device pointer.  Runs lz_probe_dots<m, real> on `grid` workgroups and lz_probe_final on one.
int lkc_probe_dots(int grid, int real, int m, int64_t n, const void* x, const void* const* probes, double* d_part, double* d_out) {
  if (bad_grid(grid) || n < 0 || m < 1 || m > HXV_MAX_PROBES || !probes) return BAD;
  LzProbes pr{};
  for (int j = 0; j < m; ++j) pr.p[j] = (const double2*)probes[j];
  if (real)
    launch_probe_dots<true>(grid, nullptr, m, n, (const double2*)x, pr, d_part, d_out);
  else
    launch_probe_dots<false>(grid, nullptr, m, n, (const double2*)x, pr, d_part, d_out);
  return finish();
}

int lkc_probe_final(int grid, const double* partial, int np, int nc, double* out) {
  if (bad_grid(grid) || np < 0 || nc < 0) return BAD;
  hipLaunchKernelGGL(lz_probe_final, dim3(grid), dim3(256), 0, nullptr, partial, np, nc, out);
  return finish();
}

int lkc_scale(int grid, int64_t n, void* q, const void* w, const double* scal, int ib) {
  if (bad_grid(grid) || n < 0 || ib < 0) return BAD;
  hipLaunchKernelGGL(lz_scale, dim3(grid), dim3(256), 0, nullptr, n, (double2*)q, (const double2*)w, scal, ib);
  return finish();
}

int lkc_axpy(int grid, int64_t n, void* y, const void* q, double c) {
  if (bad_grid(grid) || n < 0) return BAD;
  hipLaunchKernelGGL(lz_axpy, dim3(grid), dim3(256), 0, nullptr, n, (double2*)y, (const double2*)q, c);
  return finish();
}

int lkc_init(int grid, int64_t n, void* q, uint64_t seed, int dimup, int pitch, int col0, const int32_t* iperm, const uint8_t* sign) {
  if (bad_grid(grid) || n < 0 || dimup < 0 || pitch < 1 || pitch < dimup || col0 < 0) return BAD;
  hipLaunchKernelGGL(lz_init, dim3(grid), dim3(256), 0, nullptr, n, (double2*)q, seed, dimup, pitch, col0, iperm, sign);
  return finish();
}

int lkc_init_real(int grid, int64_t n, double* q, uint64_t seed, int dimup, int pitch, int col0, const int32_t* iperm, const uint8_t* sign) {
  if (bad_grid(grid) || n < 0 || dimup < 0 || pitch < 1 || pitch < dimup || col0 < 0) return BAD;
  hipLaunchKernelGGL(lz_init_real, dim3(grid), dim3(256), 0, nullptr, n, q, seed, dimup, pitch, col0, iperm, sign);
  return finish();
}

int lkc_to_real(int grid, int dimup, int dimdw, int pc, int pr, const void* src, double* dst, double* partial) {
  if (bad_grid(grid) || dimup < 0 || dimdw < 0 || pc < 1 || pr < 1 || pc < dimup || pr < dimup) return BAD;
  hipLaunchKernelGGL(lz_to_real, dim3(grid), dim3(256), 0, nullptr, dimup, dimdw, pc, pr, (const double2*)src, dst, partial);
  return finish();
}

int lkc_to_complex(int grid, int dimup, int dimdw, int pc, int pr, const double* src, void* dst) {
  if (bad_grid(grid) || dimup < 0 || dimdw < 0 || pc < 1 || pr < 1 || pc < dimup || pr < dimup) return BAD;
  hipLaunchKernelGGL(lz_to_complex, dim3(grid), dim3(256), 0, nullptr, dimup, dimdw, pc, pr, src, (double2*)dst);
  return finish();
}

// the three scalar kernels: one thread of one workgroup (a second one would race on the same slots)
int lkc_mul(int grid, double* scal, int i, int a, int b) {
  if (grid != 1 || i < 0 || a < 0 || b < 0) return BAD;
  hipLaunchKernelGGL(lz_mul, dim3(1), dim3(1), 0, nullptr, scal, i, a, b);
  return finish();
}

int lkc_sqrt(int grid, double* scal, int i) {
  if (grid != 1 || i < 0) return BAD;
  hipLaunchKernelGGL(lz_sqrt, dim3(1), dim3(1), 0, nullptr, scal, i);
  return finish();
}

int lkc_next(int grid, double* scal, double* alpha_out, double* beta_out, int nmax) {
  if (grid != 1 || nmax < 0) return BAD;
  hipLaunchKernelGGL(lz_next, dim3(1), dim3(1), 0, nullptr, scal, alpha_out, beta_out, nmax);
  return finish();
}

// HOST: LzScale::next(beta) followed by c() on state = {s_cur, beta_prev} (updated in place) -> *c
void lkc_host_scale_next(double* state, double beta, double* c) {
  LzScale sc;
  sc.s_cur = state[0];
  sc.beta_prev = state[1];
  sc.next(beta);
  *c = sc.c();
  state[0] = sc.s_cur;
  state[1] = sc.beta_prev;
}

}  // extern "C"
