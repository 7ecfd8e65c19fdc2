// TEST-ONLY: one launcher per streaming kernel of hxv_eigh_lowest, so that tests/test_gpu_eigh_kernels.py can run each kernel alone and
// compare it with an exact sum (tests/eigh_kernels_ref.py).  The kernels are the text of csrc/hxv_eigh_kernels.hpp, compiled with the
// engine's flags (build_eigh_kernels_check() of __graft_entry__.py); this library is never linked into libhxv.so.
//
// Every entry takes device pointers and the kernel's own arguments unchanged, with the grid in front; it launches on the null stream,
// waits, and returns the HIP status.  The two rotations go through launch_rotate / launch_rotate_dots, so the dispatch on m is under
// test.  Arguments beyond what a kernel's fixed-size tables hold are refused (hipErrorInvalidValue) before anything is launched.
#include "hxv_eigh_kernels.hpp"

namespace {

int finish() {
  hipError_t e = hipGetLastError();
  hipError_t s = hipStreamSynchronize(nullptr);
  return (int)(e != hipSuccess ? e : s);
}

constexpr int BAD = (int)hipErrorInvalidValue;

}  // namespace

extern "C" {

// out[0..3] = JB, TR_BLOCKS, MAXCV, FUSE_NJ
void ekc_constants(int* out) {
  out[0] = JB;
  out[1] = TR_BLOCKS;
  out[2] = MAXCV;
  out[3] = FUSE_NJ;
}

int ekc_mdot(int grid, int64_t n, const void* V, int64_t stride, int nb, const void* w, double* partial) {
  if (grid < 1 || n < 0 || nb < 0 || nb > JB) return BAD;
  hipLaunchKernelGGL(tr_mdot, dim3(grid), dim3(256), 0, nullptr, n, (const double2*)V, stride, nb, (const double2*)w, partial);
  return finish();
}

int ekc_colsum(int grid, const double* partial, int nblocks, int ld, int nval, double* out, int zero_odd) {
  if (grid < 1 || nblocks < 0 || nval < 0 || nval > ld) return BAD;
  hipLaunchKernelGGL(tr_colsum, dim3(grid), dim3(256), 0, nullptr, partial, nblocks, ld, nval, out, zero_odd);
  return finish();
}

int ekc_maxpy(int grid, int64_t n, const void* V, int64_t stride, int nj, const int* idx, const double* coef, void* w, double* partial) {
  if (grid < 1 || n < 0 || nj < 0 || nj > MAXCV + 1) return BAD;
  hipLaunchKernelGGL(tr_maxpy, dim3(grid), dim3(256), 0, nullptr, n, (const double2*)V, stride, nj, idx, coef, (double2*)w, partial);
  return finish();
}

int ekc_scale_nrm(int grid, int64_t n, void* x, double r, double* partial) {
  if (grid < 1 || n < 0) return BAD;
  hipLaunchKernelGGL(tr_scale_nrm, dim3(grid), dim3(256), 0, nullptr, n, (double2*)x, r, partial);
  return finish();
}

int ekc_rotate(int grid, int64_t n, void* V, int64_t stride, int m, int k, const double* S) {
  if (grid < 1 || n < 0 || m < 1 || m > MAXCV || k < 0 || k > m) return BAD;
  launch_rotate(grid, nullptr, n, (double2*)V, stride, m, k, S);
  return finish();
}

// *launched = what launch_rotate_dots returned (false: k > FUSE_NJ, nothing was launched)
int ekc_rotate_dots(int grid, int64_t n, void* V, int64_t stride, int m, int k, const double* S, double* partial, int* launched) {
  if (grid < 1 || n < 0 || m < 1 || m > MAXCV || k < 0 || k > m) return BAD;
  *launched = launch_rotate_dots(grid, nullptr, n, (double2*)V, stride, m, k, S, partial) ? 1 : 0;
  return finish();
}

int ekc_axpy_mdot(int grid, int64_t n, const void* V, int64_t stride, int nv, const double* coef, double a, void* w, double* partial) {
  if (grid < 1 || n < 0 || nv < 0 || nv > FUSE_NJ) return BAD;
  hipLaunchKernelGGL((tr_axpy_mdot<FUSE_NJ>), dim3(grid), dim3(256), 0, nullptr, n, (const double2*)V, stride, nv, coef, a, (double2*)w, partial);
  return finish();
}

}  // extern "C"
