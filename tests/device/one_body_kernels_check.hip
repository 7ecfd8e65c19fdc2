// TEST-ONLY: the kernels of hxv_apply_one_body (csrc/hxv_one_body_kernels.hpp) behind two launchers, so that
// tests/test_gpu_one_body_kernels.py can run them alone on synthetic tables, sizes and grids no sector passes.  The kernels are the header's
// text, compiled with the engine's flags (build_one_body_kernels_check() of __graft_entry__.py); this library is never linked into libhxv.so.
//
// The tables come as HOST arrays: the launcher refuses (hipErrorInvalidValue) whatever could make a kernel reach outside what it was given
// -- a dimension below 1, a pitch below its dimension or not a multiple of 8, an empty or oversized grid, a term that names a table that is
// not there, a table entry that is neither -1 nor a source inside the vector -- and only then uploads them and launches on the null stream.
#include "hxv_one_body_kernels.hpp"

#include <vector>

using namespace hxv;

namespace {
constexpr int BAD = (int)hipErrorInvalidValue;
bool bad_shape(int grid, int dimup, int pitch, int dimdw) {
  return grid < 1 || grid > OB_MAX_GRID || dimup < 1 || dimdw < 1 || pitch < dimup || pitch % 8 != 0;
}
bool bad_table(const int32_t* tab, int64_t n, int dim) {
  for (int64_t k = 0; k < n; ++k)
    if (tab[k] != -1 && (tab[k] & 0x7FFFFFFF) >= dim) return true;
  return false;
}
}  // namespace

extern "C" {

int obk_threads() { return OB_THREADS; }
int obk_max_grid() { return OB_MAX_GRID; }
int obk_max_terms() { return OB_MAX_TERMS; }
int obk_grid(int pitch, int dimdw) { return one_body_grid(pitch, dimdw); }

// the gather pass and its sums.  t_spin[nterms]: 0 = up term, 1 = dw term; t_tab[nterms]: which table of h_up ([n_up][dimup]) or h_dw
// ([n_dw][dimdw]); coef: [nterms] complex interleaved; psi, out: device, [dimdw][pitch]; sums[4]: <psi|psi>, Re <psi|out>, Im <psi|out>,
// <out|out> as the second kernel leaves them.  The distinct up tables are taken in order of first appearance, as the engine does.
int obk_run(int grid, int nterms, const uint8_t* t_spin, const uint8_t* t_tab, const double* coef, const int32_t* h_up, int n_up, const int32_t* h_dw,
            int n_dw, int dimup, int pitch, int dimdw, const void* psi, void* out, double* sums) {
  if (bad_shape(grid, dimup, pitch, dimdw) || nterms < 1 || nterms > OB_MAX_TERMS || n_up < 1 || n_dw < 1 || n_up > 256 || n_dw > 256 || !t_spin ||
      !t_tab || !coef || !h_up || !h_dw || !psi || !out || !sums || psi == out)
    return BAD;
  for (int t = 0; t < nterms; ++t)
    if (t_spin[t] > 1 || t_tab[t] >= (t_spin[t] ? n_dw : n_up)) return BAD;
  if (bad_table(h_up, (int64_t)n_up * dimup, dimup) || bad_table(h_dw, (int64_t)n_dw * dimdw, dimdw)) return BAD;
  const size_t bu = (size_t)n_up * dimup * sizeof(int32_t), bd = (size_t)n_dw * dimdw * sizeof(int32_t);
  char* base = nullptr;
  const size_t off_dw = (bu + 255) & ~(size_t)255, off_part = (off_dw + bd + 255) & ~(size_t)255;
  hipError_t e = hipMalloc((void**)&base, off_part + ((size_t)OB_NSUM * grid + OB_NSUM) * sizeof(double));
  if (e != hipSuccess) return (int)e;
  const int32_t *d_up = (const int32_t*)base, *d_dw = (const int32_t*)(base + off_dw);
  ObTerms tm{};
  tm.nterms = nterms;
  int uq_of[256];
  for (int k = 0; k < n_up; ++k) uq_of[k] = -1;
  for (int t = 0; t < nterms; ++t) {
    tm.coef[t] = make_double2(coef[2 * t], coef[2 * t + 1]);
    if (t_spin[t]) {
      tm.dw_tab[t] = d_dw + (size_t)t_tab[t] * dimdw;
      continue;
    }
    if (uq_of[t_tab[t]] < 0) {
      uq_of[t_tab[t]] = tm.nuq;
      tm.uq_tab[tm.nuq++] = d_up + (size_t)t_tab[t] * dimup;
    }
    tm.t_uq[t] = (uint8_t)uq_of[t_tab[t]];
  }
  e = hipMemcpy(base, h_up, bu, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(base + off_dw, h_dw, bd, hipMemcpyHostToDevice);
  double* d_part = (double*)(base + off_part);
  if (e == hipSuccess)
    e = launch_one_body(tm, grid, dimup, pitch, dimdw, (const double2*)psi, (double2*)out, d_part, d_part + (size_t)OB_NSUM * grid, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e == hipSuccess) e = hipMemcpy(sums, d_part + (size_t)OB_NSUM * grid, OB_NSUM * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(base);
  return (int)e;
}

// the mean-subtraction pass and its sum: out -= (m_re + i m_im) psi on the rows below dimup, *norm2 = <out|out> afterwards
int obk_shift(int grid, double m_re, double m_im, int dimup, int pitch, int dimdw, const void* psi, void* out, double* norm2) {
  if (bad_shape(grid, dimup, pitch, dimdw) || !psi || !out || !norm2 || psi == out) return BAD;
  double* d_part = nullptr;
  hipError_t e = hipMalloc((void**)&d_part, ((size_t)grid + 1) * sizeof(double));
  if (e != hipSuccess) return (int)e;
  e = launch_one_body_shift(make_double2(m_re, m_im), grid, dimup, pitch, dimdw, (const double2*)psi, (double2*)out, d_part, d_part + grid, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e == hipSuccess) e = hipMemcpy(norm2, d_part + grid, sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(d_part);
  return (int)e;
}

}  // extern "C"
