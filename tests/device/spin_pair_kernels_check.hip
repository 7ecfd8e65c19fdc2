// TEST-ONLY: the two kernels of hxv_apply_spin_pair (csrc/hxv_spin_pair_kernels.hpp) behind one launcher, so that
// tests/test_gpu_spin_pair_kernels.py can run them alone on synthetic tables, sizes and grids no sector passes.  The kernels are the header's
// text, compiled with the engine's flags (build_spin_pair_kernels_check() of __graft_entry__.py); this library is never linked into libhxv.so.
//
// The tables come as HOST arrays: the launcher refuses (hipErrorInvalidValue) whatever could make the kernel reach outside what it was
// given -- a dimension below 1, a pitch below its dimension or not a multiple of 8, an empty or oversized grid, a term that names a table
// that is not there, a table entry that is neither -1 nor a source inside the source vector -- and only then uploads them and launches on
// the null stream.
#include "hxv_spin_pair_kernels.hpp"

#include <vector>

using namespace hxv;

namespace {
constexpr int BAD = (int)hipErrorInvalidValue;
bool bad_pitch(int pitch, int dim) { return dim < 1 || pitch < dim || pitch % 8 != 0; }
bool bad_table(const int32_t* tab, int64_t n, int dim_from) {
  for (int64_t k = 0; k < n; ++k)
    if (tab[k] != -1 && (tab[k] & 0x7FFFFFFF) >= dim_from) return true;
  return false;
}
}  // namespace

extern "C" {

int spk_threads() { return SP_THREADS; }
int spk_max_grid() { return SP_MAX_GRID; }
int spk_max_terms() { return SP_MAX_TERMS; }
int spk_grid(int pitch_to, int dimdw_to) { return spin_pair_grid(pitch_to, dimdw_to); }

// h_up: [n_up][dimup_to], h_dw: [n_dw][dimdw_to] host tables; psi: device, [dimdw_from][pitch_from]; out: device, [dimdw_to][pitch_to];
// coef: [nterms] complex interleaved; *norm2: <out|out> as the second kernel leaves it
int spk_run(int grid, int nterms, int nuq, const uint8_t* uq_tab, const uint8_t* t_uq, const uint8_t* t_dw, const double* coef, const int32_t* h_up,
            int n_up, const int32_t* h_dw, int n_dw, int dimup_to, int pitch_to, int dimdw_to, int dimup_from, int pitch_from, int dimdw_from,
            const void* psi, void* out, double* norm2) {
  if (grid < 1 || grid > SP_MAX_GRID || nterms < 1 || nterms > SP_MAX_TERMS || nuq < 1 || nuq > nterms || n_up < 1 || n_dw < 1 || n_up > 256 || n_dw > 256 ||
      dimdw_to < 1 || dimdw_from < 1 || bad_pitch(pitch_to, dimup_to) || bad_pitch(pitch_from, dimup_from) || !uq_tab || !t_uq || !t_dw || !coef || !h_up ||
      !h_dw || !psi || !out || !norm2)
    return BAD;
  SpTerms tm{};
  tm.nterms = nterms;
  tm.nuq = nuq;
  for (int u = 0; u < nuq; ++u) {
    if (uq_tab[u] >= n_up) return BAD;
    tm.uq_tab[u] = uq_tab[u];
  }
  for (int t = 0; t < nterms; ++t) {
    if (t_uq[t] >= nuq || t_dw[t] >= n_dw) return BAD;
    tm.t_uq[t] = t_uq[t];
    tm.t_dw[t] = t_dw[t];
    tm.coef[t] = make_double2(coef[2 * t], coef[2 * t + 1]);
  }
  if (bad_table(h_up, (int64_t)n_up * dimup_to, dimup_from) || bad_table(h_dw, (int64_t)n_dw * dimdw_to, dimdw_from)) return BAD;
  const size_t bu = (size_t)n_up * dimup_to * sizeof(int32_t), bd = (size_t)n_dw * dimdw_to * sizeof(int32_t);
  char* base = nullptr;
  const size_t off_dw = (bu + 255) & ~(size_t)255, off_part = (off_dw + bd + 255) & ~(size_t)255;
  hipError_t e = hipMalloc((void**)&base, off_part + ((size_t)grid + 1) * sizeof(double));
  if (e != hipSuccess) return (int)e;
  e = hipMemcpy(base, h_up, bu, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(base + off_dw, h_dw, bd, hipMemcpyHostToDevice);
  double* d_part = (double*)(base + off_part);
  if (e == hipSuccess)
    e = launch_spin_pair(tm, grid, (const int32_t*)base, dimup_to, (const int32_t*)(base + off_dw), dimdw_to, dimup_to, pitch_to, dimdw_to, pitch_from,
                         (const double2*)psi, (double2*)out, d_part, d_part + grid, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e == hipSuccess) e = hipMemcpy(norm2, d_part + grid, sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(base);
  return (int)e;
}

}  // extern "C"
