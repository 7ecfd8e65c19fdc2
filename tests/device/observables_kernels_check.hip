// TEST-ONLY: the kernels of hxv_observables_accumulate (csrc/hxv_observables_kernels.hpp) behind one launcher each, so that
// tests/test_gpu_observables_kernels.py can run them alone on synthetic tables, sizes and grids no sector passes.  The kernels are the
// header's text, compiled with the engine's flags (build_observables_kernels_check() of __graft_entry__.py); this library is never linked
// into libhxv.so.
//
// Every pointer is a DEVICE pointer.  A launcher refuses (hipErrorInvalidValue) before it launches anything what no launch can take: a grid
// below 1 (the reduction: or beyond the record, whose element the workgroup index is), Nimp outside 1 .. OBS_MAX_NIMP, a negative size, a
// pitch below the rows, a needed pointer that is NULL.  The CONTENTS of the tables are the caller's contract (tests/observables_kernels_ref.py
// keeps every entry in range).  Launches go to the null stream and are waited for.
#include "hxv_observables_kernels.hpp"

namespace {
constexpr int BAD = (int)hipErrorInvalidValue;
bool bad_nimp(int nimp) { return nimp < 1 || nimp > OBS_MAX_NIMP; }
int finish() {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  return (int)e;
}
}  // namespace

extern "C" {

// c[0..2] = OBS_THREADS, OBS_WAVES, OBS_MAX_NIMP
void okc_constants(int* c) {
  c[0] = OBS_THREADS;
  c[1] = OBS_WAVES;
  c[2] = OBS_MAX_NIMP;
}

// obs_rows_kernel<pairs != 0> on `grid` workgroups; nw = 2^nimp, np = nimp^2; psi [qdw][pitch], colout [qdw][nw + 2 np]
int okc_rows(int pairs, int grid, int nimp, const void* psi, int pitch, int qdw, const int32_t* seg_ptr, const int32_t* ent_a, const int32_t* ent_b,
             const int8_t* ent_s, void* colout) {
  if (grid < 1 || bad_nimp(nimp) || pitch < 1 || qdw < 0 || !psi || !seg_ptr || !ent_a || !ent_b || !ent_s || !colout) return BAD;
  const int nw = 1 << nimp, np = nimp * nimp;
  if (pairs)
    hipLaunchKernelGGL(obs_rows_kernel<true>, dim3((unsigned)grid), dim3(OBS_THREADS), 0, nullptr, (const double2*)psi, pitch, qdw, nw, np, seg_ptr,
                       ent_a, ent_b, ent_s, (double2*)colout);
  else
    hipLaunchKernelGGL(obs_rows_kernel<false>, dim3((unsigned)grid), dim3(OBS_THREADS), 0, nullptr, (const double2*)psi, pitch, qdw, nw, np, seg_ptr,
                       ent_a, ent_b, ent_s, (double2*)colout);
  return finish();
}

// obs_rdw_kernel on `grid` workgroups; full: the column slots the pairs name (psi itself, or a gathered copy with the same pitch)
int okc_rdw(int grid, int nimp, const void* psi, const void* full, int pitch, int dimup, int qdw, const int32_t* dwp_ptr, const int32_t* dwp_slot,
            const int32_t* dwp_p, const int8_t* dwp_s, void* colout) {
  if (grid < 1 || bad_nimp(nimp) || dimup < 0 || pitch < dimup || pitch < 1 || qdw < 0 || !psi || !full || !dwp_ptr || !dwp_slot || !dwp_p || !dwp_s ||
      !colout)
    return BAD;
  hipLaunchKernelGGL(obs_rdw_kernel, dim3((unsigned)grid), dim3(OBS_THREADS), 0, nullptr, (const double2*)psi, (const double2*)full, pitch, dimup, qdw,
                     1 << nimp, nimp * nimp, dwp_ptr, dwp_slot, dwp_p, dwp_s, (double2*)colout);
  return finish();
}

// obs_reduce_kernel: workgroup o writes record element o (W) or the pair o - nw^2 (re, im), so the grid is at most nw^2 + 2 np; with no
// column (qdw = 0) colout is not read and may be NULL
int okc_reduce(int grid, int nimp, const void* colout, int qdw, const int32_t* dwbin_ptr, const int32_t* dwbin_cols, double* rec) {
  if (bad_nimp(nimp) || qdw < 0) return BAD;
  const int64_t nw = (int64_t)1 << nimp, np = (int64_t)nimp * nimp;
  if (grid < 1 || grid > nw * nw + 2 * np || (!colout && qdw > 0) || !dwbin_ptr || !dwbin_cols || !rec) return BAD;
  hipLaunchKernelGGL(obs_reduce_kernel, dim3((unsigned)grid), dim3(OBS_THREADS), 0, nullptr, (const double2*)colout, qdw, nimp, (int)nw, (int)np,
                     dwbin_ptr, dwbin_cols, rec);
  return finish();
}

}  // extern "C"
