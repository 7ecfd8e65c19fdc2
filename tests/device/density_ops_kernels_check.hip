// TEST-ONLY: the kernels of hxv_apply_density_ops (csrc/hxv_density_ops_kernels.hpp) behind one launcher each, so that
// tests/test_gpu_density_ops_kernels.py can run them alone on synthetic tables, sizes, chunkings and grids no sector passes.  The kernels are
// the header's text, compiled with the engine's flags (build_density_ops_kernels_check() of __graft_entry__.py); this library is never
// linked into libhxv.so.
//
// psi, occ_up, occ_dw, coef, partial, sums and the output vectors are DEVICE pointers; the list of output pointers and the means are host
// arrays of nops entries (the launcher leaves out.v[a], a >= nops, NULL).  A launcher refuses (hipErrorInvalidValue) before it launches
// anything what no launch can take: a grid below 1 (the reduction: or beyond DOP_NSUM, whose sum the workgroup index is), Nimp outside
// 1 .. DOP_MAX_NIMP, nops outside 1 .. DOP_MAX, a negative size, a pitch below the rows or not a multiple of 8, a chunk that is not a
// positive multiple of 8 rows, a needed pointer that is NULL.  Launches go to the null stream and are waited for.
#include "hxv_density_host.hpp"
#include "hxv_density_ops_kernels.hpp"

using namespace hxv;

namespace {
constexpr int BAD = (int)hipErrorInvalidValue;
bool bad_shape(int grid, int dimup, int pitch, int qdw, int nimp, int nops, int nchunk, int rows) {
  return grid < 1 || dimup < 1 || pitch < dimup || pitch % 8 != 0 || qdw < 0 || nimp < 1 || nimp > DOP_MAX_NIMP || nops < 1 || nops > DOP_MAX ||
         nchunk < 1 || rows < 8 || rows % 8 != 0 || (int64_t)qdw * nchunk >= INT32_MAX;
}
int finish() {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  return (int)e;
}
}  // namespace

extern "C" {

// c[0..6] = DOP_THREADS, DOP_MAX, DOP_NSUM, DOP_MAX_NIMP, DOP_UNROLL, DOP_CHUNK, DOP_WG_PER_CU
void dkc_constants(int* c) {
  c[0] = DOP_THREADS;
  c[1] = DOP_MAX;
  c[2] = DOP_NSUM;
  c[3] = DOP_MAX_NIMP;
  c[4] = DOP_UNROLL;
  c[5] = DOP_CHUNK;
  c[6] = DOP_WG_PER_CU;
}

// pass 1 on `grid` workgroups: partial [grid][DOP_NSUM]
int dkc_sums(int grid, int dimup, int pitch, int qdw, int nimp, int nops, int nchunk, int rows, const void* psi, const uint32_t* occ_up,
             const uint32_t* occ_dw, const double* coef, double* partial) {
  if (bad_shape(grid, dimup, pitch, qdw, nimp, nops, nchunk, rows) || !psi || !occ_up || !occ_dw || !coef || !partial) return BAD;
  const DopShape s{dimup, pitch, qdw, nimp, nops, nchunk, rows, (int64_t)qdw * nchunk};
  hipLaunchKernelGGL(dop_sums_kernel, dim3((unsigned)grid), dim3(DOP_THREADS), 0, nullptr, (const double2*)psi, occ_up, occ_dw, coef, s, partial);
  return finish();
}

// pass 2 on `grid` workgroups: outs[a] [qdw][pitch] for a < nops, m[a] what is subtracted from f_a; partial [grid][DOP_NSUM]
int dkc_apply(int grid, int dimup, int pitch, int qdw, int nimp, int nops, int nchunk, int rows, const void* psi, const uint32_t* occ_up,
              const uint32_t* occ_dw, const double* coef, void* const* outs, const double* m, double* partial) {
  if (bad_shape(grid, dimup, pitch, qdw, nimp, nops, nchunk, rows) || !psi || !occ_up || !occ_dw || !coef || !outs || !m || !partial) return BAD;
  DopOut out{};
  for (int a = 0; a < nops; ++a) {
    if (!outs[a] || outs[a] == psi) return BAD;
    out.v[a] = (double2*)outs[a];
    out.m[a] = m[a];
  }
  const DopShape s{dimup, pitch, qdw, nimp, nops, nchunk, rows, (int64_t)qdw * nchunk};
  hipLaunchKernelGGL(dop_apply_kernel, dim3((unsigned)grid), dim3(DOP_THREADS), 0, nullptr, (const double2*)psi, occ_up, occ_dw, coef, s, out, partial);
  return finish();
}

// the reduction: workgroup v writes sums[v] from column v of partial [nblocks][DOP_NSUM] (column DOP_MAX for v == norm_at)
int dkc_reduce(int grid, int nblocks, int norm_at, const double* partial, double* sums) {
  if (grid < 1 || grid > DOP_NSUM || nblocks < 0 || norm_at < -1 || norm_at > DOP_MAX || (!partial && nblocks > 0) || !sums) return BAD;
  hipLaunchKernelGGL(dop_reduce_kernel, dim3((unsigned)grid), dim3(DOP_THREADS), 0, nullptr, partial, nblocks, norm_at, sums);
  return finish();
}

}  // extern "C"
