// HIP kernels (gfx950) for the sector product  Hv = D.v + H_up v + v H_dw^T  on the
// DimUp x DimDw layout (up index fastest), complex fp64.
//
// Reference semantics: ED_HAMILTONIAN_SPARSE_HxV.f90:167-227 (serial) / :230-315 (MPI slab).
// No MFMA: the path is a sparse gather over a 2.65 GB vector, bound by HBM and by on-chip
// gather bandwidth.
#include <algorithm>

#include "hxv_device.hpp"
#include "hxv_tile_dev.hpp"

namespace hxv {

// ---------------------------------------------------------------------------------------
// Variant 0: one thread per output element, every gather straight from global memory.
// The simplest correct statement of the product; kept as the on-device cross-check of the
// tiled kernels and for tiny sectors.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) hxv_naive_kernel(DevSector s, const double2* __restrict__ v, double2* __restrict__ hv) {
  const int64_t nloc = (int64_t)s.qdw * s.dimup;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nloc; t += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(t / s.dimup);
    const int i = (int)(t - (int64_t)cl * s.dimup);
    const int c = cl + s.dw0;
    const double2* __restrict__ vcol = v + (int64_t)(s.slab0 + cl) * s.pitch;
    const double d = diag_at(s.diag, i, c, t);
    const double2 x = vcol[i];
    double2 acc = make_double2(d * x.x, d * x.y);
    for (int k = 0; k < s.up.K; ++k) {
      const uint32_t e = s.up.ell[(int64_t)k * s.up.dim + i];
      if (e == ELL_EMPTY) break;
      cfma(acc, ell_coef(s.up.coef, e), vcol[e & ELL_SRC_MASK]);
    }
    for (int k = 0; k < s.dw.K; ++k) {
      const uint32_t e = s.dw.ell[(int64_t)k * s.dw.dim + c];
      if (e == ELL_EMPTY) break;
      cfma(acc, ell_coef(s.dw.coef, e), v[(int64_t)(e & ELL_SRC_MASK) * s.pitch + i]);
    }
    hv[(int64_t)cl * s.pitch + i] = acc;
  }
}

hipError_t launch_hxv_naive(const DevSector& s, const double2* v_full, double2* hv_local, hipStream_t st) {
  const int64_t nloc = (int64_t)s.qdw * s.dimup;
  if (nloc == 0) return hipSuccess;
  int64_t blocks = (nloc + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  hipLaunchKernelGGL(hxv_naive_kernel, dim3((unsigned)blocks), dim3(256), 0, st, s, v_full, hv_local);
  return hipGetLastError();
}

}  // namespace hxv

// hxv_nonlocal_kernel, hxv_nonlocal_tab and hxv_nonlocal_csr, the three kernels of the spH0nd block, and between the second and the third
// (the header includes hxv_move_kernels.hpp there) pack_columns_kernel and add_pieces_kernel; included here, where the text of the first
// stood, so that the file's device code keeps its order
#include "hxv_nonlocal_kernels.hpp"

namespace hxv {

hipError_t launch_pack_columns(const double2* d_in, double2* d_out, const int32_t* d_cols, int ncols, int pitch, hipStream_t st) {
  if (ncols <= 0) return hipSuccess;
  hipLaunchKernelGGL(pack_columns_kernel, dim3((unsigned)ncols), dim3(256), 0, st, d_in, d_out, d_cols, pitch);
  return hipGetLastError();
}

hipError_t launch_add_pieces(void* hv, const WtRange* wtr, int nwtr, int dimup, int pitch, int ncols, bool real, hipStream_t st) {
  if (ncols <= 0) return hipSuccess;
  const dim3 grid((unsigned)std::min((dimup + 255) / 256, 64), (unsigned)std::min(ncols, 65535));   // (the kernel loops over the columns past the grid)
  if (real)
    hipLaunchKernelGGL(add_pieces_kernel<double>, grid, dim3(256), 0, st, (double*)hv, wtr, nwtr, dimup, pitch, ncols);
  else
    hipLaunchKernelGGL(add_pieces_kernel<double2>, grid, dim3(256), 0, st, (double2*)hv, wtr, nwtr, dimup, pitch, ncols);
  return hipGetLastError();
}

hipError_t launch_hxv_nonlocal(const DevSector& s, const double2* v_full, double2* hv_local, hipStream_t st) {
  const int64_t nloc = (int64_t)s.qdw * s.dimup;
  if (nloc == 0 || !s.nd.active) return hipSuccess;
  if (s.ndcsr_rowptr) {
    int64_t blocks = std::min<int64_t>((nloc + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(hxv_nonlocal_csr, dim3((unsigned)blocks), dim3(256), 0, st, s, v_full, hv_local);
    return hipGetLastError();
  }
  if (s.nd_up && s.nd_dw) {
    const int rchunks = (s.dimup + 1023) / 1024;
    hipLaunchKernelGGL(hxv_nonlocal_tab, dim3((unsigned)((int64_t)s.qdw * rchunks)), dim3(1024), 0, st, s, v_full, hv_local, rchunks);
    return hipGetLastError();
  }
  int64_t blocks = (nloc + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  hipLaunchKernelGGL(hxv_nonlocal_kernel, dim3((unsigned)blocks), dim3(256), 0, st, s, v_full, hv_local);
  return hipGetLastError();
}

}  // namespace hxv
