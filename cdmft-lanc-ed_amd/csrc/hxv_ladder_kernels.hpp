// The device code of c / c^dagger between two sectors (hxv_ladder.hip) with the launch helper of ladder_kernel: text moved out of that file
// unchanged, so that tests/device/move_kernels_check.hip can launch each kernel alone on bases, row orders, slot lists and grids of its own
// making (tests/test_gpu_move_kernels.py).
#pragma once

#include <hip/hip_runtime.h>

#include "hxv_device.hpp"

namespace {
using namespace hxv;

// ---------------------------------------------------------------------------------------
// c / c^dagger on one orbital of one spin, between two sectors (ED_GF_NORMAL.f90:180-199:
// vvinit(j) = sgn * state_cvec(i)).  One thread per TARGET element: it looks its source up.
// ---------------------------------------------------------------------------------------
// Device row order (SectorHost::up_perm; spin up only -- a dw operator leaves the row where it is): map_from is then the SORTED reference
// map of the source sector and the source row found in it goes through perm_from to its device row; the two basis signs (by device row)
// multiply the operator's own.  Null pointers = the reference's order.
__global__ void __launch_bounds__(256) ladder_kernel(const uint32_t* __restrict__ map_from, int dim_from, const uint32_t* __restrict__ map_to,
                                                    int pitch_from, int dimup_to, int pitch_to, int dimdw_to, int orbital, int spin, int create,
                                                    const double2* __restrict__ psi, double2* __restrict__ out, double2 coef,
                                                    int accumulate, const int32_t* __restrict__ perm_from, const uint8_t* __restrict__ sign_from,
                                                    const uint8_t* __restrict__ sign_to) {
  // out = (accumulate ? out : 0) + coef * c^(dagger) psi : the mixed channels of the Green's function start from
  // (c^dagger_i + c^dagger_j)|gs> and (c^dagger_i + xi c^dagger_j)|gs> (ED_GF_NORMAL.f90:370-406, 746-780)
  const int64_t n = (int64_t)dimup_to * dimdw_to;
  const uint32_t bit = 1u << orbital;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(t / dimup_to), i = (int)(t - (int64_t)c * dimup_to);
    const uint32_t m_to = map_to[spin == 0 ? i : c];
    double2 r = make_double2(0.0, 0.0);
    // the target must have the orbital occupied after a creation / empty after a destruction
    if (((m_to & bit) != 0u) == (create != 0)) {
      const uint32_t m_from = m_to ^ bit;
      int j = rank_in_map(map_from, dim_from, m_from);
      int neg = par_below(m_from, orbital);
      if (spin == 0) {
        if (perm_from) j = perm_from[j];
        if (sign_from) neg ^= (int)sign_from[j];
        if (sign_to) neg ^= (int)sign_to[i];
      }
      const double sg = neg ? -1.0 : 1.0;
      const double2 x = spin == 0 ? psi[(int64_t)c * pitch_from + j] : psi[(int64_t)j * pitch_from + i];
      r = make_double2(sg * (coef.x * x.x - coef.y * x.y), sg * (coef.x * x.y + coef.y * x.x));
    }
    if (accumulate) {
      const double2 o = out[(int64_t)c * pitch_to + i];
      r.x += o.x;
      r.y += o.y;
    }
    out[(int64_t)c * pitch_to + i] = r;
  }
}

hipError_t launch_ladder(const uint32_t* map_from, int dim_from, const uint32_t* map_to, int dim_to, int pitch_from, int dimup_to,
                         int pitch_to, int dimdw_to, int orbital, int spin, int create, const double2* psi, double2* out, hipStream_t st,
                         double2 coef, int accumulate, const int32_t* perm_from, const uint8_t* sign_from, const uint8_t* sign_to) {
  (void)dim_to;
  const int64_t n = (int64_t)dimup_to * dimdw_to;
  if (n == 0) return hipSuccess;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  hipLaunchKernelGGL(ladder_kernel, dim3((unsigned)blocks), dim3(256), 0, st, map_from, dim_from, map_to, pitch_from, dimup_to, pitch_to,
                     dimdw_to, orbital, spin, create, psi, out, coef, accumulate, perm_from, sign_from, sign_to);
  return hipGetLastError();
}

// out[c][:] = (accumulate ? out[c][:] : 0) + coef * sign[c] * src_c[:]  for the local target columns c of a spin-dw ladder operator on a
// split sector: src_c = column slot[c] of the local source slab (slot >= 0), column -1-slot[c] of the received columns (slot < 0),
// or nothing (sign[c] == 0: the target column is not reached).  Rows are untouched by a dw operator; pad rows stay as they are.
__global__ void __launch_bounds__(256) ladder_cols_kernel(int dimup, int ncols, int pitch_from, int pitch_to, const int32_t* __restrict__ slot,
                                                         const int32_t* __restrict__ sign, const double2* __restrict__ psi_local,
                                                         const double2* __restrict__ recv, double2* __restrict__ out, double2 coef, int accumulate) {
  const int c = blockIdx.x;
  if (c >= ncols) return;
  const int sg = sign[c];
  const double2* __restrict__ src = sg == 0 ? nullptr : (slot[c] >= 0 ? psi_local + (int64_t)slot[c] * pitch_from : recv + (int64_t)(-1 - slot[c]) * pitch_from);
  double2* __restrict__ dst = out + (int64_t)c * pitch_to;
  for (int i = threadIdx.x; i < dimup; i += 256) {
    double2 r = make_double2(0.0, 0.0);
    if (sg != 0) {
      const double2 x = src[i];
      r = make_double2(sg * (coef.x * x.x - coef.y * x.y), sg * (coef.x * x.y + coef.y * x.x));
    }
    if (accumulate) {
      const double2 o = dst[i];
      r.x += o.x;
      r.y += o.y;
    }
    dst[i] = r;
  }
}
}  // namespace
