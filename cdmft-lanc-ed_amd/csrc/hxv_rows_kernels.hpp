// The two kernels that carry a vector between the reference's row order and a sector's device row order (hxv_capi.hip: slab_from_host,
// slab_to_host): text moved out of that file unchanged, so that tests/device/move_kernels_check.hip can launch each alone on permutations,
// signs and grids of its own making (tests/test_gpu_move_kernels.py).  Every test that uploads a vector in a device row order judges the
// other kernels through these two.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace hxv {
namespace {
// contiguous reference layout [ncols][dimup] -> device layout [ncols][pitch]: device row d holds reference row iperm[d], times the basis sign
__global__ void __launch_bounds__(256) rows_ref_to_dev(const double2* __restrict__ src, double2* __restrict__ dst, const int32_t* __restrict__ iperm,
                                                       const uint8_t* __restrict__ sign, int dimup, int pitch, int64_t n) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const int64_t c = t / pitch;
    const int d = (int)(t - c * pitch);
    double2 x = make_double2(0.0, 0.0);   // (pad rows are zero in every device vector)
    if (d < dimup) {
      x = src[c * dimup + iperm[d]];
      if (sign[d]) x = make_double2(-x.x, -x.y);
    }
    dst[t] = x;
  }
}
// device layout -> contiguous reference layout: reference row i sits at device row perm[i]
__global__ void __launch_bounds__(256) rows_dev_to_ref(const double2* __restrict__ src, double2* __restrict__ dst, const int32_t* __restrict__ perm,
                                                       const uint8_t* __restrict__ sign, int dimup, int pitch, int64_t n) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const int64_t c = t / dimup;
    const int i = (int)(t - c * dimup);
    const int d = perm[i];
    double2 x = src[c * pitch + d];
    if (sign[d]) x = make_double2(-x.x, -x.y);
    dst[t] = x;
  }
}
}  // namespace
}  // namespace hxv
