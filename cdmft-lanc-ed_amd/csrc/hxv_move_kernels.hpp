// The two copy-and-add kernels of the slab exchanges (hxv_kernels.hip): text moved out of that file unchanged, so that
// tests/device/move_kernels_check.hip can launch each alone on column lists, row ranges and grids of its own making
// (tests/test_gpu_move_kernels.py).  Their launch helpers launch_pack_columns and launch_add_pieces have external linkage (hxv_internal.hpp)
// and stay in hxv_kernels.hip: a header would define them once per including file.
#pragma once

#include <hip/hip_runtime.h>

#include "hxv_tile_dev.hpp"

namespace hxv {

// out[b][:] = in[cols[b]][:] for the ncols = gridDim.x listed columns, whole columns of `pitch` elements (pad rows included)
__global__ void __launch_bounds__(256) pack_columns_kernel(const double2* __restrict__ in, double2* __restrict__ out, const int32_t* __restrict__ cols,
                                                          int pitch) {
  const double2* __restrict__ src = in + (int64_t)cols[blockIdx.x] * pitch;
  double2* __restrict__ dst = out + (int64_t)blockIdx.x * pitch;
  for (int i = threadIdx.x; i < pitch; i += 256) dst[i] = src[i];
}

// hv += the dw part, read where the second transpose of exchange mode 2 left it (one block per rank of origin, WtRange): the last step of
// the OVERLAPPED form of that exchange, where diagonal + up hops ran on a second stream while the transposes were under way.
// The blocks along y loop over the ncols local columns: a grid holds at most 65535 blocks along y, a skinny sector keeps more columns.
template <typename VT>
__global__ void __launch_bounds__(256) add_pieces_kernel(VT* __restrict__ hv, const WtRange* __restrict__ wtr, int nwtr, int dimup, int pitch, int ncols) {
  for (int row = blockIdx.x * 256 + threadIdx.x; row < dimup; row += gridDim.x * 256) {
    int k = 0;
    while (k + 1 < nwtr && row >= wtr[k].row1) ++k;
    for (int c = blockIdx.y; c < ncols; c += gridDim.y) {
      const VT* __restrict__ src = reinterpret_cast<const VT*>(wtr[k].base) + (int64_t)c * wtr[k].stride + (row - wtr[k].row0);
      VT a = hv[(int64_t)c * pitch + row];
      vadd(a, *src);
      hv[(int64_t)c * pitch + row] = a;
    }
  }
}

}  // namespace hxv
