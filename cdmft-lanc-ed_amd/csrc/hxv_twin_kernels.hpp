// The device code of the twin-sector map (hxv_twin.hip): text moved out of that file unchanged, so that tests/device/move_kernels_check.hip
// can launch each kernel alone on row orders, splits and grids of its own making (tests/test_gpu_move_kernels.py).  What the kernels promise
// is stated at the head of hxv_twin.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {
constexpr int TW = 32;            // tile edge, device rows of A and of B
constexpr int TW_THREADS = 256;   // TW lanes along a run, TW_THREADS / TW runs per trip
// LDS tile [TW rows of B][TW rows of A], one 16-byte element of padding per row (row stride 33 slots of 16 bytes).  Designed conflict count: 0
// both ways.  The row-wise ds_write_b128 is served in groups of 8 consecutive lanes, banks (a/4) mod 32: 8 consecutive slots of one tile row
// are 128 contiguous bytes, every bank once.  The column-wise ds_read_b128 is served in four groups of 16 lanes ({0-3,12-15,20-27}, {4-11,
// 16-19,28-31} and the same + 32), banks (a/4) mod 64, i.e. slot mod 16: lane l of a half wave reads slot 33*l + c, = l + c mod 16, and the
// lanes of every group take every residue mod 16 once.
constexpr int TW_STRIDE = TW + 1;

// grid: x = tiles along A's device rows, y = tiles along B's device rows (C5: 1520 x 1520)
__global__ void __launch_bounds__(TW_THREADS) twin_transpose_kernel(const double2* __restrict__ d_a, int dimup_a, int pitch_a,
                                                                    const int32_t* __restrict__ iperm_a, const uint8_t* __restrict__ sign_a,
                                                                    double2* __restrict__ d_b, int dimup_b, int pitch_b,
                                                                    const int32_t* __restrict__ iperm_b, const uint8_t* __restrict__ sign_b) {
  __shared__ double2 tile[TW * TW_STRIDE];
  const int tx = threadIdx.x % TW, ty = threadIdx.x / TW;
  const int ra0 = blockIdx.x * TW, rb0 = blockIdx.y * TW;
  // load: lane tx along A's rows, one run per (ty, trip) = one row of B = one column of A
  {
    const int ra = ra0 + tx;
    const bool in_a = ra < dimup_a;
    const bool neg_a = in_a && sign_a && sign_a[ra];
#pragma unroll
    for (int j = 0; j < TW; j += TW_THREADS / TW) {
      const int rb = rb0 + ty + j;
      double2 x = make_double2(0.0, 0.0);
      if (in_a && rb < dimup_b) {
        const int64_t ka = iperm_b ? iperm_b[rb] : rb;
        x = d_a[ka * pitch_a + ra];
        if (neg_a != (sign_b && sign_b[rb])) x = make_double2(-x.x, -x.y);
      }
      tile[(ty + j) * TW_STRIDE + tx] = x;
    }
  }
  __syncthreads();
  // store: lane tx along B's rows, one run per (ty, trip) = one row of A = one column of B; rows of B past DimUp_B hold the zeros loaded above
  {
    const int rb = rb0 + tx;
    if (rb < pitch_b) {
#pragma unroll
      for (int j = 0; j < TW; j += TW_THREADS / TW) {
        const int ra = ra0 + ty + j;
        if (ra < dimup_a) {
          const int64_t kb = iperm_a ? iperm_a[ra] : ra;
          d_b[kb * pitch_b + rb] = tile[tx * TW_STRIDE + ty + j];
        }
      }
    }
  }
}

// grid: x = tiles along A's device rows, y = tiles along this rank's qa columns of A (looped when there are more tiles than blocks).
// send: [DimUp_A rows by reference row][stride]; own: this rank's block in its receive buffer, reference rows [own_lo, own_hi)
__global__ void __launch_bounds__(TW_THREADS) twin_pack_kernel(const double2* __restrict__ d_a, int dimup_a, int pitch_a, int qa,
                                                               const int32_t* __restrict__ iperm_a, const uint8_t* __restrict__ sign_a,
                                                               double2* __restrict__ send, double2* __restrict__ own, int stride, int own_lo, int own_hi) {
  __shared__ double2 tile[TW * TW_STRIDE];
  const int tx = threadIdx.x % TW, ty = threadIdx.x / TW;
  const int ra0 = blockIdx.x * TW;
  for (int c0 = blockIdx.y * TW; c0 < qa; c0 += gridDim.y * TW) {
    // load: lane tx along A's rows, one run per (ty, trip) = one local column of A
    {
      const int ra = ra0 + tx;
      const bool in_a = ra < dimup_a;
      const bool neg_a = in_a && sign_a && sign_a[ra];
#pragma unroll
      for (int j = 0; j < TW; j += TW_THREADS / TW) {
        const int c = c0 + ty + j;
        double2 x = make_double2(0.0, 0.0);
        if (in_a && c < qa) {
          x = d_a[(int64_t)c * pitch_a + ra];
          if (neg_a) x = make_double2(-x.x, -x.y);
        }
        tile[(ty + j) * TW_STRIDE + tx] = x;
      }
    }
    __syncthreads();
    // store: lane tx along the local columns, one run per (ty, trip) = one row of A = one block row
    {
      const int c = c0 + tx;
      if (c < qa) {
#pragma unroll
        for (int j = 0; j < TW; j += TW_THREADS / TW) {
          const int ra = ra0 + ty + j;
          if (ra < dimup_a) {
            const int iup = iperm_a ? iperm_a[ra] : ra;
            double2* dst = (iup >= own_lo && iup < own_hi) ? own + (int64_t)(iup - own_lo) * stride : send + (int64_t)iup * stride;
            dst[c] = tile[tx * TW_STRIDE + ty + j];
          }
        }
      }
    }
    __syncthreads();  // (the next trip overwrites the tile)
  }
}

// grid: x = blocks of TW_THREADS device rows of B up to the pitch, y = this rank's qb columns of B (looped beyond the grid limit).
// tab: [P+1] first column of A per rank, [P+1] element offset of the block from each rank in recv, [P] row stride of that block
__global__ void __launch_bounds__(TW_THREADS) twin_unpack_kernel(const double2* __restrict__ recv, const int64_t* __restrict__ tab, int nranks,
                                                                 double2* __restrict__ d_b, int dimup_b, int pitch_b, int qb,
                                                                 const int32_t* __restrict__ iperm_b, const uint8_t* __restrict__ sign_b) {
  const int rb = blockIdx.x * TW_THREADS + threadIdx.x;
  if (rb >= pitch_b) return;
  const bool in_b = rb < dimup_b;
  int64_t off = 0, st = 0;
  bool neg_b = false;
  if (in_b) {
    const int64_t idw = iperm_b ? iperm_b[rb] : rb;
    int o = 0;
    for (int p = 1; p < nranks; ++p) o += idw >= tab[p] ? 1 : 0;
    off = tab[nranks + 1 + o] + idw - tab[o];
    st = tab[2 * nranks + 2 + o];
    neg_b = sign_b && sign_b[rb];
  }
  for (int kb = blockIdx.y; kb < qb; kb += gridDim.y) {
    double2 x = make_double2(0.0, 0.0);
    if (in_b) {
      x = recv[off + (int64_t)kb * st];
      if (neg_b) x = make_double2(-x.x, -x.y);
    }
    d_b[(int64_t)kb * pitch_b + rb] = x;
  }
}
}  // namespace
