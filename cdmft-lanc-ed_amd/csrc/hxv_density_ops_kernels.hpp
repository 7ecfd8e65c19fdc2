// The three kernels of hxv_apply_density_ops (hxv_density_ops.hip, which says what they compute and why in this form), 256 threads, a work
// item = (local column, chunk of its rows), item i on workgroup i mod gridDim:
//   dop_sums_kernel    pass 1: per workgroup the partial sums of  f_a |psi|^2  (a < nops) and of |psi|^2
//   dop_apply_kernel   pass 2: the nops vectors (the pad rows of every column as zero) and per workgroup the partial sums of |out_a|^2
//   dop_reduce_kernel  one workgroup per sum: the workgroups' partials, strided over its threads, then a fixed-order tree
// The chunking (DopShape::nchunk, rows) and the grid are the host's (hxv_density_host.hpp: DOP_CHUNK, DOP_WG_PER_CU).
// Like hxv_chebyshev_kernels.hpp this is a header with everything in an anonymous namespace, so that tests/device/density_ops_kernels_check.hip
// can launch each kernel alone with a grid, sizes and tables the driver never passes; the product includes it from hxv_density_ops.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/hxv.h"

namespace {
constexpr int DOP_THREADS = 256;
constexpr int DOP_WAVES = DOP_THREADS / 64;
constexpr int DOP_MAX = HXV_MAX_DENSITY_OPS;
constexpr int DOP_NSUM = DOP_MAX + 1;  // partial sums a workgroup writes: one per operator slot, then (pass 1) the norm at index DOP_MAX
constexpr int DOP_UNROLL = 4;          // 16-byte loads a thread has in flight

struct DopShape {
  int dimup, pitch, qdw, nimp, nops, nchunk, rows;
  int64_t nitems;
};
struct DopOut {
  double2* v[DOP_MAX];
  double m[DOP_MAX];  // what is subtracted from f_a: the mean, or 0
};

// tab[spin][half][a][o] = sum over the bits b of o of coef[a][spin][5*half + b], orbitals in ascending order; 0 for a >= nops
__device__ __forceinline__ void dop_fill_lds(double* tab, const double* __restrict__ coef, int nimp, int nops) {
  for (int idx = threadIdx.x; idx < 4 * DOP_MAX * 32; idx += DOP_THREADS) {
    const int o = idx & 31, a = (idx >> 5) & (DOP_MAX - 1), half = (idx >> 8) & 1, spin = idx >> 9;
    double v = 0.0;
    if (a < nops)
      for (int b = 0; b < 5; ++b) {
        const int is = 5 * half + b;
        if (is < nimp && ((o >> b) & 1)) v += coef[(a * 2 + spin) * nimp + is];
      }
    tab[idx] = v;
  }
  __syncthreads();
}
__device__ __forceinline__ double dop_f(const double* tab, int spin, int a, uint32_t occ, bool hi) {
  double f = tab[((spin * 2 + 0) * DOP_MAX + a) * 32 + (occ & 31u)];
  if (hi) f += tab[((spin * 2 + 1) * DOP_MAX + a) * 32 + (occ >> 5)];
  return f;
}

// the workgroup's sums in a fixed order (xor butterfly inside a wave, then wave 0..3) -> partial[blockIdx.x][0..DOP_NSUM)
__device__ __forceinline__ void dop_block_sums(const double (&acc)[DOP_NSUM], double* red, double* __restrict__ partial) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int a = 0; a < DOP_NSUM; ++a) {
    double v = acc[a];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((tid & 63) == 0) red[(tid >> 6) * DOP_NSUM + a] = v;
  }
  __syncthreads();
  if (tid < DOP_NSUM) {
    double v = red[tid];
    for (int w = 1; w < DOP_WAVES; ++w) v += red[w * DOP_NSUM + tid];
    partial[(int64_t)blockIdx.x * DOP_NSUM + tid] = v;
  }
}

__global__ void __launch_bounds__(DOP_THREADS) dop_sums_kernel(const double2* __restrict__ psi, const uint32_t* __restrict__ occ_up,
                                                               const uint32_t* __restrict__ occ_dw, const double* __restrict__ coef, DopShape s,
                                                               double* __restrict__ partial) {
  __shared__ double tab[4 * DOP_MAX * 32];
  __shared__ double red[DOP_WAVES * DOP_NSUM];
  dop_fill_lds(tab, coef, s.nimp, s.nops);
  const int tid = threadIdx.x;
  const bool hi = s.nimp > 5;
  double acc[DOP_NSUM];
#pragma unroll
  for (int a = 0; a < DOP_NSUM; ++a) acc[a] = 0.0;
  for (int item = blockIdx.x; item < (int)s.nitems; item += gridDim.x) {
    const int c = item / s.nchunk, r0 = (item - c * s.nchunk) * s.rows, r1 = min(r0 + s.rows, s.dimup);
    const double2* __restrict__ col = psi + (int64_t)c * s.pitch;
    const uint32_t od = occ_dw[c];
    double fd[DOP_MAX];
#pragma unroll
    for (int a = 0; a < DOP_MAX; ++a) fd[a] = dop_f(tab, 1, a, od, hi);
    for (int rb = r0; rb < r1; rb += DOP_THREADS * DOP_UNROLL) {
      double2 x[DOP_UNROLL];
      uint32_t ou[DOP_UNROLL];
#pragma unroll
      for (int u = 0; u < DOP_UNROLL; ++u) {
        const int r = rb + u * DOP_THREADS + tid;
        const bool live = r < r1;
        x[u] = live ? col[r] : make_double2(0.0, 0.0);
        ou[u] = live ? occ_up[r] : 0u;
      }
#pragma unroll
      for (int u = 0; u < DOP_UNROLL; ++u) {
        const double w = x[u].x * x[u].x + x[u].y * x[u].y;
        acc[DOP_MAX] += w;
#pragma unroll
        for (int a = 0; a < DOP_MAX; ++a)
          if (a < s.nops) acc[a] += (dop_f(tab, 0, a, ou[u], hi) + fd[a]) * w;
      }
    }
  }
  dop_block_sums(acc, red, partial);
}

__global__ void __launch_bounds__(DOP_THREADS) dop_apply_kernel(const double2* __restrict__ psi, const uint32_t* __restrict__ occ_up,
                                                                const uint32_t* __restrict__ occ_dw, const double* __restrict__ coef, DopShape s,
                                                                DopOut out, double* __restrict__ partial) {
  __shared__ double tab[4 * DOP_MAX * 32];
  __shared__ double red[DOP_WAVES * DOP_NSUM];
  dop_fill_lds(tab, coef, s.nimp, s.nops);
  const int tid = threadIdx.x;
  const bool hi = s.nimp > 5;
  double acc[DOP_NSUM];
#pragma unroll
  for (int a = 0; a < DOP_NSUM; ++a) acc[a] = 0.0;
  for (int item = blockIdx.x; item < (int)s.nitems; item += gridDim.x) {
    const int c = item / s.nchunk, r0 = (item - c * s.nchunk) * s.rows, r1 = min(r0 + s.rows, s.pitch);  // the pad rows are written
    const int64_t off = (int64_t)c * s.pitch;
    const uint32_t od = occ_dw[c];
    double fd[DOP_MAX];
#pragma unroll
    for (int a = 0; a < DOP_MAX; ++a) fd[a] = dop_f(tab, 1, a, od, hi) - out.m[a];
    for (int rb = r0; rb < r1; rb += DOP_THREADS * DOP_UNROLL) {
      double2 x[DOP_UNROLL];
      uint32_t ou[DOP_UNROLL];
#pragma unroll
      for (int u = 0; u < DOP_UNROLL; ++u) {
        const int r = rb + u * DOP_THREADS + tid;
        const bool live = r < s.dimup && r < r1;  // a pad row of psi is never read
        x[u] = live ? psi[off + r] : make_double2(0.0, 0.0);
        ou[u] = live ? occ_up[r] : 0u;
      }
#pragma unroll
      for (int u = 0; u < DOP_UNROLL; ++u) {
        const int r = rb + u * DOP_THREADS + tid;
        const bool live = r < s.dimup && r < r1;
#pragma unroll
        for (int a = 0; a < DOP_MAX; ++a)
          if (a < s.nops) {
            const double g = dop_f(tab, 0, a, ou[u], hi) + fd[a];
            const double2 y = live ? make_double2(g * x[u].x, g * x[u].y) : make_double2(0.0, 0.0);
            if (r < r1) out.v[a][off + r] = y;
            acc[a] += y.x * y.x + y.y * y.y;
          }
      }
    }
  }
  dop_block_sums(acc, red, partial);
}

// sums[v] = partial[0..nblocks)[src], v = blockIdx.x, src = v, or DOP_MAX (where pass 1 keeps the norm) for v == norm_at: strided over the
// threads in block order, then the fixed-order tree
__global__ void __launch_bounds__(DOP_THREADS) dop_reduce_kernel(const double* __restrict__ partial, int nblocks, int norm_at,
                                                                 double* __restrict__ sums) {
  __shared__ double red[DOP_WAVES];
  const int tid = threadIdx.x, v = blockIdx.x, src = v == norm_at ? DOP_MAX : v;
  double acc = 0.0;
  for (int b0 = 0; b0 < nblocks; b0 += DOP_THREADS) {
    const int b = b0 + tid;
    acc += b < nblocks ? partial[(int64_t)b * DOP_NSUM + src] : 0.0;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double r = red[0];
    for (int w = 1; w < DOP_WAVES; ++w) r += red[w];
    sums[v] = r;
  }
}
}  // namespace
