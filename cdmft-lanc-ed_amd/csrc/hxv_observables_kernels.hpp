// The four kernels of hxv_observables_accumulate (hxv_observables.hip, which says what they compute and why in this form):
//   obs_rows_kernel<false>, obs_rows_kernel<true>, obs_rdw_kernel
//                      one workgroup per local column c -> colout[c][g], g over Gtot = 2^Nimp + 2*Nimp^2 groups
//   obs_reduce_kernel  one workgroup per record element
// No floating-point atomics, every sum in a fixed order: the same vector gives the same bits on every call.
// Like hxv_chebyshev_kernels.hpp this is a header with everything in an anonymous namespace, so that tests/device/observables_kernels_check.hip
// can launch each kernel alone with a grid, sizes and tables the driver never passes; the product includes it from hxv_observables.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {
constexpr int OBS_THREADS = 256;
constexpr int OBS_WAVES = OBS_THREADS / 64;
constexpr int OBS_MAX_NIMP = 10;  // record of 4^10 + 400 doubles (8 MB); the reference's own cluster_density_matrix is 4^Nimp squared

__device__ __forceinline__ double2 wave_sum(double2 v) {
  for (int off = 32; off > 0; off >>= 1) {
    v.x += __shfl_xor(v.x, off, 64);
    v.y += __shfl_xor(v.y, off, 64);
  }
  return v;
}

// the same value on every thread of the workgroup: per-wave butterflies, then the waves in order
__device__ __forceinline__ double2 block_sum(double2 v, double2* sh) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  double2 r = sh[0];
  for (int i = 1; i < OBS_WAVES; ++i) {
    r.x += sh[i].x;
    r.y += sh[i].y;
  }
  __syncthreads();
  return r;
}

// One workgroup per local column c of this rank's slab psi [qdw][pitch]; colout[c][g], g over Gtot = nw + 2*np.
// W bins (PAIRS = false, g < nw) and R_up pairs (PAIRS = true, g = nw + p): one wave per group, lanes over the group's rows.
template <bool PAIRS>
__global__ void __launch_bounds__(OBS_THREADS) obs_rows_kernel(const double2* __restrict__ psi, int pitch, int qdw, int nw, int np,
                                                               const int32_t* __restrict__ seg_ptr, const int32_t* __restrict__ ent_a,
                                                               const int32_t* __restrict__ ent_b, const int8_t* __restrict__ ent_s,
                                                               double2* __restrict__ colout) {
  const int c = blockIdx.x;
  if (c >= qdw) return;
  const double2* __restrict__ col = psi + (int64_t)c * pitch;
  double2* __restrict__ out = colout + (int64_t)c * (nw + 2 * np);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g0 = PAIRS ? nw : 0, g1 = PAIRS ? nw + np : nw;
  for (int g = g0 + w; g < g1; g += OBS_WAVES) {
    const int e0 = seg_ptr[g], e1 = seg_ptr[g + 1];
    double2 acc = make_double2(0.0, 0.0);
    if (!PAIRS) {
      for (int e = e0 + lane; e < e1; e += 64) {
        const double2 x = col[ent_a[e]];
        acc.x += x.x * x.x + x.y * x.y;
      }
    } else {
      for (int e = e0 + lane; e < e1; e += 64) {
        const double2 x = col[ent_a[e]], y = col[ent_b[e]];
        const double sg = (double)ent_s[e];
        acc.x += sg * (x.x * y.x + x.y * y.y);  // x * conj(y)
        acc.y += sg * (x.y * y.x - x.x * y.y);
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) out[g] = acc;
  }
}

// R_dw pairs: whole-column products <partner column | this column>; full: the column slots the dw pairs name ([nranks*cmax][pitch] gathered
// copy, or psi itself)
__global__ void __launch_bounds__(OBS_THREADS) obs_rdw_kernel(const double2* __restrict__ psi, const double2* __restrict__ full, int pitch, int dimup,
                                                              int qdw, int nw, int np, const int32_t* __restrict__ dwp_ptr,
                                                              const int32_t* __restrict__ dwp_slot, const int32_t* __restrict__ dwp_p,
                                                              const int8_t* __restrict__ dwp_s, double2* __restrict__ colout) {
  __shared__ double2 sh[OBS_WAVES];
  __shared__ double2 sdw[OBS_MAX_NIMP * OBS_MAX_NIMP];
  const int c = blockIdx.x;
  if (c >= qdw) return;
  const double2* __restrict__ col = psi + (int64_t)c * pitch;
  double2* __restrict__ out = colout + (int64_t)c * (nw + 2 * np);
  for (int i = threadIdx.x; i < np; i += OBS_THREADS) sdw[i] = make_double2(0.0, 0.0);
  __syncthreads();
  for (int k = dwp_ptr[c]; k < dwp_ptr[c + 1]; ++k) {
    const double2* __restrict__ pc = full + (int64_t)dwp_slot[k] * pitch;
    double2 acc = make_double2(0.0, 0.0);
    for (int r = threadIdx.x; r < dimup; r += OBS_THREADS) {
      const double2 x = col[r], y = pc[r];
      acc.x += x.x * y.x + x.y * y.y;
      acc.y += x.y * y.x - x.x * y.y;
    }
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) {
      const double sg = (double)dwp_s[k];
      sdw[dwp_p[k]] = make_double2(sg * acc.x, sg * acc.y);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < np; i += OBS_THREADS) out[nw + np + i] = sdw[i];
}

// rec: [nw*nw] W, then [2*np] R_up, [2*np] R_dw (re, im); R's diagonal is left 0 here (the host fills it from W)
__global__ void __launch_bounds__(OBS_THREADS) obs_reduce_kernel(const double2* __restrict__ colout, int qdw, int nimp, int nw, int np,
                                                                 const int32_t* __restrict__ dwbin_ptr, const int32_t* __restrict__ dwbin_cols,
                                                                 double* __restrict__ rec) {
  __shared__ double2 sh[OBS_WAVES];
  const int64_t o = blockIdx.x;
  const int64_t nww = (int64_t)nw * nw;
  const int gtot = nw + 2 * np;
  double2 acc = make_double2(0.0, 0.0);
  if (o < nww) {
    const int a_up = (int)(o & (nw - 1)), a_dw = (int)(o >> nimp);
    for (int k = dwbin_ptr[a_dw] + threadIdx.x; k < dwbin_ptr[a_dw + 1]; k += OBS_THREADS) acc.x += colout[(int64_t)dwbin_cols[k] * gtot + a_up].x;
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) rec[o] = acc.x;
  } else {
    const int q = (int)(o - nww);  // 0..2np-1: R_up(p), then R_dw(p)
    for (int c = threadIdx.x; c < qdw; c += OBS_THREADS) {
      const double2 v = colout[(int64_t)c * gtot + nw + q];
      acc.x += v.x;
      acc.y += v.y;
    }
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) {
      rec[nww + 2 * q] = acc.x;
      rec[nww + 2 * q + 1] = acc.y;
    }
  }
}
}  // namespace
