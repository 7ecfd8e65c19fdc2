// The device code of hxv_apply_spin_pair (hxv_spin_pair.hip): out = sum_t coef_t X_t Y_t psi for operators that change BOTH spin sectors
// at once, X_t = c / c^dagger on an up orbital, Y_t on a dw orbital -- the start vectors of the pair and spin-flip susceptibilities.  In a
// header of its own so that tests/device/spin_pair_kernels_check.hip can launch the kernel alone on synthetic tables
// (tests/test_gpu_spin_pair_kernels.py).
//
// Gather form, one pass.  A table entry (host: hxv_spin_pair_tables.cpp) is -1 (the target is not reached) or source | sign << 31:
//   up table  [dimup_to]  target device row    -> source device row, sign = operator parity x both basis signs
//   dw table  [dimdw_to]  target column        -> source column,     sign = operator parity
// A work item is SP_THREADS consecutive rows of one target column, a thread owns one element of it: the dw entry of every term is uniform
// over the workgroup (scalar loads), a term whose source column is -1 is skipped for the whole item.  Each DISTINCT up table is looked up
// once per row and parked in the thread's own LDS slot (no barrier: a thread reads back what it wrote), whichever terms use it.  The terms
// are added in the order given, in registers; one 16-byte store per element, zeros where no term is live and in the pad rows.  <out|out>
// rides along: per-thread sums over the items in a fixed order, a fixed tree over the workgroup, one partial per workgroup;
// spin_pair_norm_kernel adds the partials in index order.  No atomics: the same inputs on the same grid give the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace hxv {

constexpr int SP_THREADS = 256;    // rows of a work item
constexpr int SP_MAX_TERMS = 32;   // = HXV_MAX_SPIN_PAIR_TERMS
constexpr int SP_MAX_GRID = 2048;  // partials of the norm: the handle's reduction scratch holds that many

// the term list, passed by value (kernel arguments: uniform, read by scalar loads)
struct SpTerms {
  int32_t nterms;                 // 1 .. SP_MAX_TERMS
  int32_t nuq;                    // distinct up tables, 1 .. nterms
  uint8_t uq_tab[SP_MAX_TERMS];   // [nuq] which up table (index into the up-table block)
  uint8_t t_uq[SP_MAX_TERMS];     // [nterms] term -> position in uq_tab
  uint8_t t_dw[SP_MAX_TERMS];     // [nterms] term -> dw table (index into the dw-table block)
  double2 coef[SP_MAX_TERMS];     // [nterms]
};

// dynamic LDS: nuq * SP_THREADS * 4 bytes
__global__ void __launch_bounds__(SP_THREADS) spin_pair_kernel(SpTerms tm, const int32_t* __restrict__ up_tab, int64_t up_stride,
                                                              const int32_t* __restrict__ dw_tab, int64_t dw_stride, int dimup_to, int pitch_to,
                                                              int dimdw_to, int pitch_from, const double2* __restrict__ psi,
                                                              double2* __restrict__ out, double* __restrict__ partials) {
  extern __shared__ int32_t sp_entries[];  // [nuq][SP_THREADS]
  __shared__ double sp_red[SP_THREADS];
  const int tid = threadIdx.x;
  const int nchunk = (pitch_to + SP_THREADS - 1) / SP_THREADS;
  const int64_t nitems = (int64_t)dimdw_to * nchunk;
  double s = 0.0;
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int c = (int)(item / nchunk);
    const int i = (int)(item - (int64_t)c * nchunk) * SP_THREADS + tid;
    if (i >= pitch_to) continue;
    double2 acc = make_double2(0.0, 0.0);
    if (i < dimup_to) {
      for (int u = 0; u < tm.nuq; ++u) sp_entries[u * SP_THREADS + tid] = up_tab[(int64_t)tm.uq_tab[u] * up_stride + i];
      bool first = true;
      for (int t = 0; t < tm.nterms; ++t) {
        const int32_t d = dw_tab[(int64_t)tm.t_dw[t] * dw_stride + c];  // uniform
        if (d == -1) continue;
        const int32_t e = sp_entries[(int)tm.t_uq[t] * SP_THREADS + tid];
        if (e == -1) continue;
        const double2 x = psi[(int64_t)(d & 0x7FFFFFFF) * pitch_from + (e & 0x7FFFFFFF)];
        const double sg = ((uint32_t)(d ^ e) >> 31) ? -1.0 : 1.0;
        const double2 cf = tm.coef[t];
        const double2 r = make_double2(sg * (cf.x * x.x - cf.y * x.y), sg * (cf.x * x.y + cf.y * x.x));
        // the first live term is stored, not added to zero: a single term is then the ladder kernels' expression, bit for bit
        acc = first ? r : make_double2(acc.x + r.x, acc.y + r.y);
        first = false;
      }
    }
    out[(int64_t)c * pitch_to + i] = acc;
    s += acc.x * acc.x + acc.y * acc.y;
  }
  sp_red[tid] = s;
  __syncthreads();
  for (int w = SP_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) sp_red[tid] += sp_red[tid + w];
    __syncthreads();
  }
  if (tid == 0) partials[blockIdx.x] = sp_red[0];
}

// *result = partials[0] + ... + partials[n-1]: every thread its strided share in index order, then the same fixed tree.  One workgroup.
__global__ void __launch_bounds__(SP_THREADS) spin_pair_norm_kernel(const double* __restrict__ partials, int n, double* __restrict__ result) {
  __shared__ double sp_red[SP_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int k = tid; k < n; k += SP_THREADS) s += partials[k];
  sp_red[tid] = s;
  __syncthreads();
  for (int w = SP_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) sp_red[tid] += sp_red[tid + w];
    __syncthreads();
  }
  if (tid == 0) *result = sp_red[0];
}

// the grid the engine uses for a target of dimdw_to columns of pitch_to rows: one workgroup per work item up to SP_MAX_GRID
inline int spin_pair_grid(int pitch_to, int dimdw_to) {
  const int64_t nitems = (int64_t)dimdw_to * ((pitch_to + SP_THREADS - 1) / SP_THREADS);
  return (int)(nitems < SP_MAX_GRID ? (nitems < 1 ? 1 : nitems) : SP_MAX_GRID);
}

// both kernels on `st`: every element of `out` ([dimdw_to][pitch_to]) is written, partials[0..grid) and *result too
inline hipError_t launch_spin_pair(const SpTerms& tm, int grid, const int32_t* up_tab, int64_t up_stride, const int32_t* dw_tab, int64_t dw_stride,
                                   int dimup_to, int pitch_to, int dimdw_to, int pitch_from, const double2* psi, double2* out, double* partials,
                                   double* result, hipStream_t st) {
  hipLaunchKernelGGL(spin_pair_kernel, dim3((unsigned)grid), dim3(SP_THREADS), (size_t)tm.nuq * SP_THREADS * sizeof(int32_t), st, tm, up_tab, up_stride,
                     dw_tab, dw_stride, dimup_to, pitch_to, dimdw_to, pitch_from, psi, out, partials);
  hipLaunchKernelGGL(spin_pair_norm_kernel, dim3(1), dim3(SP_THREADS), 0, st, (const double*)partials, grid, result);
  return hipGetLastError();
}

}  // namespace hxv
