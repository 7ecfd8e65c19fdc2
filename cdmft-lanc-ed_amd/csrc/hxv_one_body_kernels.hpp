// The device code of hxv_apply_one_body (hxv_one_body.hip): out = (sum_t coef_t c^dagger_{i_t s_t} c_{j_t s_t} - m) psi inside one sector --
// the start vectors of the bond, current and exciton susceptibilities.  In a header of its own so that
// tests/device/one_body_kernels_check.hip can launch the kernels alone on synthetic tables (tests/test_gpu_one_body_kernels.py).
//
// Gather form, one pass.  A table entry (host: hxv_one_body_tables.cpp) is -1 (the target is not reached) or source | sign << 31:
//   up table  [dimup]  target device row -> source device row, sign = parity x both basis signs
//   dw table  [dimdw]  target column     -> source column,     sign = parity
// A work item is OB_THREADS consecutive rows of one target column, a thread owns one element of it.  A dw term's entry is uniform over the
// workgroup (scalar load), a dead column skips the term for the whole item, and its source is the same rows of another column: a coalesced
// read.  An up term gathers another row of the SAME column (element-granular, served by L2: a column is 16 dimup bytes); each DISTINCT up
// table is looked up once per row and parked in the thread's own LDS slot (no barrier: a thread reads back what it wrote), whichever terms
// use it.  The terms are added in the order given, in registers; the first live term is stored, not added to zero.  One 16-byte store per
// element, zeros where no term is live and in the pad rows.  The thread's own psi element rides along (one more coalesced read) for the
// four sums <psi|psi>, Re <psi|out>, Im <psi|out>, <out|out>: per-thread sums over the items in a fixed order, a fixed tree over the
// workgroup, one partial of each per workgroup; one_body_sums_kernel adds the partials in index order.  one_body_shift_kernel is the
// streaming pass out -= m psi with <out|out> summed afresh from what it stores.  No atomics: the same inputs on the same grid give the
// same bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace hxv {

constexpr int OB_THREADS = 256;    // rows of a work item
constexpr int OB_MAX_TERMS = 32;   // = HXV_MAX_ONE_BODY_TERMS
constexpr int OB_MAX_GRID = 2048;  // workgroups of the two passes, at most
constexpr int OB_NSUM = 4;         // <psi|psi>, Re <psi|out>, Im <psi|out>, <out|out>; partials[k * grid + workgroup]

// the term list, passed by value (kernel arguments: uniform, read by scalar loads)
struct ObTerms {
  int32_t nterms;                     // 1 .. OB_MAX_TERMS
  int32_t nuq;                        // distinct up tables, 0 .. nterms
  const int32_t* uq_tab[OB_MAX_TERMS];  // [nuq] the distinct up tables
  const int32_t* dw_tab[OB_MAX_TERMS];  // [nterms] the dw table of a dw term, null for an up term
  uint8_t t_uq[OB_MAX_TERMS];         // [nterms] up term -> position in uq_tab
  double2 coef[OB_MAX_TERMS];         // [nterms]
};

// the workgroup's sum of v in a fixed tree -> the return value on thread 0
__device__ __forceinline__ double ob_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();  // (red may still be read from the sum before)
  red[tid] = v;
  __syncthreads();
  for (int w = OB_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  return red[0];
}

// dynamic LDS: max(nuq, 1) * OB_THREADS * 4 bytes
__global__ void __launch_bounds__(OB_THREADS) one_body_kernel(ObTerms tm, int dimup, int pitch, int dimdw, const double2* __restrict__ psi,
                                                             double2* __restrict__ out, double* __restrict__ partials) {
  extern __shared__ int32_t ob_entries[];  // [nuq][OB_THREADS]
  __shared__ double ob_red[OB_THREADS];
  const int tid = threadIdx.x;
  const int nchunk = (pitch + OB_THREADS - 1) / OB_THREADS;
  const int64_t nitems = (int64_t)dimdw * nchunk;
  double s_pp = 0.0, s_re = 0.0, s_im = 0.0, s_oo = 0.0;
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int c = (int)(item / nchunk);
    const int i = (int)(item - (int64_t)c * nchunk) * OB_THREADS + tid;
    if (i >= pitch) continue;
    const double2* __restrict__ col = psi + (int64_t)c * pitch;
    double2 acc = make_double2(0.0, 0.0), own = make_double2(0.0, 0.0);
    if (i < dimup) {
      own = col[i];
      for (int u = 0; u < tm.nuq; ++u) ob_entries[u * OB_THREADS + tid] = tm.uq_tab[u][i];
      bool first = true;
      for (int t = 0; t < tm.nterms; ++t) {
        const int32_t* __restrict__ dt = tm.dw_tab[t];  // uniform
        int32_t e;
        double2 x;
        if (dt) {
          e = dt[c];  // uniform
          if (e == -1) continue;
          x = psi[(int64_t)(e & 0x7FFFFFFF) * pitch + i];
        } else {
          e = ob_entries[(int)tm.t_uq[t] * OB_THREADS + tid];
          if (e == -1) continue;
          x = col[e & 0x7FFFFFFF];
        }
        const double sg = ((uint32_t)e >> 31) ? -1.0 : 1.0;
        const double2 cf = tm.coef[t];
        const double2 r = make_double2(sg * (cf.x * x.x - cf.y * x.y), sg * (cf.x * x.y + cf.y * x.x));
        // the first live term is stored, not added to zero: a single term is then the ladder kernels' expression, bit for bit
        acc = first ? r : make_double2(acc.x + r.x, acc.y + r.y);
        first = false;
      }
    }
    out[(int64_t)c * pitch + i] = acc;
    s_pp += own.x * own.x + own.y * own.y;
    s_re += own.x * acc.x + own.y * acc.y;
    s_im += own.x * acc.y - own.y * acc.x;
    s_oo += acc.x * acc.x + acc.y * acc.y;
  }
  const double sums[OB_NSUM] = {s_pp, s_re, s_im, s_oo};
#pragma unroll
  for (int k = 0; k < OB_NSUM; ++k) {
    const double v = ob_block_sum(sums[k], ob_red);
    if (tid == 0) partials[(int64_t)k * gridDim.x + blockIdx.x] = v;
  }
}

// out -= m psi on the rows below dimup (the pad rows of out stay as they are, those of psi are never read); partials[workgroup] = the
// workgroup's share of <out|out>, from the elements it stores.  The work items and their order are one_body_kernel's.
__global__ void __launch_bounds__(OB_THREADS) one_body_shift_kernel(double2 m, int dimup, int pitch, int dimdw, const double2* __restrict__ psi,
                                                                   double2* __restrict__ out, double* __restrict__ partials) {
  __shared__ double ob_red[OB_THREADS];
  const int tid = threadIdx.x;
  const int nchunk = (pitch + OB_THREADS - 1) / OB_THREADS;
  const int64_t nitems = (int64_t)dimdw * nchunk;
  double s = 0.0;
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int c = (int)(item / nchunk);
    const int i = (int)(item - (int64_t)c * nchunk) * OB_THREADS + tid;
    if (i >= dimup) continue;
    const int64_t at = (int64_t)c * pitch + i;
    const double2 x = psi[at];
    double2 o = out[at];
    o.x -= m.x * x.x - m.y * x.y;
    o.y -= m.x * x.y + m.y * x.x;
    out[at] = o;
    s += o.x * o.x + o.y * o.y;
  }
  const double v = ob_block_sum(s, ob_red);
  if (tid == 0) partials[blockIdx.x] = v;
}

// result[k] = partials[k * n + 0] + ... + partials[k * n + n - 1], k = blockIdx.x: every thread its strided share in index order, then the
// same fixed tree.  One workgroup per sum.
__global__ void __launch_bounds__(OB_THREADS) one_body_sums_kernel(const double* __restrict__ partials, int n, double* __restrict__ result) {
  __shared__ double ob_red[OB_THREADS];
  const int tid = threadIdx.x;
  const double* __restrict__ p = partials + (int64_t)blockIdx.x * n;
  double s = 0.0;
  for (int k = tid; k < n; k += OB_THREADS) s += p[k];
  const double v = ob_block_sum(s, ob_red);
  if (tid == 0) result[blockIdx.x] = v;
}

// the grid the engine uses for a sector of dimdw columns of pitch rows: one workgroup per work item up to OB_MAX_GRID
inline int one_body_grid(int pitch, int dimdw) {
  const int64_t nitems = (int64_t)dimdw * ((pitch + OB_THREADS - 1) / OB_THREADS);
  return (int)(nitems < OB_MAX_GRID ? (nitems < 1 ? 1 : nitems) : OB_MAX_GRID);
}

// the gather pass and its sums on `st`: every element of `out` ([dimdw][pitch]) is written, partials[0 .. OB_NSUM * grid) and
// result[0 .. OB_NSUM) too
inline hipError_t launch_one_body(const ObTerms& tm, int grid, int dimup, int pitch, int dimdw, const double2* psi, double2* out,
                                  double* partials, double* result, hipStream_t st) {
  const size_t lds = (size_t)(tm.nuq > 0 ? tm.nuq : 1) * OB_THREADS * sizeof(int32_t);
  hipLaunchKernelGGL(one_body_kernel, dim3((unsigned)grid), dim3(OB_THREADS), lds, st, tm, dimup, pitch, dimdw, psi, out, partials);
  hipLaunchKernelGGL(one_body_sums_kernel, dim3(OB_NSUM), dim3(OB_THREADS), 0, st, (const double*)partials, grid, result);
  return hipGetLastError();
}

// the mean-subtraction pass and its sum on `st`: partials[0 .. grid) and *result = <out|out> are written
inline hipError_t launch_one_body_shift(double2 m, int grid, int dimup, int pitch, int dimdw, const double2* psi, double2* out, double* partials,
                                        double* result, hipStream_t st) {
  hipLaunchKernelGGL(one_body_shift_kernel, dim3((unsigned)grid), dim3(OB_THREADS), 0, st, m, dimup, pitch, dimdw, psi, out, partials);
  hipLaunchKernelGGL(one_body_sums_kernel, dim3(1), dim3(OB_THREADS), 0, st, (const double*)partials, grid, result);
  return hipGetLastError();
}

}  // namespace hxv
