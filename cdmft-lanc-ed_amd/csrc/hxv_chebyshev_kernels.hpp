// The two streaming kernels of the Chebyshev recurrence (hxv_chebyshev.hip):  t_0 = v,  t_1 = Ht v,  t_{n+1} = 2 Ht t_n - t_{n-1}  with
// Ht = (H - b)/a.  The product H t_n is the engine's own (apply_slab, no epilogue); what is here is everything else a step does, in ONE pass
// over the vectors: the linear combination, the running sum  out += c_{n+1} t_{n+1},  the overlaps of t_{n+1} with up to HXV_MAX_PROBES probe
// vectors, and the two self-overlaps <t_{n+1}|t_{n+1}>, <t_{n+1}|t_n> that give two diagonal moments per product.
// COMPLEX VECTORS (double2 elements, this rank's slab of qdw * pitch elements); the real-vector form is hxv_chebyshev_real_kernels.hpp.
// Pad rows are zero in every input; they come out as +0.0 and enter every sum as zeros.
// Reductions as everywhere in the engine (hxv_lanczos_kernels.hpp): per-thread sums in the order of the grid-stride loop, products rounded
// before they are added, block_sum's fixed 256-entry LDS tree, one partial per workgroup and accumulator, and lz_probe_final on ONE workgroup
// adding the partials in block order.  No floating-point atomics: the same inputs on the same grid give the same bits.
// Like hxv_lanczos_kernels.hpp this is a header with everything in an anonymous namespace, so that tests/device/chebyshev_kernels_check.hip can
// launch each kernel alone with a grid and sizes the driver never passes; the product includes it from hxv_chebyshev.hip only.
#pragma once

#include "hxv_lanczos_kernels.hpp"  // block_sum, grid_for, LzProbes, lz_probe_final, with_probe_count

namespace {

// accumulators of one step: (Re, Im) <p_j|t> for j < M, then <t|t>, then (Re, Im) <t|t_cur>
constexpr int ch_sums(int m) { return 2 * m + 3; }

// acc[2j], acc[2j+1] += conj(p) * t  -- lz_probe_dots' own terms
__device__ __forceinline__ void ch_probe_add(double& re, double& im, const double2 p, const double2 t) {
#pragma clang fp contract(off)
  const double u = p.x * t.x, w = p.x * t.y;
  re = re + fma(p.y, t.y, u);
  im = im + fma(-p.y, t.x, w);
}

// STEP 0:  out = c0 * v  (out may be null: nothing is stored);  partial[block][2M+3] = this workgroup's sums of <p_j|v>, <v|v>, and two zeros
// where the later steps keep <t_next|t_cur>.
template <int M>
__global__ void __launch_bounds__(256) ch_init(int64_t n, const double2* __restrict__ v, double2* __restrict__ out, LzProbes pr, double c0r,
                                               double c0i, double* __restrict__ partial) {
  constexpr int NC = ch_sums(M);
  double acc[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) acc[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double2 t = v[i];
    if (out) out[i] = make_double2(fma(c0r, t.x, fma(-c0i, t.y, 0.0)), fma(c0r, t.y, fma(c0i, t.x, 0.0)));  // (the running sum's own form, from +0.0)
#pragma unroll
    for (int j = 0; j < M; ++j) ch_probe_add(acc[2 * j], acc[2 * j + 1], pr.p[j][i], t);
    {
#pragma clang fp contract(off)
      const double u = t.x * t.x;
      acc[2 * M] = acc[2 * M] + fma(t.y, t.y, u);
    }
  }
  block_sum(acc);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NC; ++k) partial[(size_t)blockIdx.x * NC + k] = acc[k];
  }
}

// ONE STEP.  Per element, the thread that reads it also writes it:
//   general form :  t_next = ch*hv - cc*cur - prev     (ch = 2/a, cc = 2b/a),  stored OVER prev
//   FIRST        :  t_next = ch*hv - cc*cur            (ch = 1/a, cc = b/a; cur = v), stored to prev_next, which is not read
//   SUM          :  out += (cr + i ci) * t_next
//   partial[block][2M+3] = this workgroup's sums of  conj(p_j) t_next (re, im; j < M),  |t_next|^2,  conj(t_next) cur (re, im).
// Each component of t_next is two fused multiply-adds in this order, whatever the build.
template <int M, bool SUM, bool FIRST>
__global__ void __launch_bounds__(256) ch_step(int64_t n, const double2* __restrict__ hv, const double2* __restrict__ cur,
                                               double2* __restrict__ prev_next, double2* __restrict__ out, LzProbes pr, double ch, double cc,
                                               double cr, double ci, double* __restrict__ partial) {
  constexpr int NC = ch_sums(M);
  double acc[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) acc[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double2 w = hv[i], c = cur[i];
    double2 p = make_double2(0.0, 0.0);
    if (!FIRST) p = prev_next[i];
    double2 t;
    t.x = fma(-cc, c.x, fma(ch, w.x, -p.x));
    t.y = fma(-cc, c.y, fma(ch, w.y, -p.y));
    prev_next[i] = t;
    if (SUM) {
      double2 o = out[i];
      o.x = fma(cr, t.x, fma(-ci, t.y, o.x));
      o.y = fma(cr, t.y, fma(ci, t.x, o.y));
      out[i] = o;
    }
#pragma unroll
    for (int j = 0; j < M; ++j) ch_probe_add(acc[2 * j], acc[2 * j + 1], pr.p[j][i], t);
    {
#pragma clang fp contract(off)
      const double u = t.x * t.x;
      acc[2 * M] = acc[2 * M] + fma(t.y, t.y, u);
      const double r = t.x * c.x, s = t.x * c.y;
      acc[2 * M + 1] = acc[2 * M + 1] + fma(t.y, c.y, r);
      acc[2 * M + 2] = acc[2 * M + 2] + fma(-t.y, c.x, s);
    }
  }
  block_sum(acc);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NC; ++k) partial[(size_t)blockIdx.x * NC + k] = acc[k];
  }
}

// step 0 on g workgroups, then the block-ordered sum of the partials on one: d_sums[2m+3].  d_part: g * (2m+3) doubles.
inline void launch_ch_init(int g, hipStream_t st, int m, int64_t n, const double2* v, double2* out, const LzProbes& pr, double c0r, double c0i,
                           double* d_part, double* d_sums) {
  with_probe_count<0>(m, [&](auto M) { hipLaunchKernelGGL((ch_init<M()>), dim3(g), dim3(256), 0, st, n, v, out, pr, c0r, c0i, d_part); });
  hipLaunchKernelGGL(lz_probe_final, dim3(1), dim3(256), 0, st, d_part, g, ch_sums(m), d_sums);
}

// one step on g workgroups (out null: no running sum; first: the form without t_prev), then the block-ordered sum of the partials
template <bool SUM, bool FIRST>
void launch_ch_step_form(int g, hipStream_t st, int m, int64_t n, const double2* hv, const double2* cur, double2* prev_next, double2* out,
                         const LzProbes& pr, double ch, double cc, double cr, double ci, double* d_part) {
  with_probe_count<0>(m, [&](auto M) {
    hipLaunchKernelGGL((ch_step<M(), SUM, FIRST>), dim3(g), dim3(256), 0, st, n, hv, cur, prev_next, out, pr, ch, cc, cr, ci, d_part);
  });
}
inline void launch_ch_step(int g, hipStream_t st, int m, bool first, int64_t n, const double2* hv, const double2* cur, double2* prev_next,
                           double2* out, const LzProbes& pr, double ch, double cc, double cr, double ci, double* d_part, double* d_sums) {
  if (out && first)
    launch_ch_step_form<true, true>(g, st, m, n, hv, cur, prev_next, out, pr, ch, cc, cr, ci, d_part);
  else if (out)
    launch_ch_step_form<true, false>(g, st, m, n, hv, cur, prev_next, out, pr, ch, cc, cr, ci, d_part);
  else if (first)
    launch_ch_step_form<false, true>(g, st, m, n, hv, cur, prev_next, out, pr, ch, cc, cr, ci, d_part);
  else
    launch_ch_step_form<false, false>(g, st, m, n, hv, cur, prev_next, out, pr, ch, cc, cr, ci, d_part);
  hipLaunchKernelGGL(lz_probe_final, dim3(1), dim3(256), 0, st, d_part, g, ch_sums(m), d_sums);
}

}  // namespace
