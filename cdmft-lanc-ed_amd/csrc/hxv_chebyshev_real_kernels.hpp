// The REAL-vector form of the two streaming kernels of the Chebyshev recurrence (hxv_chebyshev_kernels.hpp), the conversion that opens a real
// run, and the kernel behind hxv_vector_random.
// LAYOUT of the real kernels: the buffers are double[qdw][pitch_real] (pitch_real a multiple of 16) viewed as double2 -- two consecutive real
// elements per double2, n = pitch_real * qdw / 2 of them -- exactly the view hxv_lanczos.hip gives its streaming kernels (lz_len).  Each lane
// makes one 16-byte access per vector, as in the complex kernels; a state costs half the bytes: (3 + M)*8, (4 + M)*8 with a running sum.
// ARITHMETIC: per component the complex kernel's own two fused multiply-adds for t_next, ONE for the running sum (the coefficient is real);
// M + 2 sums per step instead of 2M + 3, each adding per double2 element  fma(a.y, b.y, a.x*b.x)  with the product rounded first -- the term
// of the Re accumulators of ch_probe_add and of the complex self-overlaps.  So on the same memory these kernels store the bits ch_step /
// ch_init store for t_next, and their sums are bit for bit the Re accumulators of those kernels (tests/test_gpu_chebyshev_real_kernels.py).
// Pad rows are zero in every input; they come out as +0.0.  Reductions as in the complex kernels: block_sum, one partial per workgroup and
// accumulator, lz_probe_final on ONE workgroup.  No floating-point atomics.
// Like its neighbour this is a header with everything in an anonymous namespace, so that tests/device/chebyshev_real_kernels_check.hip can
// launch each kernel alone; the product includes it from hxv_chebyshev.hip only.
#pragma once

#include "hxv_chebyshev_kernels.hpp"

namespace {

// accumulators of one real step: <p_j|t> for j < M, then <t|t>, then <t|t_cur>
constexpr int ch_sums_real(int m) { return m + 2; }

// acc += a.x*b.x + a.y*b.y over the two real elements of one double2: the Re term of ch_probe_add
__device__ __forceinline__ void ch_dot_add(double& acc, const double2 a, const double2 b) {
#pragma clang fp contract(off)
  const double u = a.x * b.x;
  acc = acc + fma(a.y, b.y, u);
}

// STEP 0:  out = c0 * v  (out may be null: nothing is stored);  partial[block][M+2] = this workgroup's sums of <p_j|v>, <v|v>, and one zero
// where the later steps keep <t_next|t_cur>.
template <int M>
__global__ void __launch_bounds__(256) ch_init_real(int64_t n, const double2* __restrict__ v, double2* __restrict__ out, LzProbes pr, double c0,
                                                    double* __restrict__ partial) {
  constexpr int NC = ch_sums_real(M);
  double acc[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) acc[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double2 t = v[i];
    if (out) out[i] = make_double2(fma(c0, t.x, 0.0), fma(c0, t.y, 0.0));  // (the running sum's own form, from +0.0)
#pragma unroll
    for (int j = 0; j < M; ++j) ch_dot_add(acc[j], pr.p[j][i], t);
    ch_dot_add(acc[M], t, t);
  }
  block_sum(acc);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NC; ++k) partial[(size_t)blockIdx.x * NC + k] = acc[k];
  }
}

// ONE STEP on real vectors; forms and scalars as in ch_step, cr the REAL coefficient of the running sum:
//   general form :  t_next = ch*hv - cc*cur - prev,  stored OVER prev
//   FIRST        :  t_next = ch*hv - cc*cur,         stored to prev_next, which is not read
//   SUM          :  out += cr * t_next
//   partial[block][M+2] = this workgroup's sums of  p_j t_next (j < M),  t_next^2,  t_next cur.
template <int M, bool SUM, bool FIRST>
__global__ void __launch_bounds__(256) ch_step_real(int64_t n, const double2* __restrict__ hv, const double2* __restrict__ cur,
                                                    double2* __restrict__ prev_next, double2* __restrict__ out, LzProbes pr, double ch, double cc,
                                                    double cr, double* __restrict__ partial) {
  constexpr int NC = ch_sums_real(M);
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
      o.x = fma(cr, t.x, o.x);
      o.y = fma(cr, t.y, o.y);
      out[i] = o;
    }
#pragma unroll
    for (int j = 0; j < M; ++j) ch_dot_add(acc[j], pr.p[j][i], t);
    ch_dot_add(acc[M], t, t);
    ch_dot_add(acc[M + 1], t, c);
  }
  block_sum(acc);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NC; ++k) partial[(size_t)blockIdx.x * NC + k] = acc[k];
  }
}

// step 0 on g workgroups, then the block-ordered sum of the partials on one: d_sums[m+2].  d_part: g * (m+2) doubles.
inline void launch_ch_init_real(int g, hipStream_t st, int m, int64_t n, const double2* v, double2* out, const LzProbes& pr, double c0,
                                double* d_part, double* d_sums) {
  with_probe_count<0>(m, [&](auto M) { hipLaunchKernelGGL((ch_init_real<M()>), dim3(g), dim3(256), 0, st, n, v, out, pr, c0, d_part); });
  hipLaunchKernelGGL(lz_probe_final, dim3(1), dim3(256), 0, st, d_part, g, ch_sums_real(m), d_sums);
}

template <bool SUM, bool FIRST>
void launch_ch_step_real_form(int g, hipStream_t st, int m, int64_t n, const double2* hv, const double2* cur, double2* prev_next, double2* out,
                              const LzProbes& pr, double ch, double cc, double cr, double* d_part) {
  with_probe_count<0>(m, [&](auto M) {
    hipLaunchKernelGGL((ch_step_real<M(), SUM, FIRST>), dim3(g), dim3(256), 0, st, n, hv, cur, prev_next, out, pr, ch, cc, cr, d_part);
  });
}
// one real step on g workgroups (out null: no running sum; first: the form without t_prev), then the block-ordered sum of the partials
inline void launch_ch_step_real(int g, hipStream_t st, int m, bool first, int64_t n, const double2* hv, const double2* cur, double2* prev_next,
                                double2* out, const LzProbes& pr, double ch, double cc, double cr, double* d_part, double* d_sums) {
  if (out && first)
    launch_ch_step_real_form<true, true>(g, st, m, n, hv, cur, prev_next, out, pr, ch, cc, cr, d_part);
  else if (out)
    launch_ch_step_real_form<true, false>(g, st, m, n, hv, cur, prev_next, out, pr, ch, cc, cr, d_part);
  else if (first)
    launch_ch_step_real_form<false, true>(g, st, m, n, hv, cur, prev_next, out, pr, ch, cc, cr, d_part);
  else
    launch_ch_step_real_form<false, false>(g, st, m, n, hv, cur, prev_next, out, pr, ch, cc, cr, d_part);
  hipLaunchKernelGGL(lz_probe_final, dim3(1), dim3(256), 0, st, d_part, g, ch_sums_real(m), d_sums);
}

// real [dimdw][pr] <- Re(complex [dimdw][pc]), pads zero: lz_to_real's conversion.  partial = per-block sum of |Im| over the rows below dimup:
// the absolute value, not lz_to_real's square, because the square of a tiny imaginary part (1e-300) underflows to zero and a caller who asked
// for the real form by name is refused for ANY imaginary part.
__global__ void __launch_bounds__(256) ch_to_real(int dimup, int dimdw, int pc, int pr, const double2* __restrict__ src, double* __restrict__ dst,
                                                  double* __restrict__ partial) {
  const int64_t n = (int64_t)dimdw * pr;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t col = i / pr;
    const int row = (int)(i - col * pr);
    double x = 0.0;
    if (row < dimup) {
      const double2 z = src[col * pc + row];
      x = z.x;
      acc += fabs(z.y);
    }
    dst[i] = x;
  }
  const double sum = block_sum(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// ---- hxv_vector_random (include/hxv.h) ----
// the splitmix64 finaliser (lz_uniform's): add the golden constant, two xorshift-multiplies, ^ >> 31
__host__ __device__ inline uint64_t vr_mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// u(I, c) = (double)(mix(key ^ (2 I + c)) >> 11) * 2^-53 - 0.5,  key = mix(seed): uniform in [-0.5, 0.5)
__device__ __forceinline__ double vr_uniform(uint64_t key, uint64_t I, uint64_t c) {
  return (double)(vr_mix(key ^ (2 * I + c)) >> 11) * (1.0 / 9007199254740992.0) - 0.5;
}
// q[i] = (u(I, 0), complex_valued ? u(I, 1) : +0.0) times the basis sign of the row, I = col * dimup + reference row, on this rank's slab of n =
// qdw * pitch elements; pad rows zero.  col0, iperm, sign as in lz_init: the vector is defined on the GLOBAL REFERENCE index.
__global__ void __launch_bounds__(256) vec_random(int64_t n, double2* __restrict__ q, uint64_t key, int complex_valued, int dimup, int pitch,
                                                  int col0, const int32_t* __restrict__ iperm, const uint8_t* __restrict__ sign) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t lcol = i / pitch;
    const int row = (int)(i - lcol * pitch);
    if (row >= dimup) {
      q[i] = make_double2(0.0, 0.0);
      continue;
    }
    const int rrow = iperm ? iperm[row] : row;
    const double sgn = (sign && sign[row]) ? -1.0 : 1.0;
    const uint64_t I = (uint64_t)((lcol + col0) * dimup + rrow);
    q[i] = make_double2(sgn * vr_uniform(key, I, 0), complex_valued ? sgn * vr_uniform(key, I, 1) : 0.0);
  }
}

}  // namespace
