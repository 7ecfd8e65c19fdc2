// The streaming and scalar kernels of the single-vector Lanczos recurrence (hxv_lanczos.hip), the block reduction they end with, the grid
// rule and the dispatch of the probe overlaps on the number of probes.
// They live in a header of their own so that tests/device/lanczos_kernels_check.hip can launch each of them alone, with a grid, a stride and
// shapes the drivers never pass; the product includes this file from hxv_lanczos.hip only.  Everything stays in an anonymous namespace:
// each including file gets its own copy, with internal linkage, exactly as when the text stood in hxv_lanczos.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "hxv_handle.hpp"  // RED_BLOCKS, the LzSlot indices, HXV_MAX_PROBES (include/hxv.h)

namespace {

using namespace hxv;

// acc[k] = sum of acc[k] over the 256 threads of a workgroup (every thread gets it), k < N: the LDS tree the reductions end with.  One
// 256-entry tree per accumulator and one barrier per level for all of them; each sum is added in the order of the single tree, so its bits
// do not depend on N.
template <int N>
__device__ __forceinline__ void block_sum(double (&acc)[N]) {
  __shared__ double red[N][256];
  for (int k = 0; k < N; ++k) red[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
      for (int k = 0; k < N; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
    __syncthreads();
  }
  for (int k = 0; k < N; ++k) acc[k] = red[k][0];
}
__device__ __forceinline__ double block_sum(double acc) {
  double a[1] = {acc};
  block_sum(a);
  return a[0];
}

// w -= b*qm ; partial sums of Re<q,w>
__global__ void __launch_bounds__(256) lz_sub_dot(int64_t n, double2* __restrict__ w, const double2* __restrict__ qm,
                                                  const double2* __restrict__ q, const double* __restrict__ scal, int ib,
                                                  double* __restrict__ partial) {
  const double b = ib >= 0 ? scal[ib] : 0.0;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double2 x = w[i];
    if (ib >= 0) {
      double2 p = qm[i];
      x.x -= b * p.x;
      x.y -= b * p.y;
      w[i] = x;
    }
    double2 y = q[i];
    acc += y.x * x.x + y.y * x.y;
  }
  const double sum = block_sum(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// w -= a*q ; partial sums of |w|^2
__global__ void __launch_bounds__(256) lz_sub_nrm(int64_t n, double2* __restrict__ w, const double2* __restrict__ q,
                                                  const double* __restrict__ scal, int ia, double* __restrict__ partial) {
  const double a = scal[ia];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double2 x = w[i], y = q[i];
    // (written out -- one fused multiply-add per component, the squares rounded before they are added -- so that the paired
    //  kernel below reproduces two runs of this one bit for bit)
    x.x = fma(-a, y.x, x.x);
    x.y = fma(-a, y.y, x.y);
    w[i] = x;
    {
#pragma clang fp contract(off)  // (the _rn intrinsics of HIP are plain operators, open to contraction)
      const double t = x.x * x.x;
      acc = acc + fma(x.y, x.y, t);
    }
  }
  const double sum = block_sum(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// PAIRED vectors (real part = vector a, imaginary part = vector b): w.re -= a_a*q.re, w.im -= a_b*q.im; partial sums of
// |w.re|^2 and |w.im|^2 separately
__global__ void __launch_bounds__(256) lz_sub_nrm_pair(int64_t n, double2* __restrict__ w, const double2* __restrict__ q,
                                                       const double* __restrict__ scal, int ia, int ib, double* __restrict__ partial_a,
                                                       double* __restrict__ partial_b) {
  const double a = scal[ia], b = scal[ib];
  double acc = 0.0, acc2 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double2 x = w[i], y = q[i];
    x.x = fma(-a, y.x, x.x);
    x.y = fma(-b, y.y, x.y);
    w[i] = x;
    {
#pragma clang fp contract(off)
      const double t = x.x * x.x, t2 = x.y * x.y;
      acc = acc + t;
      acc2 = acc2 + t2;
    }
  }
  double sum[2] = {acc, acc2};
  block_sum(sum);
  if (threadIdx.x == 0) {
    partial_a[blockIdx.x] = sum[0];
    partial_b[blockIdx.x] = sum[1];
  }
}

// q = (Re a, Re b) from two complex vectors; partial sums of Im(a)^2 + Im(b)^2 (must be zero), |Re a|^2, |Re b|^2
__global__ void __launch_bounds__(256) lz_pack_pair(int64_t n, const double2* __restrict__ a, const double2* __restrict__ b,
                                                    double2* __restrict__ q, double* __restrict__ p_im, double* __restrict__ p_a,
                                                    double* __restrict__ p_b) {
  double im = 0.0, na = 0.0, nb = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double2 x = a[i], y = b[i];
    q[i] = make_double2(x.x, y.x);
    im += x.y * x.y + y.y * y.y;
    {
#pragma clang fp contract(off)
      const double t = x.x * x.x, t2 = y.x * y.x;
      na = na + t;
      nb = nb + t2;
    }
  }
  double sum[3] = {im, na, nb};
  block_sum(sum);
  if (threadIdx.x == 0) {
    p_im[blockIdx.x] = sum[0];
    p_a[blockIdx.x] = sum[1];
    p_b[blockIdx.x] = sum[2];
  }
}

// partial sums of |x|^2
__global__ void __launch_bounds__(256) lz_nrm(int64_t n, const double2* __restrict__ x, double* __restrict__ partial) {
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double2 a = x[i];
    {
#pragma clang fp contract(off)  // (written out: see lz_sub_nrm)
      const double t = a.x * a.x;
      acc = acc + fma(a.y, a.y, t);
    }
  }
  const double sum = block_sum(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// scal[io] = op(sum partial[0..np))   op: 0 identity, 1 sqrt
__global__ void __launch_bounds__(256) lz_final(const double* __restrict__ partial, int np, double* __restrict__ scal, int io, int op) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < np; i += 256) acc += partial[i];
  const double sum = block_sum(acc);
  if (threadIdx.x == 0) scal[io] = op ? sqrt(sum) : sum;
}

// PROBE OVERLAPS (hxv_lanczos_tridiag_probes): partial sums of <p_j|x> = sum conj(p_j[i]) x[i] for the M probes of one run, x and every probe
// read once.  partial[block][2M]: (re, im) per probe.  REAL: the buffers are double[DimDw][pitch_real] viewed as double2 (see lz_len) -- two
// consecutive real elements per load, the sum has a real part only and the imaginary slot is written as zero.  The sums are written out
// (products rounded before they are added, one fused multiply-add per element) like lz_nrm's, so that every build adds the same numbers.
struct LzProbes {
  const double2* p[HXV_MAX_PROBES];
};
template <int M, bool REAL>
__global__ void __launch_bounds__(256) lz_probe_dots(int64_t n, const double2* __restrict__ x, LzProbes pr, double* __restrict__ partial) {
  double re[M], im[M];
#pragma unroll
  for (int j = 0; j < M; ++j) re[j] = im[j] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double2 a = x[i];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const double2 p = pr.p[j][i];
      {
#pragma clang fp contract(off)
        const double t = p.x * a.x;
        re[j] = re[j] + fma(p.y, a.y, t);
        if (!REAL) {
          const double u = p.x * a.y;
          im[j] = im[j] + fma(-p.y, a.x, u);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const double sr = block_sum(re[j]);
    __syncthreads();  // (block_sum's buffer is read by every thread: the next sum must not overwrite it before)
    double si = 0.0;
    if (!REAL) {
      si = block_sum(im[j]);
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      partial[(size_t)blockIdx.x * (2 * M) + 2 * j] = sr;
      partial[(size_t)blockIdx.x * (2 * M) + 2 * j + 1] = si;
    }
  }
}
// out[c] = sum over the np blocks, in block order, of partial[block][c], c < nc (one workgroup)
__global__ void __launch_bounds__(256) lz_probe_final(const double* __restrict__ partial, int np, int nc, double* __restrict__ out) {
  for (int c = 0; c < nc; ++c) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += 256) acc += partial[(size_t)i * nc + c];
    const double sum = block_sum(acc);
    __syncthreads();
    if (threadIdx.x == 0) out[c] = sum;
  }
}

// PROBE OVERLAPS OF A PAIRED RUN (hxv_lanczos_tridiag_pair_probes): x holds two real Lanczos vectors as (re, im) = (a, b), the M probes are
// REAL vectors on the complex slab's index (double[qdw][pitch], written once per call by lz_probe_real_pc), shared by both components.
// partial[block][2M]: (a_j, b_j) = partial sums of p_j * x.re and p_j * x.im.  One element per thread and iteration, each product rounded
// before it is added: with p.y = x.y = 0 lz_probe_dots<M, false> adds exactly these terms in this order (fma(0, 0, t) == t), so component a's
// sums carry the bits of the single run's complex path; 16 + 8M bytes per state where that kernel reads 16 + 16M.
struct LzRealProbes {
  const double* p[HXV_MAX_PROBES];
};
template <int M>
__global__ void __launch_bounds__(256) lz_probe_dots_pair(int64_t n, const double2* __restrict__ x, LzRealProbes pr, double* __restrict__ partial) {
  double ra[M], rb[M];
#pragma unroll
  for (int j = 0; j < M; ++j) ra[j] = rb[j] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double2 a = x[i];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const double p = pr.p[j][i];
      {
#pragma clang fp contract(off)
        const double t = p * a.x, u = p * a.y;
        ra[j] = ra[j] + t;
        rb[j] = rb[j] + u;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const double sa = block_sum(ra[j]);
    __syncthreads();  // (block_sum's buffer is read by every thread: the next sum must not overwrite it before)
    const double sb = block_sum(rb[j]);
    __syncthreads();
    if (threadIdx.x == 0) {
      partial[(size_t)blockIdx.x * (2 * M) + 2 * j] = sa;
      partial[(size_t)blockIdx.x * (2 * M) + 2 * j + 1] = sb;
    }
  }
}
// dst[i] = Re src[i] on the complex slab's own index (n = qdw * pitch elements: the index of the paired Lanczos vector), pad rows
// (row >= dimup) written as zero whatever the caller left there; partial = per-block sum of Im^2 over the rows below dimup.  Once per call
// and probe.
__global__ void __launch_bounds__(256) lz_probe_real_pc(int64_t n, int dimup, int pitch, const double2* __restrict__ src, double* __restrict__ dst,
                                                        double* __restrict__ partial) {
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(i % pitch);
    double re = 0.0;
    if (row < dimup) {
      const double2 z = src[i];
      re = z.x;
      acc += z.y * z.y;
    }
    dst[i] = re;
  }
  const double sum = block_sum(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// q = w / scal[ib]
__global__ void __launch_bounds__(256) lz_scale(int64_t n, double2* q, const double2* w,
                                                const double* __restrict__ scal, int ib) {
  const double r = 1.0 / scal[ib];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double2 x = w[i];
    q[i] = make_double2(x.x * r, x.y * r);
  }
}

// y += c * q   (c real, host scalar)
__global__ void __launch_bounds__(256) lz_axpy(int64_t n, double2* __restrict__ y, const double2* __restrict__ q, double c) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double2 x = q[i], z = y[i];
    y[i] = make_double2(z.x + c * x.x, z.y + c * x.y);
  }
}

// splitmix64 hash of x -> uniform(-0.5,0.5)
__device__ __forceinline__ double lz_uniform(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x = x ^ (x >> 31);
  return (double)(x >> 11) * (1.0 / 9007199254740992.0) - 0.5;
}

// deterministic start vector: the hash of the global index -> re and im
// (col0 = first global column of this rank's slab: a split sector starts from the same global vector as the unsplit one)
// (device row order, SectorHost::up_perm: the vector is defined on the REFERENCE index -- device row `row` holds reference row iperm[row],
//  times its basis sign -- so a sector starts from the same vector whatever order its rows are stored in)
__global__ void __launch_bounds__(256) lz_init(int64_t n, double2* __restrict__ q, uint64_t seed, int dimup, int pitch, int col0,
                                               const int32_t* __restrict__ iperm, const uint8_t* __restrict__ sign) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t lcol = i / pitch;
    const int row = (int)(i - lcol * pitch);
    const int64_t col = lcol + col0;
    if (row >= dimup) {  // pad rows stay zero: they must not enter the dot products
      q[i] = make_double2(0.0, 0.0);
      continue;
    }
    const int rrow = iperm ? iperm[row] : row;
    const double sgn = (sign && sign[row]) ? -1.0 : 1.0;
    const uint64_t z = (uint64_t)(col * dimup + rrow) * 2 + seed;
    q[i] = make_double2(sgn * lz_uniform(z), sgn * lz_uniform(z + 1));
  }
}

int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, RED_BLOCKS)); }  // (never an empty grid: a rank may own no column)

// ---- REAL-vector mode: layout conversions and the real start vector ----------------------------------------------
// real [DimDw][pr] <- Re(complex [DimDw][pc]); pads zero.  partial = per-block sum of Im^2 (may be null)
__global__ void __launch_bounds__(256) lz_to_real(int dimup, int dimdw, int pc, int pr, const double2* __restrict__ src,
                                                  double* __restrict__ dst, double* __restrict__ partial) {
  const int64_t n = (int64_t)dimdw * pr;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t col = i / pr;
    const int row = (int)(i - col * pr);
    double x = 0.0;
    if (row < dimup) {
      const double2 z = src[col * pc + row];
      x = z.x;
      acc += z.y * z.y;
    }
    if (dst) dst[i] = x;
  }
  const double sum = block_sum(acc);
  if (threadIdx.x == 0 && partial) partial[blockIdx.x] = sum;
}

// complex [DimDw][pc] <- real [DimDw][pr]; pads zero
__global__ void __launch_bounds__(256) lz_to_complex(int dimup, int dimdw, int pc, int pr, const double* __restrict__ src,
                                                     double2* __restrict__ dst) {
  const int64_t n = (int64_t)dimdw * pc;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t col = i / pc;
    const int row = (int)(i - col * pc);
    dst[i] = make_double2(row < dimup ? src[col * pr + row] : 0.0, 0.0);
  }
}

// real start vector: the real part of lz_init's vector
__global__ void __launch_bounds__(256) lz_init_real(int64_t n, double* __restrict__ q, uint64_t seed, int dimup, int pitch, int col0,
                                                    const int32_t* __restrict__ iperm, const uint8_t* __restrict__ sign) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t lcol = i / pitch;
    const int row = (int)(i - lcol * pitch);
    const int64_t col = lcol + col0;  // global column: a split sector starts from the same global vector as the unsplit one
    if (row >= dimup) {
      q[i] = 0.0;
      continue;
    }
    const int rrow = iperm ? iperm[row] : row;
    const double r = lz_uniform((uint64_t)(col * dimup + rrow) * 2 + seed);
    q[i] = (sign && sign[row]) ? -r : r;
  }
}

// scal[i] = scal[a] * scal[b]
__global__ void lz_mul(double* scal, int i, int a, int b) { scal[i] = scal[a] * scal[b]; }
// scal[i] = sqrt(scal[i])   (split sector: the square root comes after the all-reduce of the partial sums of squares)
__global__ void lz_sqrt(double* scal, int i) { scal[i] = sqrt(scal[i]); }

// End of one fused iteration without the host: record alpha_k, beta_{k+1} at the device-side step counter scal[LZ_STEP], and prepare the
// next iteration's scalars  s = 1/beta_{k+1},  c = s_old/s = beta_{k+1}/beta_k.
__global__ void lz_next(double* scal, double* alpha_out, double* beta_out, int nmax) {
  const int k = (int)scal[LZ_STEP];
  if (k < nmax) {
    alpha_out[k] = scal[LZ_ALPHA];
    if (k + 1 < nmax) beta_out[k + 1] = scal[LZ_BETA];
  }
  // (the same operations, in the same order, as LzScale::next() + c() on the host: bit-identical recurrences)
  const double beta_prev = 1.0 / scal[LZ_S], s_new = 1.0 / scal[LZ_BETA];
  scal[LZ_S] = s_new;
  scal[LZ_C] = 1.0 / (s_new * beta_prev);
  scal[LZ_STEP] = (double)(k + 1);
}

// THE dispatch on a number of probes known at run time: f(std::integral_constant<int, M>{}) for M = m when LO <= m <= HXV_MAX_PROBES, nothing
// otherwise (the launchers below and of the Chebyshev headers then launch their final kernel alone).  LO: 1 for kernels that need a probe, 0
// for those that run without.
template <int LO, int M = LO, typename F>
void with_probe_count(int m, F&& f) {
  if (m == M)
    f(std::integral_constant<int, M>{});
  else if constexpr (M < HXV_MAX_PROBES)
    with_probe_count<LO, M + 1>(m, f);
}

// out[2*j], out[2*j+1] = Re, Im <p_j|x> of this rank's share (n double2 elements), j < m: one pass over x and the probes on g workgroups, then
// one workgroup that adds the block partials in block order.  d_part: g * 2m doubles.  (The drivers pass g = grid_for(n) and the handle's
// stream: LzProbeSet::enqueue of hxv_lanczos.hip.)
template <bool REAL>
void launch_probe_dots(int g, hipStream_t st, int m, int64_t n, const double2* x, const LzProbes& pr, double* d_part, double* d_out) {
  with_probe_count<1>(m, [&](auto M) { hipLaunchKernelGGL((lz_probe_dots<M(), REAL>), dim3(g), dim3(256), 0, st, n, x, pr, d_part); });
  hipLaunchKernelGGL(lz_probe_final, dim3(1), dim3(256), 0, st, d_part, g, 2 * m, d_out);
}
// out[2*j], out[2*j+1] = <p_j|Re x>, <p_j|Im x> of this rank's share for the m REAL probes of a paired run: lz_probe_dots_pair<m> on g workgroups,
// then lz_probe_final as above.  d_part: g * 2m doubles.
inline void launch_probe_dots_pair(int g, hipStream_t st, int m, int64_t n, const double2* x, const LzRealProbes& pr, double* d_part, double* d_out) {
  with_probe_count<1>(m, [&](auto M) { hipLaunchKernelGGL((lz_probe_dots_pair<M()>), dim3(g), dim3(256), 0, st, n, x, pr, d_part); });
  hipLaunchKernelGGL(lz_probe_final, dim3(1), dim3(256), 0, st, d_part, g, 2 * m, d_out);
}

}  // namespace
