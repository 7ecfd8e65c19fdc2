// The streaming vector kernels of hxv_eigh_lowest (hxv_eigh.hip) and the two launchers that dispatch on the basis size.
// They live in a header of their own so that tests/device/eigh_kernels_check.hip can launch each of them alone, with a stride, a grid and
// shapes the driver never passes; the product includes this file from hxv_eigh.hip only.  Everything stays in an anonymous namespace:
// each including file gets its own copy, with internal linkage, exactly as when the text stood in hxv_eigh.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int JB = 8;       // basis vectors per multi-dot pass (w is re-read once per JB vectors)
constexpr int TR_BLOCKS = 4096;  // workgroups of the streaming kernels (16 per CU)
constexpr int MAXCV = 64;   // largest Krylov basis (the rotation keeps one element of every vector in registers)

__device__ inline double wave_sum(double x) {
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

// partial[blockIdx][2*j..2*j+1] = sum_i conj(V_j[i]) * w[i]   for j < nb (nb <= JB)
__global__ void __launch_bounds__(256) tr_mdot(int64_t n, const double2* __restrict__ V, int64_t stride, int nb,
                                               const double2* __restrict__ w, double* __restrict__ partial) {
  double re[JB], im[JB];
#pragma unroll
  for (int j = 0; j < JB; ++j) re[j] = im[j] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double2 x = w[i];
#pragma unroll
    for (int j = 0; j < JB; ++j)
      if (j < nb) {
        const double2 y = V[(int64_t)j * stride + i];
        re[j] += y.x * x.x + y.y * x.y;
        im[j] += y.x * x.y - y.y * x.x;
      }
  }
  __shared__ double red[4][2 * JB];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < JB; ++j) {
    const double a = wave_sum(re[j]), b = wave_sum(im[j]);
    if (lane == 0) {
      red[wave][2 * j] = a;
      red[wave][2 * j + 1] = b;
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * JB)
    partial[(int64_t)blockIdx.x * 2 * JB + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// out[t] = sum_b partial[b][t]  (t < nval), partial rows of `ld` values
__global__ void __launch_bounds__(256) tr_colsum(const double* __restrict__ partial, int nblocks, int ld, int nval, double* __restrict__ out,
                                                 int zero_odd) {
  __shared__ double red[256];
  for (int t = 0; t < nval; ++t) {
    if (zero_odd && (t & 1)) {  // REAL-vector mode: the "imaginary parts" of the reinterpreted dot products are not coefficients
      if (threadIdx.x == 0) out[t] = 0.0;
      continue;
    }
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) acc += partial[(int64_t)b * ld + t];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[t] = red[0];
    __syncthreads();
  }
}

// w -= sum_{j<nj} c_j V_{idx[j]} ; partial[blockIdx] = sum |w|^2
__global__ void __launch_bounds__(256) tr_maxpy(int64_t n, const double2* __restrict__ V, int64_t stride, int nj, const int* __restrict__ idx,
                                                const double* __restrict__ coef, double2* __restrict__ w, double* __restrict__ partial) {
  __shared__ double sc[2 * (MAXCV + 1)];
  __shared__ int sidx[MAXCV + 1];
  for (int t = threadIdx.x; t < 2 * nj; t += 256) sc[t] = coef[t];
  for (int t = threadIdx.x; t < nj; t += 256) sidx[t] = idx[t];
  __syncthreads();
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    double2 x = w[i];
#pragma unroll 4
    for (int j = 0; j < nj; ++j) {
      const double2 y = V[(int64_t)sidx[j] * stride + i];
      const double cr = sc[2 * j], ci = sc[2 * j + 1];
      x.x -= cr * y.x - ci * y.y;
      x.y -= cr * y.y + ci * y.x;
    }
    w[i] = x;
    acc += x.x * x.x + x.y * x.y;
  }
  __shared__ double red[4];
  const double a = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// x *= r ; also usable for the norm alone (r == 1 skips the store)
__global__ void __launch_bounds__(256) tr_scale_nrm(int64_t n, double2* __restrict__ x, double r, double* __restrict__ partial) {
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    double2 a = x[i];
    acc += a.x * a.x + a.y * a.y;
    if (r != 1.0) x[i] = make_double2(a.x * r, a.y * r);
  }
  __shared__ double red[4];
  const double a = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0 && partial) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// In-place basis rotation  V[:, 0..k) <- V[:, 0..m) * S  (S real m x k, column-major S[l + j*m]).
// Each thread keeps one element of all m vectors in registers, so every vector is read once and the
// first k are written once: (m + k) vector passes instead of m*k.
template <int MAXM>
__global__ void __launch_bounds__(256) tr_rotate(int64_t n, double2* __restrict__ V, int64_t stride, int m, int k,
                                                 const double* __restrict__ S) {
  __shared__ double sS[MAXM * MAXM];
  for (int t = threadIdx.x; t < m * k; t += 256) sS[t] = S[t];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    double2 x[MAXM];
#pragma unroll
    for (int l = 0; l < MAXM; ++l)
      if (l < m) x[l] = V[(int64_t)l * stride + i];
    for (int j = 0; j < k; ++j) {
      double yr = 0.0, yi = 0.0;
#pragma unroll
      for (int l = 0; l < MAXM; ++l)
        if (l < m) {
          const double s = sS[l + j * m];
          yr += s * x[l].x;
          yi += s * x[l].y;
        }
      V[(int64_t)j * stride + i] = make_double2(yr, yi);
    }
  }
}

void launch_rotate(int grid, hipStream_t st, int64_t n, double2* V, int64_t stride, int m, int k, const double* S) {
  if (m <= 8)
    hipLaunchKernelGGL(tr_rotate<8>, dim3(grid), dim3(256), 0, st, n, V, stride, m, k, S);
  else if (m <= 16)
    hipLaunchKernelGGL(tr_rotate<16>, dim3(grid), dim3(256), 0, st, n, V, stride, m, k, S);
  else if (m <= 32)
    hipLaunchKernelGGL(tr_rotate<32>, dim3(grid), dim3(256), 0, st, n, V, stride, m, k, S);
  else
    hipLaunchKernelGGL(tr_rotate<MAXCV>, dim3(grid), dim3(256), 0, st, n, V, stride, m, k, S);
}

// First step of a restart cycle, one pass instead of two: x = a*w - sum_{l<nv} c_l V_l (the arrow of T taken out with its KNOWN coefficients;
// c_l = 0 for vectors that are only measured), stored back to w, and partial[blockIdx][2l..2l+1] = sum_i conj(V_l[i]) x[i] for all l < nv --
// the measurement the following Gram-Schmidt pass needs.  Every V_l[i] is loaded once for both.  nv <= NJ.
template <int NJ>
__global__ void __launch_bounds__(256) tr_axpy_mdot(int64_t n, const double2* __restrict__ V, int64_t stride, int nv, const double* __restrict__ coef,
                                                    double a, double2* __restrict__ w, double* __restrict__ partial) {
  __shared__ double sc[NJ];
  if ((int)threadIdx.x < NJ) sc[threadIdx.x] = (int)threadIdx.x < nv ? coef[threadIdx.x] : 0.0;
  __syncthreads();
  double re[NJ], im[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) re[j] = im[j] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    double2 y[NJ];
    double2 x = w[i];
    x.x *= a;
    x.y *= a;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (j < nv) {
        y[j] = V[(int64_t)j * stride + i];
        x.x -= sc[j] * y[j].x;
        x.y -= sc[j] * y[j].y;
      }
    w[i] = x;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (j < nv) {
        re[j] += y[j].x * x.x + y[j].y * x.y;
        im[j] += y[j].x * x.y - y[j].y * x.x;
      }
  }
  __shared__ double red[4][2 * NJ];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const double p = wave_sum(re[j]), q = wave_sum(im[j]);
    if (lane == 0) {
      red[wave][2 * j] = p;
      red[wave][2 * j + 1] = q;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * NJ)
    partial[(int64_t)blockIdx.x * 2 * NJ + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// The restart rotation (tr_rotate) that also brings the residual vector r = V[m] to its new place V[k] and measures it against the k new
// Ritz vectors as they are formed: partial[blockIdx][2j..2j+1] = sum_i conj(y_j[i]) r[i].  Replaces rotation + copy + one multi-dot pass.  k <= KD.
template <int MAXM, int KD>
__global__ void __launch_bounds__(256) tr_rotate_dots(int64_t n, double2* __restrict__ V, int64_t stride, int m, int k, const double* __restrict__ S,
                                                      double* __restrict__ partial) {
  __shared__ double sS[MAXM * KD];
  for (int t = threadIdx.x; t < m * k; t += 256) sS[t] = S[t];
  __syncthreads();
  double re[KD], im[KD];
#pragma unroll
  for (int j = 0; j < KD; ++j) re[j] = im[j] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    double2 x[MAXM];
#pragma unroll
    for (int l = 0; l < MAXM; ++l)
      if (l < m) x[l] = V[(int64_t)l * stride + i];
    const double2 r = V[(int64_t)m * stride + i];
#pragma unroll
    for (int j = 0; j < KD; ++j)
      if (j < k) {
        double yr = 0.0, yi = 0.0;
#pragma unroll
        for (int l = 0; l < MAXM; ++l)
          if (l < m) {
            const double sv = sS[l + j * m];
            yr += sv * x[l].x;
            yi += sv * x[l].y;
          }
        V[(int64_t)j * stride + i] = make_double2(yr, yi);
        re[j] += yr * r.x + yi * r.y;
        im[j] += yr * r.y - yi * r.x;
      }
    V[(int64_t)k * stride + i] = r;
  }
  __shared__ double red[4][2 * KD];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < KD; ++j) {
    const double p = wave_sum(re[j]), q = wave_sum(im[j]);
    if (lane == 0) {
      red[wave][2 * j] = p;
      red[wave][2 * j + 1] = q;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * KD)
    partial[(int64_t)blockIdx.x * 2 * KD + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

constexpr int FUSE_NJ = 16;  // most vectors the two fused restart kernels handle (larger kept sets take the separate passes)

bool launch_rotate_dots(int grid, hipStream_t st, int64_t n, double2* V, int64_t stride, int m, int k, const double* S, double* partial) {
  if (k > FUSE_NJ) return false;
  if (m <= 8)
    hipLaunchKernelGGL((tr_rotate_dots<8, FUSE_NJ>), dim3(grid), dim3(256), 0, st, n, V, stride, m, k, S, partial);
  else if (m <= 16)
    hipLaunchKernelGGL((tr_rotate_dots<16, FUSE_NJ>), dim3(grid), dim3(256), 0, st, n, V, stride, m, k, S, partial);
  else if (m <= 32)
    hipLaunchKernelGGL((tr_rotate_dots<32, FUSE_NJ>), dim3(grid), dim3(256), 0, st, n, V, stride, m, k, S, partial);
  else
    hipLaunchKernelGGL((tr_rotate_dots<MAXCV, FUSE_NJ>), dim3(grid), dim3(256), 0, st, n, V, stride, m, k, S, partial);
  return true;
}

}  // namespace
