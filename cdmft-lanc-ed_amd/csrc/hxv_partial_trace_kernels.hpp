// The device code of the partial-trace engine (hxv_partial_trace.hip) and the host routine that scatters its class blocks: text moved out of
// that file unchanged, so that tests/device/partial_trace_kernels_check.hip can launch each kernel alone on tables of its own making
// (tests/test_gpu_partial_trace_kernels.py).  The tables are those of hxv_partial_trace_host.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>

#include "hxv_partial_trace_host.hpp"

namespace {
using namespace hxv;

constexpr int PT_LOADS = 4;  // 16-byte loads a thread has in flight while staging

// src: the column slots the dw groups name ([nranks*cmax][pitch] gathered copy, or this rank's slab itself); pad rows are never read.
// One thread per pair of a class with n <= 4; component k = iu + du*id of the pair is x[k], components past n are zero.
__global__ void __launch_bounds__(PT_THREADS) pt_pair_kernel(const double2* __restrict__ src, int pitch, const PtClass* __restrict__ cls,
                                                             const PtItem* __restrict__ items, const uint32_t* __restrict__ rows,
                                                             const uint32_t* __restrict__ cols, const uint32_t* __restrict__ tiles,
                                                             double2* __restrict__ partial) {
  constexpr int N = PT_PAIR_N;
  __shared__ double2 red[PT_THREADS / 64][N * N];
  const PtItem it = items[blockIdx.x];
  const PtClass c = cls[it.cls];
  const int tid = threadIdx.x;
  const uint32_t* __restrict__ crow = rows + c.rows_off;
  const uint32_t* __restrict__ ccol = cols + c.cols_off;
  double2 acc[N][N];  // the upper triangle is used
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) acc[i][j] = make_double2(0.0, 0.0);
  for (int base = it.p0; base < it.p1; base += PT_THREADS) {
    const int p = base + tid;
    if (p < it.p1) {
      const int gd = p / c.ngu, g = p - gd * c.ngu;
      uint32_t sg[N];
      double2 x[N];
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const int kk = min(k, c.n - 1);  // past the block: a repeated load, zeroed below
        const uint32_t r = crow[g * c.du + kk % c.du], cc = ccol[gd * c.dd + kk / c.du];
        sg[k] = (r ^ cc) >> 31;
        x[k] = src[(int64_t)(cc & 0x7fffffffu) * pitch + (int64_t)(r & 0x7fffffffu)];
      }
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const double f = k < c.n ? (sg[k] ? -1.0 : 1.0) : 0.0;
        x[k] = make_double2(f * x[k].x, f * x[k].y);
      }
#pragma unroll
      for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j) {
          acc[i][j].x += x[i].x * x[j].x + x[i].y * x[j].y;  // x_i * conj(x_j)
          acc[i][j].y += x[i].y * x[j].x - x[i].x * x[j].y;
        }
    }
  }
  // the workgroup's sum in a fixed order: xor butterfly inside each wave (every lane ends with the same bits), then wave 0, 1, 2, 3
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = i; j < N; ++j) {
      double re = acc[i][j].x, im = acc[i][j].y;
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        re += __shfl_xor(re, m, 64);
        im += __shfl_xor(im, m, 64);
      }
      if ((tid & 63) == 0) red[tid >> 6][i * N + j] = make_double2(re, im);
    }
  __syncthreads();
  if (tid < c.ntiles * 4) {  // (a pair-kernel class has 2 x 2 tiles)
    const uint32_t pk = tiles[c.tile_off + (tid >> 2)];
    const int i = (int)(pk & 0xffffu) * 2 + ((tid >> 1) & 1), j = (int)(pk >> 16) * 2 + (tid & 1);
    double2 v = make_double2(0.0, 0.0);
    if (i <= j && j < N)
      for (int w = 0; w < PT_THREADS / 64; ++w) {
        v.x += red[w][i * N + j].x;
        v.y += red[w][i * N + j].y;
      }
    partial[it.out_off + tid] = v;
  }
}

template <int T, int NT>
__global__ void __launch_bounds__(PT_THREADS) pt_tile_kernel(const double2* __restrict__ src, int pitch, const PtClass* __restrict__ cls,
                                                             const PtItem* __restrict__ items, const uint32_t* __restrict__ rows,
                                                             const uint32_t* __restrict__ cols, const uint32_t* __restrict__ tiles,
                                                             double2* __restrict__ partial) {
  __shared__ double2 xs[PT_XS];
  const PtItem it = items[blockIdx.x];
  const PtClass c = cls[it.cls];
  const int tid = threadIdx.x;
  // this thread's tiles: LDS offsets of their T row and T column components (indices past the block edge repeat the last component: those
  // elements are computed, stored and never used)
  int offi[NT][T], offj[NT][T];
  bool live[NT];
  double2 acc[NT][T][T];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int tile = (c.nrep > 1 ? (tid & 63) : tid) + t * PT_THREADS;
    live[t] = tile < c.ntiles;
    const uint32_t pk = tiles[c.tile_off + (live[t] ? tile : 0)];
    const int ti = (int)(pk & 0xffffu), tj = (int)(pk >> 16);
#pragma unroll
    for (int a = 0; a < T; ++a) {
      const int i = min(ti * T + a, c.n - 1), j = min(tj * T + a, c.n - 1);
      offi[t][a] = (i / c.du) * c.stride + (i % c.du);
      offj[t][a] = (j / c.du) * c.stride + (j % c.du);
#pragma unroll
      for (int b = 0; b < T; ++b) acc[t][a][b] = make_double2(0.0, 0.0);
    }
  }
  const uint32_t* __restrict__ crow = rows + c.rows_off;
  const uint32_t* __restrict__ ccol = cols + c.cols_off;
  const int gd0 = it.p0 / c.ngu, gd1 = (it.p1 - 1) / c.ngu;
  for (int gd = gd0; gd <= gd1; ++gd) {
    const int lo = gd == gd0 ? it.p0 - gd0 * c.ngu : 0, hi = gd == gd1 ? it.p1 - gd1 * c.ngu : c.ngu;
    for (int g0 = lo; g0 < hi; g0 += c.batch) {
      const int bc = min(c.batch, hi - g0), nk = bc * c.du;
      __syncthreads();
      for (int k0 = 0; k0 < nk; k0 += PT_THREADS) {
        const int k = k0 + tid;  // k = b * du + iu: the position in the row table and in the staging area
        if (k < nk) {
          const uint32_t r = crow[g0 * c.du + k];
          const int64_t row = (int64_t)(r & 0x7fffffffu);
          for (int id0 = 0; id0 < c.dd; id0 += PT_LOADS) {
            double2 x[PT_LOADS];
            uint32_t sg[PT_LOADS];
#pragma unroll
            for (int u = 0; u < PT_LOADS; ++u) {
              const uint32_t cc = ccol[gd * c.dd + min(id0 + u, c.dd - 1)];
              sg[u] = (r ^ cc) >> 31;
              x[u] = src[(int64_t)(cc & 0x7fffffffu) * pitch + row];
            }
#pragma unroll
            for (int u = 0; u < PT_LOADS; ++u)
              if (id0 + u < c.dd) {
                const double f = sg[u] ? -1.0 : 1.0;
                xs[(id0 + u) * c.stride + k] = make_double2(f * x[u].x, f * x[u].y);
              }
          }
        }
      }
      __syncthreads();
      if (!live[0]) continue;  // a thread without a first tile has no further one: a wave of them skips the loop (the barriers are behind it)
      for (int b = c.nrep > 1 ? (tid >> 6) : 0; b < bc; b += c.nrep) {
        const int o = b * c.du;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if (t > 0 && !live[t]) continue;
          double2 xi[T], xj[T];
#pragma unroll
          for (int a = 0; a < T; ++a) {
            xi[a] = xs[offi[t][a] + o];
            xj[a] = xs[offj[t][a] + o];
          }
#pragma unroll
          for (int a = 0; a < T; ++a)
#pragma unroll
            for (int q = 0; q < T; ++q) {
              acc[t][a][q].x += xi[a].x * xj[q].x + xi[a].y * xj[q].y;  // x_i * conj(x_j)
              acc[t][a][q].y += xi[a].y * xj[q].x - xi[a].x * xj[q].y;
            }
        }
      }
    }
  }
  double2* __restrict__ out = partial + it.out_off + (c.nrep > 1 ? (int64_t)(tid >> 6) * c.ntiles * (T * T) : 0);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int tile = (c.nrep > 1 ? (tid & 63) : tid) + t * PT_THREADS;
    if (!live[t]) continue;
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
      for (int q = 0; q < T; ++q) out[(int64_t)tile * (T * T) + a * T + q] = acc[t][a][q];
  }
}

// out[e] = the partial blocks' element, summed in work-list order (cnt may be 0: a rank without dw groups of the class)
__global__ void __launch_bounds__(PT_THREADS) pt_reduce_kernel(const double2* __restrict__ partial, const int64_t* __restrict__ el_src,
                                                               const int32_t* __restrict__ el_cnt, const int32_t* __restrict__ el_stride,
                                                               int64_t nel, double2* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x;
  if (e >= nel) return;
  const double2* __restrict__ p = partial + el_src[e];
  const int n = el_cnt[e];
  const int64_t st = el_stride[e];
  double2 acc = make_double2(0.0, 0.0);
  for (int k = 0; k < n; ++k) {
    const double2 v = p[k * st];
    acc.x += v.x;
    acc.y += v.y;
  }
  out[e] = acc;
}

// class blocks -> the dense matrix, element (io,jo) at 2*(io + 4^nsub*jo); weight * raw is rounded before it is added, so that an
// accumulated matrix equals the sum of the single results bit for bit
void scatter(const PtHostTables& t, const std::vector<double2>& raw, double weight, bool accumulate, double* rho) {
#pragma clang fp contract(off)
  const int64_t nn = (int64_t)1 << (2 * t.nsub);
  if (!accumulate) std::memset(rho, 0, (size_t)(2 * nn * nn) * sizeof(double));
  for (size_t ci = 0; ci < t.cls.size(); ++ci) {
    const PtClass& c = t.cls[ci];
    const PtClassHost& h = t.hcls[ci];
    auto orb = [&](int i) -> int64_t { return (int64_t)h.au[i % c.du] + ((int64_t)h.ad[i / c.du] << t.nsub); };
    for (int tile = 0; tile < c.ntiles; ++tile) {
      const int ti = (int)(h.tiles[tile] & 0xffffu), tj = (int)(h.tiles[tile] >> 16);
      for (int a = 0; a < c.t; ++a)
        for (int q = 0; q < c.t; ++q) {
          const int i = ti * c.t + a, j = tj * c.t + q;
          if (i > j || j >= c.n) continue;
          const double2 v = raw[(size_t)(h.out_off + (int64_t)tile * c.t * c.t + a * c.t + q)];
          const double re = weight * v.x, im = i == j ? 0.0 : weight * v.y;
          const int64_t io = orb(i), jo = orb(j);
          rho[2 * (io + nn * jo)] += re;
          rho[2 * (io + nn * jo) + 1] += im;
          if (i != j) {
            rho[2 * (jo + nn * io)] += re;
            rho[2 * (jo + nn * io) + 1] -= im;
          }
        }
    }
  }
}
}  // namespace
