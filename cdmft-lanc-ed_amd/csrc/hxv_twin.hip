// Twin-sector map of a device-resident state (include/hxv.h: hxv_twin_vector).
//
// With ed_twin the reference solves one sector of every pair A = (nup,ndw), B = (ndw,nup) (ED_SETUP.f90:353-362), stores each eigenstate once
// with a twin link (ED_DIAG.f90:84,231) and rebuilds B's vector on demand, vector(i) = cvec(Order(i)) (es_return_cvector,
// ED_EIGENSPACE.f90:485-494).  Order (twin_sector_order, ED_SETUP.f90:854-898) is the argsort of the spin-flipped Fock states; with A's index
// iup + idw*DimUp_A and B's iup' + idw'*DimUp_B, iup' = idw, idw' = iup, that is the plain transpose of the DimUp x DimDw amplitude matrix,
//     v_B[idw_A + iup_A*DimDw_A] = v_A[iup_A + idw_A*DimUp_A],
// without a sign.  On device vectors (columns padded to the pitch, rows in each sector's device row order, basis signs by device row):
//     d_B[kB*pitch_B + rB] = sB[rB] * sA[rA] * d_A[kA*pitch_A + rA],     kB = iperm_A[rA],  kA = iperm_B[rB].
//   twin_transpose_kernel  one workgroup per tile of TW device rows of A by TW device rows of B, through LDS.  A tile row of the load is a
//                      run of TW elements inside ONE column of A (column iperm_B[rB]), a tile row of the store a run of TW elements inside
//                      ONE column of B (column iperm_A[rA]): both sides move whole 128-byte lines (TW and both pitches are multiples of 8),
//                      whatever the two row orders are.  Pad rows of d_A are never read; every element of d_B is written, its pad rows with
//                      zeros (the last tile along rB reaches pitch_B).  Only moves and +-1: the same input gives the same bits.
#include <hip/hip_runtime.h>

#include "hxv_handle.hpp"

using namespace hxv;

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
}  // namespace

extern "C" {

int hxv_twin_vector(hxv_handle* from, hxv_handle* to, const void* d_psi, void* d_out) {
  if (!from || !to || !d_psi || !d_out) return fail(HXV_ERR_ARG, "hxv_twin_vector: NULL argument");
  const SectorHost &a = from->host, &b = to->host;
  if (a.map_up.empty() || a.map_dw.empty() || b.map_up.empty() || b.map_dw.empty() || a.panel_rows > 0 || b.panel_rows > 0)
    return fail(HXV_ERR_STATE, "hxv_twin_vector needs handles built from a model (basis maps)");
  if (from->device != to->device) return fail(HXV_ERR_ARG, "hxv_twin_vector: handles on different devices");
  if (d_out == d_psi) return fail(HXV_ERR_ARG, "hxv_twin_vector: d_out must not be d_psi (the map is not done in place)");
  if (a.nranks > 1 || b.nranks > 1 || comm_ready(from) || comm_ready(to))
    return fail(HXV_ERR_UNSUPPORTED, "hxv_twin_vector: split sectors are not supported (the twin of a DimDw split is a DimUp split: an all-to-all)");
  if (a.ns != b.ns || b.nup != a.ndw || b.ndw != a.nup || b.dimup != a.dimdw || b.dimdw != a.dimup)
    return fail(HXV_ERR_ARG, "hxv_twin_vector: `to` is not the twin sector (ndw,nup) of `from`");
  HIPCHK(hipSetDevice(to->device));
  hipStream_t st = to->stream;
  const unsigned gx = (unsigned)((a.dimup + TW - 1) / TW), gy = (unsigned)((b.pitch + TW - 1) / TW);
  if (gy > 65535u) return fail(HXV_ERR_UNSUPPORTED, "hxv_twin_vector: more than 65535 tiles along the target's rows");
  hipLaunchKernelGGL(twin_transpose_kernel, dim3(gx, gy), dim3(TW_THREADS), 0, st, (const double2*)d_psi, a.dimup, a.pitch, from->dev.up_iperm,
                     from->dev.up_sign, (double2*)d_out, b.dimup, b.pitch, to->dev.up_iperm, to->dev.up_sign);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("twin kernel: ") + hipGetErrorString(e));
  HIPCHK(hipStreamSynchronize(st));
  return HXV_OK;
}

}  // extern "C"
