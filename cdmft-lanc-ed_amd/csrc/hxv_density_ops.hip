// Density-type operators on a device-resident state (include/hxv.h: hxv_apply_density_ops): the start vectors of the two-particle stage.
//
// O_a = sum_is (cu_a[is] n_is,up + cd_a[is] n_is,dw) over the Nimp impurity orbitals is diagonal in the Fock basis: on the basis state
// (iup, idw) it is the number  f_a = fu_a(o_up) + fd_a(o_dw),  o_s = the low Nimp bits of that spin's configuration.  S^z_i, n_i, n_i,s and
// every total or staggered combination of them are of this kind, and  out_a = (f_a - m_a) psi,  m_a = <psi|O_a|psi> / <psi|psi>,  is the start
// vector (and the probe) of the spin / charge susceptibility chi_ab (the reference's buildChi_impurity, ED_GREENS_FUNCTIONS.f90:68-106).
// Tables (built on the host, kept with the sector image): one 32-bit impurity-occupation word per DEVICE row and one per local column.  A
// diagonal operator keeps the row, and the basis sign of a device row multiplies psi and out alike: only the occupation lookup goes through
// the device row order.
// Kernels, 256 threads, a work item = (local column, chunk of its rows), item i on workgroup i mod gridDim:
//   dop_sums_kernel    pass 1: reads psi once (16-byte loads), per workgroup the partial sums of  f_a |psi|^2  (a < nops) and of |psi|^2.
//   dop_apply_kernel   pass 2: reads psi once, writes the nops vectors (16-byte stores; the pad rows of every column as zero) and per
//                      workgroup the partial sums of |out_a|^2.  Pad rows of psi are never read by either pass.
//   dop_reduce_kernel  one workgroup per sum: the workgroups' partials, strided over its threads, then a fixed-order tree.
// f is looked up, not summed per element: every workgroup first writes fu_a and fd_a of the two 5-bit halves of an occupation word into LDS
// (2 spins x 2 halves x 8 operators x 32 entries, 8 KB), so that f_a costs the element two LDS reads and an add per spin however large Nimp
// is, and fd_a is read once per work item.  No floating-point atomics, the work list is a function of the sector and the device alone: the
// same inputs give the same bits on every call.  On a split sector every rank works on its slab, and the sums of a pass are all-reduced at once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "hxv_call_scope.hpp"

using namespace hxv;

namespace {
struct DopTables : DeviceTables {
  uint32_t *occ_up = nullptr, *occ_dw = nullptr;  // [pitch] by device row (pad rows 0), [max(qdw,1)] by local column
  int nchunk = 1, rows = 0;                       // chunks a column is cut into, rows of a chunk (a multiple of 8)
  int64_t nitems = 0;
  int grid = 1;                                   // workgroups of the two passes
};
constexpr int DOP_THREADS = 256;
constexpr int DOP_WAVES = DOP_THREADS / 64;
constexpr int DOP_MAX = HXV_MAX_DENSITY_OPS;
constexpr int DOP_NSUM = DOP_MAX + 1;  // partial sums a workgroup writes: one per operator slot, then (pass 1) the norm at index DOP_MAX
constexpr int DOP_MAX_NIMP = 10;       // two 5-bit halves
constexpr int DOP_UNROLL = 4;          // 16-byte loads a thread has in flight
constexpr int DOP_CHUNK = 2048;        // rows of a work item, at most
constexpr int DOP_WG_PER_CU = 8;

struct DopShape {
  int dimup, pitch, qdw, nimp, nops, nchunk, rows;
  int64_t nitems;
};
struct DopOut {
  double2* v[DOP_MAX];
  double m[DOP_MAX];  // what is subtracted from f_a: the mean, or 0
};

std::string build_tables(const SectorHost& s, int nimp, int device, int ncu, DopTables& t) {
  const uint32_t mask = (1u << nimp) - 1u;
  t.device = device;
  const std::vector<uint32_t>& mdev = s.dev_map_up();  // reference bit strings by device row
  std::vector<uint32_t> ou((size_t)s.pitch, 0u), od((size_t)std::max(s.qdw, 1), 0u);
  for (int r = 0; r < s.dimup; ++r) ou[r] = mdev[r] & mask;
  for (int c = 0; c < s.qdw; ++c) od[c] = s.map_dw[s.dw0 + c] & mask;
  t.nchunk = std::max(1, (s.pitch + DOP_CHUNK - 1) / DOP_CHUNK);
  t.rows = (((s.pitch + t.nchunk - 1) / t.nchunk) + 7) & ~7;
  t.nitems = (int64_t)std::max(s.qdw, 0) * t.nchunk;
  if (t.nitems >= INT32_MAX) return "density operators: too many work items";
  t.grid = (int)std::max<int64_t>(1, std::min<int64_t>(t.nitems, (int64_t)DOP_WG_PER_CU * ncu));
  TableArena ar;
  (void)ar.add(ou, &t.occ_up);
  (void)ar.add(od, &t.occ_dw);
  hipError_t e = ar.commit(&t.base, &t.bytes);
  if (e != hipSuccess) return std::string("density operators tables: ") + hipGetErrorString(e);
  return std::string();
}

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

extern "C" {

int hxv_apply_density_ops(hxv_handle* h, int32_t nops, const double* coef, int32_t subtract_mean, const void* d_psi, void* const* d_out,
                          double* mean, double* norm2) {
  if (!h) return fail(HXV_ERR_ARG, "hxv_apply_density_ops: NULL handle");
  const SectorHost& s = h->host;
  if (s.map_up.empty() || s.map_dw.empty() || s.panel_rows > 0)
    return fail(HXV_ERR_STATE, "hxv_apply_density_ops needs a handle built from a model (basis maps)");
  const int nimp = nimp_of(s);
  if (nimp < 1 || nimp > s.ns) return fail(HXV_ERR_STATE, "hxv_apply_density_ops: the handle carries no impurity size");
  if (nimp > DOP_MAX_NIMP) return fail(HXV_ERR_UNSUPPORTED, "hxv_apply_density_ops: Nimp > 10");
  const bool split = s.nranks > 1;
  if (split && !comm_ready(h)) return fail(HXV_ERR_STATE, "hxv_apply_density_ops on a split sector needs the communicator (hxv_comm_init after opening it)");
  HIPCHK(hipSetDevice(h->device));  // (before the first collective)
  hipStream_t st = h->stream;
  // what a rank decides from its own arguments and resources; every rank learns whether all could go on before the first collective step
  auto check_args = [&]() -> int {
    if (!coef || !d_psi || !d_out || !mean || !norm2) return fail(HXV_ERR_ARG, "hxv_apply_density_ops: NULL argument");
    if (nops < 1 || nops > DOP_MAX) return fail(HXV_ERR_ARG, "hxv_apply_density_ops: nops must be 1 .. HXV_MAX_DENSITY_OPS (8)");
    for (int a = 0; a < nops; ++a) {
      if (!d_out[a]) return fail(HXV_ERR_ARG, "hxv_apply_density_ops: NULL entry in the output list");
      if (d_out[a] == d_psi) return fail(HXV_ERR_ARG, "hxv_apply_density_ops: an output is d_psi (the operators are not applied in place)");
      for (int b = 0; b < a; ++b)
        if (d_out[a] == d_out[b]) return fail(HXV_ERR_ARG, "hxv_apply_density_ops: an output is named twice");
    }
    for (int i = 0; i < nops * 2 * nimp; ++i)
      if (!std::isfinite(coef[i])) return fail(HXV_ERR_ARG, "hxv_apply_density_ops: a coefficient is not finite");
    return HXV_OK;
  };
  int rc_local = check_args();
  std::shared_ptr<DopTables> t;
  if (rc_local == HXV_OK)
    rc_local = h->img->tables.get("density operators", "", 1, t, [&](std::shared_ptr<DopTables>& nt) {
      nt = std::make_shared<DopTables>();
      const std::string err = build_tables(s, nimp, h->device, compute_units(h->device), *nt);
      return err.empty() ? HXV_OK : fail(err.rfind("density operators tables", 0) == 0 ? HXV_ERR_HIP : HXV_ERR_STATE, err);
    });
  // scratch: the coefficients, the workgroups' partial sums, the sums of pass 1 (nops + 1) and of pass 2 (nops)
  const size_t ncoef = (size_t)DOP_MAX * 2 * DOP_MAX_NIMP;
  double* d_ws = nullptr;
  CallScope scratch(h);
  if (rc_local == HXV_OK && scratch.take((ncoef + (size_t)t->grid * DOP_NSUM + 2 * DOP_NSUM) * sizeof(double), &d_ws) != hipSuccess)
    rc_local = fail(HXV_ERR_HIP, "hxv_apply_density_ops: scratch buffer");
  int rc = split ? comm_agree(h, rc_local) : rc_local;
  if (rc) return rc;
  double *d_coef = d_ws, *d_part = d_ws + ncoef, *d_s1 = d_part + (size_t)t->grid * DOP_NSUM, *d_s2 = d_s1 + DOP_NSUM;
  const DopShape shape{s.dimup, s.pitch, s.qdw, nimp, nops, t->nchunk, t->rows, t->nitems};
  const double2* psi = (const double2*)d_psi;
  auto step_failed = [&](const char* what, hipError_t e) {
    return fail(HXV_ERR_HIP, std::string("hxv_apply_density_ops: ") + what + ": " + hipGetErrorString(e));
  };
  hipError_t e = hipMemcpyAsync(d_coef, coef, (size_t)nops * 2 * nimp * sizeof(double), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return step_failed("coefficients", e);
  // pass 1
  hipLaunchKernelGGL(dop_sums_kernel, dim3((unsigned)t->grid), dim3(DOP_THREADS), 0, st, psi, t->occ_up, t->occ_dw, (const double*)d_coef, shape, d_part);
  hipLaunchKernelGGL(dop_reduce_kernel, dim3((unsigned)(nops + 1)), dim3(DOP_THREADS), 0, st, (const double*)d_part, t->grid, (int)nops, d_s1);
  e = hipGetLastError();
  if (e != hipSuccess) return step_failed("pass 1", e);
  if (split) {
    rc = comm_allreduce_sum(h, d_s1, (size_t)nops + 1, st);
    if (rc) return rc;
  }
  double s1[DOP_NSUM] = {}, s2[DOP_NSUM] = {};
  e = hipMemcpyAsync(s1, d_s1, ((size_t)nops + 1) * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return step_failed("sums of pass 1", e);
  // the global <psi|psi>: the same number on every rank, so every rank takes the same way out
  if (!(s1[nops] > 0.0) || !std::isfinite(s1[nops])) return fail(HXV_ERR_ARG, "hxv_apply_density_ops: the state is zero or not finite");
  DopOut out{};
  double m[DOP_MAX] = {};
  for (int a = 0; a < nops; ++a) {
    m[a] = s1[a] / s1[nops];
    out.v[a] = (double2*)d_out[a];
    out.m[a] = subtract_mean ? m[a] : 0.0;
  }
  // pass 2
  hipLaunchKernelGGL(dop_apply_kernel, dim3((unsigned)t->grid), dim3(DOP_THREADS), 0, st, psi, t->occ_up, t->occ_dw, (const double*)d_coef, shape, out, d_part);
  hipLaunchKernelGGL(dop_reduce_kernel, dim3((unsigned)nops), dim3(DOP_THREADS), 0, st, (const double*)d_part, t->grid, -1, d_s2);
  e = hipGetLastError();
  if (e != hipSuccess) return step_failed("pass 2", e);
  if (split) {
    rc = comm_allreduce_sum(h, d_s2, (size_t)nops, st);
    if (rc) return rc;
  }
  e = hipMemcpyAsync(s2, d_s2, (size_t)nops * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return step_failed("sums of pass 2", e);
  for (int a = 0; a < nops; ++a) {
    mean[a] = m[a];
    norm2[a] = s2[a];
  }
  return HXV_OK;
}

}  // extern "C"
