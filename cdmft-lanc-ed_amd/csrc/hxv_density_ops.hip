// Density-type operators on a device-resident state (include/hxv.h: hxv_apply_density_ops): the start vectors of the two-particle stage.
//
// O_a = sum_is (cu_a[is] n_is,up + cd_a[is] n_is,dw) over the Nimp impurity orbitals is diagonal in the Fock basis: on the basis state
// (iup, idw) it is the number  f_a = fu_a(o_up) + fd_a(o_dw),  o_s = the low Nimp bits of that spin's configuration.  S^z_i, n_i, n_i,s and
// every total or staggered combination of them are of this kind, and  out_a = (f_a - m_a) psi,  m_a = <psi|O_a|psi> / <psi|psi>,  is the start
// vector (and the probe) of the spin / charge susceptibility chi_ab (the reference's buildChi_impurity, ED_GREENS_FUNCTIONS.f90:68-106).
// Tables (built on the host, kept with the sector image): one 32-bit impurity-occupation word per DEVICE row and one per local column.  A
// diagonal operator keeps the row, and the basis sign of a device row multiplies psi and out alike: only the occupation lookup goes through
// the device row order.
// Kernels (hxv_density_ops_kernels.hpp; the tables and the work list: hxv_density_ops_tables.cpp), 256 threads, a work item = (local column, chunk of its rows), item i on workgroup i mod gridDim:
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
#include "hxv_density_host.hpp"
#include "hxv_density_ops_kernels.hpp"

using namespace hxv;

namespace {
struct DopTables : DeviceTables {
  uint32_t *occ_up = nullptr, *occ_dw = nullptr;  // [pitch] by device row (pad rows 0), [max(qdw,1)] by local column
  int nchunk = 1, rows = 0;                       // chunks a column is cut into, rows of a chunk (a multiple of 8)
  int64_t nitems = 0;
  int grid = 1;                                   // workgroups of the two passes
};

// the host tables (dop_build_tables, hxv_density_ops_tables.cpp), the two occupation lists uploaded in one block
std::string build_tables(const SectorHost& s, int nimp, int device, int ncu, DopTables& t) {
  DopHostTables ht;
  const std::string err = dop_build_tables(s, nimp, ncu, ht);
  if (!err.empty()) return err;
  t.device = device;
  t.nchunk = ht.nchunk;
  t.rows = ht.rows;
  t.nitems = ht.nitems;
  t.grid = ht.grid;
  TableArena ar;
  (void)ar.add(ht.occ_up, &t.occ_up);
  (void)ar.add(ht.occ_dw, &t.occ_dw);
  hipError_t e = ar.commit(&t.base, &t.bytes);
  if (e != hipSuccess) return std::string("density operators tables: ") + hipGetErrorString(e);
  return std::string();
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
