// Impurity observables of a device-resident state (include/hxv.h: hxv_observables_accumulate).
//
// Every quantity of the reference's lanc_observables / lanc_local_energy and the single-particle density matrix of
// density_matrix_impurity (ED_OBSERVABLES.f90:94-236, 246-452, 609-686) is a function of one small RAW RECORD per state:
//   W[a_up + 2^Nimp a_dw] = sum |psi(iup,idw)|^2 over the basis states whose impurity bits (the low Nimp bits of each spin's
//                           configuration, ED_OBSERVABLES.f90:540-556) are a_up and a_dw;
//   R_s(is,js)            = sum sgn * psi_i * conj(psi_j),  |j> = c^+_is c_js |i>  (same spin s; is < js on the device, the host fills
//                           R_s(js,is) = conj R_s(is,js));  R_s(is,is) from W.
// Four kernels compute it without floating-point atomics, in a fixed order (the same vector gives the same bits on every call):
//   obs_rows_kernel<false>, obs_rows_kernel<true>, obs_rdw_kernel
//                      one workgroup per local column c -> colout[c][g], g over Gtot = 2^Nimp + 2*Nimp^2 groups:
//                        g <  2^Nimp           sum |psi(r,c)|^2 over the device rows r whose up impurity bits are g
//                        g in R_up block       sum sgn * psi(a,c) * conj(psi(b,c)) over the row pairs of impurity pair p
//                                              (partner row in the same column: the access pattern of the product's up hops)
//                        g in R_dw block       sgn * <psi(:,c'), psi(:,c)>  for the column c' = c^+_is c_js c (whole columns, as the
//                                              dw-hop pass; c' may live on another rank: then it is read from a gathered copy)
//   obs_reduce_kernel  one workgroup per record element: W(a_up,a_dw) sums colout[c][a_up] over the columns with dw bits a_dw,
//                      R(p) sums colout[c][p] over every local column; per-thread strided sums + a fixed-order tree.
// The kernels are in hxv_observables_kernels.hpp.  The pair and bin tables are built on the host (hxv_observables_tables.cpp) in device-row
// numbering (the basis signs of the device row order folded into the pair's sign) and cached with the sector image.  On a split sector
// every rank reduces its columns and the record is all-reduced.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "hxv_call_scope.hpp"
#include "hxv_density_host.hpp"
#include "hxv_observables_kernels.hpp"

using namespace hxv;

namespace {
struct ObsTables : DeviceTables {
  int nimp = 0, nw = 0, np = 0, gtot = 0;
  int64_t nent = 0, ndwp = 0;
  // the device copies of ObsHostTables' vectors (hxv_density_host.hpp)
  int32_t *seg_ptr = nullptr, *ent_a = nullptr, *ent_b = nullptr;
  int8_t* ent_s = nullptr;
  int32_t *dwp_ptr = nullptr, *dwp_slot = nullptr, *dwp_p = nullptr, *dwbin_ptr = nullptr, *dwbin_cols = nullptr;
  int8_t* dwp_s = nullptr;
};

// the host tables (obs_build_tables, hxv_observables_tables.cpp) uploaded in one block
std::string build_tables(const SectorHost& s, int nimp, int device, ObsTables& t) {
  ObsHostTables ht;
  const std::string err = obs_build_tables(s, nimp, ht);
  if (!err.empty()) return err;
  t.nimp = ht.nimp;
  t.nw = ht.nw;
  t.np = ht.np;
  t.gtot = ht.gtot;
  t.device = device;
  t.nent = (int64_t)ht.ent_a.size();
  t.ndwp = (int64_t)ht.dwp_slot.size();
  TableArena ar;
  (void)ar.add(ht.seg_ptr, &t.seg_ptr);
  (void)ar.add(ht.ent_a, &t.ent_a);
  (void)ar.add(ht.ent_b, &t.ent_b);
  (void)ar.add(ht.ent_s, &t.ent_s);
  (void)ar.add(ht.dwp_ptr, &t.dwp_ptr);
  (void)ar.add(ht.dwp_slot, &t.dwp_slot);
  (void)ar.add(ht.dwp_p, &t.dwp_p);
  (void)ar.add(ht.dwp_s, &t.dwp_s);
  (void)ar.add(ht.dwbin_ptr, &t.dwbin_ptr);
  (void)ar.add(ht.dwbin_cols, &t.dwbin_cols);
  hipError_t e = ar.commit(&t.base, &t.bytes);
  if (e != hipSuccess) return std::string("observables tables: ") + hipGetErrorString(e);
  return std::string();
}
}  // namespace

extern "C" {

int64_t hxv_obs_record_elems(const hxv_handle* h) {
  if (!h || h->host.map_up.empty() || h->host.map_dw.empty() || h->host.panel_rows > 0) return 0;
  const int n = nimp_of(h->host);
  if (n < 1 || n > OBS_MAX_NIMP) return 0;
  return ((int64_t)1 << (2 * n)) + 4 * (int64_t)n * n;
}

int hxv_observables_accumulate(hxv_handle* h, const void* d_psi, double weight, int32_t accumulate, double* record) {
  if (!h || !d_psi || !record) return fail(HXV_ERR_ARG, "hxv_observables_accumulate: NULL argument");
  const SectorHost& s = h->host;
  if (s.map_up.empty() || s.map_dw.empty() || s.panel_rows > 0)
    return fail(HXV_ERR_STATE, "hxv_observables_accumulate needs a handle built from a model (basis maps)");
  const int nimp = nimp_of(s);
  if (nimp < 1 || nimp > s.ns) return fail(HXV_ERR_STATE, "hxv_observables_accumulate: the handle carries no impurity size");
  if (nimp > OBS_MAX_NIMP) return fail(HXV_ERR_UNSUPPORTED, "hxv_observables_accumulate: Nimp > 10 (a record of more than 8 MB)");
  const bool split = s.nranks > 1;
  if (split && !comm_ready(h)) return fail(HXV_ERR_STATE, "hxv_observables_accumulate on a split sector needs the communicator (hxv_comm_init after opening it)");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  // rank-local preparation: tables (once per sector image), scratch; every rank learns whether all could go on
  int rc_local = HXV_OK;
  std::shared_ptr<ObsTables> t;
  rc_local = h->img->tables.get("observables", "", 1, t, [&](std::shared_ptr<ObsTables>& nt) {
    nt = std::make_shared<ObsTables>();
    const std::string err = build_tables(s, nimp, h->device, *nt);
    return err.empty() ? HXV_OK : fail(err.rfind("observables tables", 0) == 0 ? HXV_ERR_HIP : HXV_ERR_STATE, err);
  });
  const int np = nimp * nimp, gtot = (1 << nimp) + 2 * np;
  const int64_t nww = (int64_t)1 << (2 * nimp), nrec = nww + 4 * (int64_t)np;
  double2 *d_col = nullptr, *d_full = nullptr;
  double* d_rec = nullptr;
  CallScope scratch(h);
  if (rc_local == HXV_OK) {
    hipError_t e1 = scratch.take(std::max<size_t>((size_t)s.qdw * gtot, 1) * sizeof(double2), &d_col);
    hipError_t e2 = scratch.take((size_t)nrec * sizeof(double), &d_rec);
    hipError_t e3 = split ? scratch.take(std::max<size_t>((size_t)s.nranks * s.cmax * s.pitch, 1) * sizeof(double2), &d_full) : hipSuccess;
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) rc_local = fail(HXV_ERR_HIP, "hxv_observables_accumulate: scratch buffers");
  }
  int rc = split ? comm_agree(h, rc_local) : rc_local;
  if (rc) return rc;
  const double2* psi = (const double2*)d_psi;
  if (split) {
    rc = comm_allgather_slab(h, psi, d_full, st);
    if (rc) return rc;
  }
  if (s.qdw > 0) {
    const dim3 grid((unsigned)s.qdw), block(OBS_THREADS);
    hipLaunchKernelGGL(obs_rows_kernel<false>, grid, block, 0, st, psi, s.pitch, s.qdw, t->nw, t->np, t->seg_ptr, t->ent_a, t->ent_b, t->ent_s, d_col);
    hipLaunchKernelGGL(obs_rows_kernel<true>, grid, block, 0, st, psi, s.pitch, s.qdw, t->nw, t->np, t->seg_ptr, t->ent_a, t->ent_b, t->ent_s, d_col);
    hipLaunchKernelGGL(obs_rdw_kernel, grid, block, 0, st, psi, split ? (const double2*)d_full : psi, s.pitch, s.dimup, s.qdw, t->nw, t->np,
                       t->dwp_ptr, t->dwp_slot, t->dwp_p, t->dwp_s, d_col);
  }
  hipLaunchKernelGGL(obs_reduce_kernel, dim3((unsigned)(nww + 2 * np)), dim3(OBS_THREADS), 0, st, (const double2*)d_col, s.qdw, nimp, t->nw,
                     t->np, t->dwbin_ptr, t->dwbin_cols, d_rec);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("observables kernels: ") + hipGetErrorString(e));
  if (split) {
    rc = comm_allreduce_sum(h, d_rec, (size_t)nrec, st);
    if (rc) return rc;
  }
  std::vector<double> raw((size_t)nrec);
  e = hipMemcpyAsync(raw.data(), d_rec, (size_t)nrec * sizeof(double), hipMemcpyDeviceToHost, st);
  scratch.release();  // (synchronises the stream: raw is read below)
  if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("hxv_observables_accumulate: ") + hipGetErrorString(e));
  // R_s(js,is) = conj R_s(is,js): c^+_js c_is is the adjoint of c^+_is c_js, and the device computes is < js only
  for (int spin = 0; spin < 2; ++spin) {
    double* R = raw.data() + nww + 2 * np * spin;
    for (int js = 0; js < nimp; ++js)
      for (int is = js + 1; is < nimp; ++is) {
        R[2 * (is + js * nimp)] = R[2 * (js + is * nimp)];
        R[2 * (is + js * nimp) + 1] = -R[2 * (js + is * nimp) + 1];
      }
  }
  // R_s(is,is) = sum of W over the impurity configurations with orbital is occupied in spin s (ED_OBSERVABLES.f90:633-640)
  for (int is = 0; is < nimp; ++is) {
    double up = 0.0, dw = 0.0;
    for (int64_t a = 0; a < nww; ++a) {
      if ((a >> is) & 1) up += raw[a];
      if ((a >> (nimp + is)) & 1) dw += raw[a];
    }
    raw[nww + 2 * (is + is * nimp)] = up;
    raw[nww + 2 * np + 2 * (is + is * nimp)] = dw;
  }
  for (int64_t i = 0; i < nrec; ++i) record[i] = accumulate ? record[i] + weight * raw[i] : weight * raw[i];
  return HXV_OK;
}

}  // extern "C"
