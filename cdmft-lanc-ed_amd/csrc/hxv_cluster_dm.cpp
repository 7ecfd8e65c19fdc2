// Cluster reduced density matrix of a device-resident state (include/hxv.h: hxv_cluster_dm_accumulate).
//
// rho_imp = Tr_bath |psi><psi| (density_matrix_impurity, ED_OBSERVABLES.f90:465-582):
//   rho(io,jo) += peso * sum_{b_up,b_dw} psi(a_up,b_up ; a_dw,b_dw) * conj psi(a'_up,b_up ; a'_dw,b_dw),   io = a_up + 2^Nimp a_dw  (0-based)
// the partial trace over everything but the Nimp impurity orbitals, without a Fermi sign: cluster_dm_groups (hxv_partial_trace_groups.cpp)
// lists the bath groups, the engine (hxv_partial_trace.hip) does the rest, every class through its tile kernel.  The tables are built on the
// first call and cached with the sector image.
#include "hxv_handle.hpp"
#include "hxv_partial_trace_host.hpp"

using namespace hxv;

namespace {
constexpr int CDM_MAX_NIMP = 5;  // the dense matrix: 16 MB at Nimp 5, 268 MB at Nimp 6
}

extern "C" {

int64_t hxv_cluster_dm_elems(const hxv_handle* h) {
  if (!h || h->host.map_up.empty() || h->host.map_dw.empty() || h->host.panel_rows > 0) return 0;
  const int n = nimp_of(h->host);
  if (n < 1 || n > CDM_MAX_NIMP || n > h->host.ns) return 0;
  return (int64_t)2 << (4 * n);
}

int hxv_cluster_dm_accumulate(hxv_handle* h, const void* d_psi, double weight, int32_t accumulate, double* cdm) {
  if (!h || !d_psi || !cdm) return fail(HXV_ERR_ARG, "hxv_cluster_dm_accumulate: NULL argument");
  const SectorHost& s = h->host;
  if (s.map_up.empty() || s.map_dw.empty() || s.panel_rows > 0)
    return fail(HXV_ERR_STATE, "hxv_cluster_dm_accumulate needs a handle built from a model (basis maps)");
  const int nimp = nimp_of(s);
  if (nimp < 1 || nimp > s.ns) return fail(HXV_ERR_STATE, "hxv_cluster_dm_accumulate: the handle carries no impurity size");
  if (nimp > CDM_MAX_NIMP) return fail(HXV_ERR_UNSUPPORTED, "hxv_cluster_dm_accumulate: Nimp > 5 (a dense matrix of 268 MB and more)");
  if (s.nranks > 1 && !comm_ready(h)) return fail(HXV_ERR_STATE, "hxv_cluster_dm_accumulate on a split sector needs the communicator (hxv_comm_init after opening it)");
  HIPCHK(hipSetDevice(h->device));
  std::shared_ptr<PtTables> t;
  const int rc_local = pt_stored_tables(h, "cluster density matrix", "", 1, t, [&](std::shared_ptr<PtTables>& nt) {
    PtGroups up, dw;
    const std::string err = cluster_dm_groups(s, nimp, up, dw);
    return err.empty() ? pt_make_tables(h, nimp, up, dw, 0, "cluster density matrix", nt) : fail(HXV_ERR_STATE, err);
  });
  return pt_accumulate(h, t, rc_local, d_psi, weight, accumulate != 0, cdm, "hxv_cluster_dm_accumulate");
}

}  // extern "C"
