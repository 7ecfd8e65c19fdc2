// Reduced density matrix of a subset S of the impurity orbitals of a device-resident state (include/hxv.h: hxv_reduced_dm_accumulate).
//
// rho_S = Tr_env |psi><psi|, env = every orbital outside S (the bath and the traced impurity orbitals), with or without the Fermi sign of
// moving the operators of S in front of the others: reduced_dm_groups (hxv_partial_trace_groups.cpp) lists the groups and their signs, the
// engine (hxv_partial_trace.hip) does the rest.  Classes with n <= 4 (every class of a one- or two-orbital mask) take the engine's pair
// kernel, the others (n <= 36 with four orbitals) its 2 x 2 tile kernel.  The tables are cached with the sector image by (mask, fermi_sign).
#include <cstdlib>

#include "hxv_handle.hpp"
#include "hxv_partial_trace_host.hpp"

using namespace hxv;

namespace {
constexpr int RDM_MAX_NRED = 4;  // 256 x 256, blocks up to 36 x 36
constexpr size_t RDM_CACHE = 8;  // tables kept per sector image: the masks of one solve (sites, pairs of sites), both conventions

bool has_maps(const hxv_handle* h) { return !h->host.map_up.empty() && !h->host.map_dw.empty() && h->host.panel_rows == 0; }
}  // namespace

extern "C" {

int64_t hxv_reduced_dm_elems(const hxv_handle* h, uint32_t orbital_mask) {
  if (!h || !has_maps(h)) return 0;
  const int n = nimp_of(h->host);
  if (n < 1 || n > h->host.ns || n > 32) return 0;
  const int nred = __builtin_popcount(orbital_mask);
  if (nred < 1 || nred > RDM_MAX_NRED || (n < 32 && (orbital_mask >> n))) return 0;
  return (int64_t)2 << (4 * nred);
}

int hxv_reduced_dm_accumulate(hxv_handle* h, const void* d_psi, uint32_t orbital_mask, int32_t fermi_sign, double weight, int32_t accumulate,
                              double* rdm) {
  if (!h || !d_psi || !rdm) return fail(HXV_ERR_ARG, "hxv_reduced_dm_accumulate: NULL argument");
  if (fermi_sign != 0 && fermi_sign != 1) return fail(HXV_ERR_ARG, "hxv_reduced_dm_accumulate: fermi_sign is 0 or 1");
  if (!orbital_mask) return fail(HXV_ERR_ARG, "hxv_reduced_dm_accumulate: empty orbital mask");
  const SectorHost& s = h->host;
  if (!has_maps(h)) return fail(HXV_ERR_STATE, "hxv_reduced_dm_accumulate needs a handle built from a model (basis maps)");
  const int nimp = nimp_of(s);
  if (nimp < 1 || nimp > s.ns || nimp > 32) return fail(HXV_ERR_STATE, "hxv_reduced_dm_accumulate: the handle carries no impurity size");
  if (nimp < 32 && (orbital_mask >> nimp)) return fail(HXV_ERR_ARG, "hxv_reduced_dm_accumulate: the orbital mask names bits outside the Nimp impurity orbitals");
  if (__builtin_popcount(orbital_mask) > RDM_MAX_NRED) return fail(HXV_ERR_UNSUPPORTED, "hxv_reduced_dm_accumulate: more than 4 orbitals in the mask");
  if (s.nranks > 1 && !comm_ready(h)) return fail(HXV_ERR_STATE, "hxv_reduced_dm_accumulate on a split sector needs the communicator (hxv_comm_init after opening it)");
  HIPCHK(hipSetDevice(h->device));
  // HXV_RDM_PAIR_KERNEL=0 sends every class to the tile kernel (the A/B hook of scripts/reduced_dm_bench.py)
  const char* ab = std::getenv("HXV_RDM_PAIR_KERNEL");
  const int small_n = (ab && ab[0] == '0' && !ab[1]) ? 0 : PT_PAIR_N;
  const uint64_t key = (uint64_t)orbital_mask | ((uint64_t)fermi_sign << 32) | ((uint64_t)(small_n == 0) << 33);
  std::shared_ptr<PtTables> t;
  const int rc_local = pt_stored_tables(h, "reduced density matrix", std::string((const char*)&key, sizeof key), RDM_CACHE, t, [&](std::shared_ptr<PtTables>& nt) {
    PtGroups up, dw;
    const std::string err = reduced_dm_groups(s, orbital_mask, fermi_sign, up, dw);
    return err.empty() ? pt_make_tables(h, __builtin_popcount(orbital_mask), up, dw, small_n, "reduced density matrix", nt) : fail(HXV_ERR_STATE, err);
  });
  return pt_accumulate(h, t, rc_local, d_psi, weight, accumulate != 0, rdm, "hxv_reduced_dm_accumulate");
}

}  // extern "C"
