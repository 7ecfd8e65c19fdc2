// Operators that change both spin sectors at once, behind the C-ABI (include/hxv.h: hxv_apply_spin_pair): out = sum_t coef_t X_t Y_t psi,
// X_t = c / c^dagger on an up orbital, Y_t on a dw orbital -- c_{i,up} c_{j,dw} of the pair susceptibility (the reference's build_chi_pair,
// ED_GREENS_FUNCTIONS.f90:68-106, carried commented out) and c^+_{j,dw} c_{i,up} of the transverse spin susceptibility.  One gather pass over
// the target (hxv_spin_pair_kernels.hpp) instead of two ladder calls per term through an intermediate sector.  The per-orbital tables
// (hxv_spin_pair_tables.cpp) are built on first use and kept with `to`'s sector image, by source sector, flags and orbital.
#include <cstdint>
#include <string>
#include <vector>

#include "hxv_handle.hpp"  // (no per-call scratch here: the tables live with `to`'s image, the sums in the handle's own scalars)
#include "hxv_spin_pair_host.hpp"
#include "hxv_spin_pair_kernels.hpp"

using namespace hxv;

namespace {
constexpr size_t SP_CACHE = 8;  // source sectors x flags kept per target image: the four neighbours of one solve, both directions

// The tables of one (source sector and its row order, create_up, create_dw) into the image's sector: a block of Ns up tables and Ns dw tables,
// one per orbital, filled when an orbital is first asked for.
struct SpTables : DeviceTables {
  int32_t* d_up = nullptr;  // [ns][dimup_to]
  int32_t* d_dw = nullptr;  // [ns][dimdw_to]
  uint32_t have_up = 0, have_dw = 0;
};

bool has_maps(const hxv_handle* h) { return !h->host.map_up.empty() && !h->host.map_dw.empty() && h->host.panel_rows == 0; }

// the two empty blocks of a new table set on `to`'s device
int make_tables(const hxv_handle* to, std::shared_ptr<SpTables>& t) {
  const SectorHost& b = to->host;
  t = std::make_shared<SpTables>();
  t->device = to->device;
  hipError_t e = hipMalloc((void**)&t->d_up, (size_t)b.ns * b.dimup * sizeof(int32_t));
  if (e == hipSuccess) t->more.push_back(t->d_up);
  if (e == hipSuccess) e = hipMalloc((void**)&t->d_dw, (size_t)b.ns * b.dimdw * sizeof(int32_t));
  if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("hxv_apply_spin_pair tables: ") + hipGetErrorString(e));
  t->more.push_back(t->d_dw);
  return HXV_OK;
}

// every orbital of the plan that the set does not hold yet: built and uploaded (under the store's lock)
int fill_tables(const hxv_handle* from, const hxv_handle* to, int create_up, int create_dw, const SpPlan& plan, SpTables& t) {
  const SectorHost &a = from->host, &b = to->host;
  std::vector<int32_t> tab;
  for (int u = 0; u < plan.nuq; ++u) {
    const int o = plan.uq_orb[u];
    if (t.have_up >> o & 1u) continue;
    spin_pair_up_table(a, b, o, create_up, tab);
    HIPCHK(hipMemcpy(t.d_up + (size_t)o * b.dimup, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    t.have_up |= 1u << o;
  }
  for (int d = 0; d < plan.ndq; ++d) {
    const int o = plan.dq_orb[d];
    if (t.have_dw >> o & 1u) continue;
    spin_pair_dw_table(a, b, o, create_dw, tab);
    HIPCHK(hipMemcpy(t.d_dw + (size_t)o * b.dimdw, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    t.have_dw |= 1u << o;
  }
  return HXV_OK;
}
}  // namespace

extern "C" {

int hxv_apply_spin_pair(hxv_handle* from, hxv_handle* to, int32_t create_up, int32_t create_dw, int32_t nterms, const int32_t* orb_up,
                        const int32_t* orb_dw, const double* coef, const void* d_psi, void* d_out, double* norm2) {
  if (!from || !to || !d_psi || !d_out || !orb_up || !orb_dw || !coef) return fail(HXV_ERR_ARG, "hxv_apply_spin_pair: NULL argument");
  const SectorHost &a = from->host, &b = to->host;
  if (!has_maps(from) || !has_maps(to)) return fail(HXV_ERR_STATE, "hxv_apply_spin_pair needs handles built from a model (basis maps)");
  // decided from the handles alone, the same on every rank, before anything collective could start
  if (a.nranks > 1 || b.nranks > 1) return fail(HXV_ERR_UNSUPPORTED, "hxv_apply_spin_pair: split sectors are not supported");
  if (from->device != to->device) return fail(HXV_ERR_ARG, "hxv_apply_spin_pair: handles on different devices");
  if (a.ns != b.ns) return fail(HXV_ERR_ARG, "hxv_apply_spin_pair: the two sectors have different Ns");
  if (d_out == d_psi) return fail(HXV_ERR_ARG, "hxv_apply_spin_pair: d_out == d_psi");
  if (b.nup != a.nup + (create_up ? 1 : -1) || b.ndw != a.ndw + (create_dw ? 1 : -1))
    return fail(HXV_ERR_ARG, "hxv_apply_spin_pair: `to` is not the sector reached by this operator");
  SpPlan plan;
  const std::string perr = spin_pair_plan(a.ns, nterms, orb_up, orb_dw, coef, plan);
  if (!perr.empty()) return fail(HXV_ERR_ARG, "hxv_apply_spin_pair: " + perr);
  HIPCHK(hipSetDevice(to->device));
  std::shared_ptr<SpTables> t;
  const int cu = create_up ? 1 : 0, cd = create_dw ? 1 : 0;
  const int rc = to->img->tables.get(
      "spin pair", spin_pair_key(a, cu, cd), SP_CACHE, t, [&](std::shared_ptr<SpTables>& nt) { return make_tables(to, nt); },
      [&](SpTables& have) { return fill_tables(from, to, cu, cd, plan, have); });
  if (rc) return rc;
  SpTerms tm{};
  tm.nterms = plan.nterms;
  tm.nuq = plan.nuq;
  for (int u = 0; u < plan.nuq; ++u) tm.uq_tab[u] = plan.uq_orb[u];
  for (int k = 0; k < plan.nterms; ++k) {
    tm.t_uq[k] = plan.t_uq[k];
    tm.t_dw[k] = plan.dq_orb[plan.t_dq[k]];  // the dw block is indexed by orbital
    tm.coef[k] = make_double2(plan.coef[2 * k], plan.coef[2 * k + 1]);
  }
  hipStream_t st = to->stream;
  const int grid = spin_pair_grid(b.pitch, b.dimdw);
  const hipError_t e = launch_spin_pair(tm, grid, t->d_up, b.dimup, t->d_dw, b.dimdw, b.dimup, b.pitch, b.dimdw, a.pitch, (const double2*)d_psi,
                                        (double2*)d_out, to->d_partials, to->d_scalars + LZ_TMP, st);
  if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("spin-pair kernel: ") + hipGetErrorString(e));
  if (norm2) HIPCHK(hipMemcpyAsync(norm2, to->d_scalars + LZ_TMP, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return HXV_OK;
}

}  // extern "C"
