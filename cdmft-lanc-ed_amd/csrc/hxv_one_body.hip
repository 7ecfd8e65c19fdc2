// Particle-conserving same-spin bilinears behind the C-ABI (include/hxv.h: hxv_apply_one_body): out = (sum_t coef_t c^dagger_{i_t s_t}
// c_{j_t s_t} - m) psi inside the handle's sector -- the start vectors of the bond-order, current-current and inter-orbital exciton
// susceptibilities, and the one-body density matrix over all Ns orbitals from the means.  One gather pass over the vector
// (hxv_one_body_kernels.hpp) instead of two ladder calls per term through an intermediate sector.  The tables, one per distinct
// (spin, i, j) (hxv_one_body_tables.cpp), are built on first use and kept with the handle's sector image.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "hxv_call_scope.hpp"
#include "hxv_one_body_host.hpp"
#include "hxv_one_body_kernels.hpp"

using namespace hxv;

namespace {
// Tables kept per sector image, at most: 4 dim_s bytes each (C3, DimUp = DimDw = 12870: 51 KB, 6.6 MB in all; Ns = 18 half filling: 194 KB,
// 25 MB in all).  All 2 Ns^2 of them would be 126 MB at Ns = 18.  Past the cap the least recently used table that the call under way does
// not name is dropped; a call that still launches on a dropped table keeps it alive through its own reference.
constexpr size_t OB_TABLE_CAP = 128;

struct ObTable {
  int32_t* d = nullptr;
  int device = -1;
  ~ObTable() {
    if (d) free_on_device(device, {d});
  }
};
// the tables of one sector image, most recently used last
struct ObTables : DeviceTables {
  struct Entry {
    uint32_t triple;
    std::shared_ptr<ObTable> tab;
  };
  std::vector<Entry> entries;
};

bool has_maps(const hxv_handle* h) { return !h->host.map_up.empty() && !h->host.map_dw.empty() && h->host.panel_rows == 0; }

// use[k] = the table of the plan's k-th triple: the stored one, or built and uploaded now (under the store's lock)
int fill_tables(const hxv_handle* h, const ObPlan& plan, ObTables& t, std::shared_ptr<ObTable>* use) {
  const SectorHost& s = h->host;
  std::vector<int32_t> tab;
  for (int k = 0; k < plan.ntab; ++k) {
    const uint32_t key = plan.tab[k];
    auto it = std::find_if(t.entries.begin(), t.entries.end(), [&](const ObTables::Entry& e) { return e.triple == key; });
    if (it != t.entries.end()) {
      std::rotate(it, it + 1, t.entries.end());
    } else {
      if (triple_spin(key) == 0)
        one_body_up_table(s, triple_to(key), triple_from(key), tab);
      else
        one_body_dw_table(s, triple_to(key), triple_from(key), tab);
      auto nt = std::make_shared<ObTable>();
      nt->device = h->device;
      const size_t bytes = std::max<size_t>(tab.size(), 1) * sizeof(int32_t);
      hipError_t e = hipMalloc((void**)&nt->d, bytes);
      if (e == hipSuccess && !tab.empty()) e = hipMemcpy(nt->d, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice);
      if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("hxv_apply_one_body tables: ") + hipGetErrorString(e));
      // (at most OB_PLAN_MAX_TERMS tables are the present call's and sit at the end: the front one is never among them)
      if (t.entries.size() >= OB_TABLE_CAP) t.entries.erase(t.entries.begin());
      t.entries.push_back({key, nt});
    }
    use[k] = t.entries.back().tab;
  }
  return HXV_OK;
}
}  // namespace

extern "C" {

int hxv_apply_one_body(hxv_handle* h, int32_t nterms, const int32_t* spin, const int32_t* orb_to, const int32_t* orb_from, const double* coef,
                       int32_t subtract_mean, const void* d_psi, void* d_out, double* mean, double* norm2) {
  if (!h || !d_psi || !d_out || !spin || !orb_to || !orb_from || !coef) return fail(HXV_ERR_ARG, "hxv_apply_one_body: NULL argument");
  const SectorHost& s = h->host;
  if (!has_maps(h)) return fail(HXV_ERR_STATE, "hxv_apply_one_body needs a handle built from a model (basis maps)");
  // decided from the handle alone, the same on every rank, before anything collective could start
  if (s.nranks > 1) return fail(HXV_ERR_UNSUPPORTED, "hxv_apply_one_body: split sectors are not supported");
  if (d_out == d_psi) return fail(HXV_ERR_ARG, "hxv_apply_one_body: d_out == d_psi");
  ObPlan plan;
  const std::string perr = one_body_plan(s.ns, nterms, spin, orb_to, orb_from, coef, plan);
  if (!perr.empty()) return fail(HXV_ERR_ARG, "hxv_apply_one_body: " + perr);
  HIPCHK(hipSetDevice(h->device));
  std::shared_ptr<ObTables> t;
  std::shared_ptr<ObTable> use[OB_PLAN_MAX_TERMS];  // held until the kernels are done
  int rc = h->img->tables.get(
      "one body", "", 1, t,
      [&](std::shared_ptr<ObTables>& nt) {
        nt = std::make_shared<ObTables>();
        nt->device = h->device;
        return HXV_OK;
      },
      [&](ObTables& have) { return fill_tables(h, plan, have, use); });
  if (rc) return rc;
  ObTerms tm{};
  tm.nterms = plan.nterms;
  int uq_of[OB_PLAN_MAX_TERMS];
  for (int k = 0; k < plan.ntab; ++k) {
    uq_of[k] = -1;
    if (triple_spin(plan.tab[k]) == 0) {
      uq_of[k] = tm.nuq;
      tm.uq_tab[tm.nuq++] = use[k]->d;
    }
  }
  for (int k = 0; k < plan.nterms; ++k) {
    const int tab = plan.t_tab[k];
    tm.dw_tab[k] = uq_of[tab] < 0 ? use[tab]->d : nullptr;
    tm.t_uq[k] = (uint8_t)(uq_of[tab] < 0 ? 0 : uq_of[tab]);
    tm.coef[k] = make_double2(plan.coef[2 * k], plan.coef[2 * k + 1]);
  }
  hipStream_t st = h->stream;
  const int grid = one_body_grid(s.pitch, s.dimdw);
  // per-call scratch: the workgroups' partial sums and the OB_NSUM + 1 sums
  CallScope scratch(h);
  double* d_ws = nullptr;
  if (scratch.take(((size_t)OB_NSUM * grid + OB_NSUM + 1) * sizeof(double), &d_ws) != hipSuccess)
    return fail(HXV_ERR_HIP, "hxv_apply_one_body: scratch buffer");
  double *d_part = d_ws, *d_sums = d_ws + (size_t)OB_NSUM * grid;
  const double2* psi = (const double2*)d_psi;
  hipError_t e = launch_one_body(tm, grid, s.dimup, s.pitch, s.dimdw, psi, (double2*)d_out, d_part, d_sums, st);
  if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("one-body kernel: ") + hipGetErrorString(e));
  double sums[OB_NSUM + 1] = {};
  HIPCHK(hipMemcpyAsync(sums, d_sums, OB_NSUM * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  // known only after the pass that also wrote d_out: the one error of this call that leaves d_out overwritten
  if (!(sums[0] > 0.0) || !std::isfinite(sums[0])) return fail(HXV_ERR_ARG, "hxv_apply_one_body: the state is zero or not finite");
  const double m_re = sums[1] / sums[0], m_im = sums[2] / sums[0];
  double n2 = sums[3];
  if (subtract_mean) {
    e = launch_one_body_shift(make_double2(m_re, m_im), grid, s.dimup, s.pitch, s.dimdw, psi, (double2*)d_out, d_part, d_sums + OB_NSUM, st);
    if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("one-body mean subtraction: ") + hipGetErrorString(e));
    HIPCHK(hipMemcpyAsync(&n2, d_sums + OB_NSUM, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  if (mean) mean[0] = m_re, mean[1] = m_im;
  if (norm2) *norm2 = n2;
  return HXV_OK;
}

}  // extern "C"
