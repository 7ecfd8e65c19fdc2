// Host tables of hxv_observables_accumulate (hxv_density_host.hpp): pure C++, no HIP call.  The pair and bin tables of one sector, from the
// basis maps alone, in device-row numbering.
#include <algorithm>

#include "hxv_density_host.hpp"

namespace hxv {

namespace {
inline int parity_below(uint32_t m, int bit) { return __builtin_popcount(m & ((1u << bit) - 1u)) & 1; }

// |k> = c^+_is c_js |m> (ED_SETUP.f90 c / cdg: the sign counts the occupied orbitals below the one acted on); false if not applicable
inline bool hop(uint32_t m, int is, int js, uint32_t& k, int& sg) {
  if (!((m >> js) & 1u) || ((m >> is) & 1u)) return false;
  const uint32_t r = m ^ (1u << js);
  sg = (parity_below(m, js) ^ parity_below(r, is)) ? -1 : 1;
  k = r | (1u << is);
  return true;
}
}  // namespace

std::string obs_build_tables(const SectorHost& s, int nimp, ObsHostTables& t) {
  const int nw = 1 << nimp, np = nimp * nimp;
  const uint32_t mask = (uint32_t)nw - 1u;
  t = ObsHostTables{};
  t.nimp = nimp;
  t.nw = nw;
  t.np = np;
  t.gtot = nw + 2 * np;
  const std::vector<uint32_t>& mdev = s.dev_map_up();  // reference bit strings by device row
  const bool ro = s.row_order();
  std::vector<int32_t>&seg_ptr = t.seg_ptr, &ea = t.ent_a, &eb = t.ent_b;
  std::vector<int8_t>& es = t.ent_s;
  seg_ptr.assign(nw + np + 1, 0);
  ea.reserve((size_t)s.dimup * 4);
  eb.reserve((size_t)s.dimup * 4);
  es.reserve((size_t)s.dimup * 4);
  {
    std::vector<std::vector<int32_t>> bins(nw);
    for (int r = 0; r < s.dimup; ++r) bins[mdev[r] & mask].push_back(r);
    for (int g = 0; g < nw; ++g) {
      seg_ptr[g] = (int32_t)ea.size();
      for (int r : bins[g]) {
        ea.push_back(r);
        eb.push_back(r);
        es.push_back(1);
      }
    }
  }
  for (int p = 0; p < np; ++p) {
    const int is = p % nimp, js = p / nimp;
    seg_ptr[nw + p] = (int32_t)ea.size();
    if (is >= js) continue;  // R(js,is) = conj R(is,js): the host fills the lower triangle
    for (int r = 0; r < s.dimup; ++r) {
      uint32_t k;
      int sg;
      if (!hop(mdev[r], is, js, k, sg)) continue;
      const int jref = rank_in(s.map_up, k);
      if (jref < 0) return "observables: a hop target is missing from the up basis";
      const int rb = ro ? s.up_perm[jref] : jref;
      if (ro && (s.up_sign[r] ^ s.up_sign[rb])) sg = -sg;
      ea.push_back(r);
      eb.push_back(rb);
      es.push_back((int8_t)sg);
    }
  }
  seg_ptr[nw + np] = (int32_t)ea.size();
  if ((int64_t)ea.size() >= INT32_MAX) return "observables: too many row pairs";
  // dw side: this rank's columns; a partner column owned by rank o sits at slot o*cmax + (its index in o's slab) of the gathered copy,
  // or is read from the slab itself when the sector is not split
  std::vector<int32_t> first(s.nranks + 1, 0);
  for (int p = 0; p < s.nranks; ++p) {
    int q, c0;
    dw_split(s.dimdw, p, s.nranks, q, c0);
    first[p] = c0;
  }
  first[s.nranks] = s.dimdw;
  std::vector<int32_t>&dwp_ptr = t.dwp_ptr, &dslot = t.dwp_slot, &dp = t.dwp_p;
  std::vector<int8_t>& ds = t.dwp_s;
  dwp_ptr.assign(std::max(s.qdw, 0) + 1, 0);
  std::vector<std::vector<int32_t>> cbins(nw);
  for (int c = 0; c < s.qdw; ++c) {
    const uint32_t m = s.map_dw[s.dw0 + c];
    cbins[m & mask].push_back(c);
    dwp_ptr[c] = (int32_t)dslot.size();
    for (int p = 0; p < np; ++p) {
      const int is = p % nimp, js = p / nimp;
      if (is >= js) continue;  // (as the up side)
      uint32_t k;
      int sg;
      if (!hop(m, is, js, k, sg)) continue;
      const int cj = rank_in(s.map_dw, k);
      if (cj < 0) return "observables: a hop target is missing from the dw basis";
      int32_t slot = cj;
      if (s.nranks > 1) {
        const int o = (int)(std::upper_bound(first.begin(), first.end(), cj) - first.begin()) - 1;
        slot = o * s.cmax + (cj - first[o]);
      }
      dslot.push_back(slot);
      dp.push_back(p);
      ds.push_back((int8_t)sg);
    }
  }
  dwp_ptr[std::max(s.qdw, 0)] = (int32_t)dslot.size();
  t.dwbin_ptr.assign(nw + 1, 0);
  for (int g = 0; g < nw; ++g) {
    t.dwbin_ptr[g] = (int32_t)t.dwbin_cols.size();
    t.dwbin_cols.insert(t.dwbin_cols.end(), cbins[g].begin(), cbins[g].end());
  }
  t.dwbin_ptr[nw] = (int32_t)t.dwbin_cols.size();
  return std::string();
}

}  // namespace hxv
