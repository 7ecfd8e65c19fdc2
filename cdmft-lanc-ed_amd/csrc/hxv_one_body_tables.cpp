// Host tables of hxv_apply_one_body (hxv_one_body_host.hpp): pure C++, no HIP call.  One table per (spin, i, j) inside one sector, from the
// basis maps alone -- c_j then c^dagger_i as the ladder operators apply them, read backwards, from the target to its source.
#include <cmath>

#include "hxv_one_body_host.hpp"

namespace hxv {

std::string one_body_plan(int ns, int nterms, const int32_t* spin, const int32_t* orb_to, const int32_t* orb_from, const double* coef, ObPlan& p) {
  if (nterms < 1 || nterms > OB_PLAN_MAX_TERMS) return "the number of terms is outside [1, HXV_MAX_ONE_BODY_TERMS]";
  p = ObPlan{};
  p.nterms = nterms;
  for (int t = 0; t < nterms; ++t) {
    if (spin[t] != 0 && spin[t] != 1) return "a spin that is not 0 (up) or 1 (dw)";
    if (orb_to[t] < 0 || orb_to[t] >= ns || orb_from[t] < 0 || orb_from[t] >= ns) return "an orbital outside [0, Ns)";
    if (!std::isfinite(coef[2 * t]) || !std::isfinite(coef[2 * t + 1])) return "a coefficient that is not finite";
    const uint32_t key = one_body_triple(spin[t], orb_to[t], orb_from[t]);
    int k = 0;
    while (k < p.ntab && p.tab[k] != key) ++k;
    if (k == p.ntab) p.tab[p.ntab++] = key;
    p.t_tab[t] = (uint8_t)k;
    p.coef[2 * t] = coef[2 * t];
    p.coef[2 * t + 1] = coef[2 * t + 1];
  }
  return "";
}

namespace {
// the source configuration of target configuration m_to under c^dagger_i c_j, or false; neg = the sign of c_j on the source times the sign
// of c^dagger_i on what c_j leaves = (-1)^(occupied orbitals strictly between i and j)
inline bool source_of(uint32_t m_to, int i, int j, uint32_t& m_from, int& neg) {
  const uint32_t bi = 1u << i, bj = 1u << j;
  if (!(m_to & bi)) return false;
  if (i != j && (m_to & bj)) return false;
  m_from = m_to ^ bi ^ bj;  // (i == j: the target itself)
  const uint32_t mid = m_from ^ bj;
  neg = (__builtin_popcount(m_from & (bj - 1u)) + __builtin_popcount(mid & (bi - 1u))) & 1;
  return true;
}
}  // namespace

void one_body_up_table(const SectorHost& s, int orb_to, int orb_from, std::vector<int32_t>& tab) {
  const std::vector<uint32_t>& md = s.dev_map_up();  // reference bit strings by device row
  tab.assign((size_t)s.dimup, OB_DEAD);
  for (int r = 0; r < s.dimup; ++r) {
    uint32_t m_from;
    int neg;
    if (!source_of(md[r], orb_to, orb_from, m_from, neg)) continue;
    int j = rank_in(s.map_up, m_from);
    if (j < 0) continue;  // (cannot happen: the source has as many particles as the target)
    if (s.row_order()) {
      j = s.up_perm[j];
      neg ^= (int)s.up_sign[j] ^ (int)s.up_sign[r];
    }
    tab[r] = (int32_t)((uint32_t)j | ((uint32_t)neg << 31));
  }
}

void one_body_dw_table(const SectorHost& s, int orb_to, int orb_from, std::vector<int32_t>& tab) {
  tab.assign((size_t)s.dimdw, OB_DEAD);
  for (int c = 0; c < s.dimdw; ++c) {
    uint32_t m_from;
    int neg;
    if (!source_of(s.map_dw[c], orb_to, orb_from, m_from, neg)) continue;
    const int j = rank_in(s.map_dw, m_from);
    if (j < 0) continue;
    tab[c] = (int32_t)((uint32_t)j | ((uint32_t)neg << 31));
  }
}

}  // namespace hxv
