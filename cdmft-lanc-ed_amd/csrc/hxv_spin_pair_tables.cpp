// Host tables of hxv_apply_spin_pair (hxv_spin_pair_host.hpp): pure C++, no HIP call.  One table per (orbital, spin) between two sectors,
// from the basis maps alone -- the reference's c / cdg (ED_SETUP.f90:807-833) read backwards, from the target to its source.
#include <cmath>

#include "hxv_spin_pair_host.hpp"

namespace hxv {

std::string spin_pair_plan(int ns, int nterms, const int32_t* orb_up, const int32_t* orb_dw, const double* coef, SpPlan& p) {
  if (nterms < 1 || nterms > SP_PLAN_MAX_TERMS) return "the number of terms is outside [1, HXV_MAX_SPIN_PAIR_TERMS]";
  p = SpPlan{};
  p.nterms = nterms;
  for (int t = 0; t < nterms; ++t) {
    if (orb_up[t] < 0 || orb_up[t] >= ns || orb_dw[t] < 0 || orb_dw[t] >= ns) return "an orbital outside [0, Ns)";
    if (!std::isfinite(coef[2 * t]) || !std::isfinite(coef[2 * t + 1])) return "a coefficient that is not finite";
    int u = 0, d = 0;
    while (u < p.nuq && p.uq_orb[u] != orb_up[t]) ++u;
    if (u == p.nuq) p.uq_orb[p.nuq++] = (uint8_t)orb_up[t];
    while (d < p.ndq && p.dq_orb[d] != orb_dw[t]) ++d;
    if (d == p.ndq) p.dq_orb[p.ndq++] = (uint8_t)orb_dw[t];
    p.t_uq[t] = (uint8_t)u;
    p.t_dq[t] = (uint8_t)d;
    p.coef[2 * t] = coef[2 * t];
    p.coef[2 * t + 1] = coef[2 * t + 1];
  }
  return "";
}

namespace {
// the source configuration of target configuration m_to, or false: the target must hold the orbital after a creation, not after a destruction
inline bool source_of(uint32_t m_to, uint32_t bit, int create, uint32_t& m_from, int& neg) {
  if (((m_to & bit) != 0u) != (create != 0)) return false;
  m_from = m_to ^ bit;
  neg = __builtin_popcount(m_from & (bit - 1u)) & 1;
  return true;
}
}  // namespace

void spin_pair_up_table(const SectorHost& a, const SectorHost& b, int orbital, int create, std::vector<int32_t>& tab) {
  const uint32_t bit = 1u << orbital;
  const std::vector<uint32_t>& mb = b.dev_map_up();  // reference bit strings by device row
  tab.assign((size_t)b.dimup, SP_DEAD);
  for (int i = 0; i < b.dimup; ++i) {
    uint32_t m_from;
    int neg;
    if (!source_of(mb[i], bit, create, m_from, neg)) continue;
    int j = rank_in(a.map_up, m_from);
    if (j < 0) continue;  // (cannot happen between sectors nup -+ 1 of one Ns)
    if (a.row_order()) {
      j = a.up_perm[j];
      neg ^= (int)a.up_sign[j];
    }
    if (b.row_order()) neg ^= (int)b.up_sign[i];
    tab[i] = (int32_t)((uint32_t)j | ((uint32_t)neg << 31));
  }
}

void spin_pair_dw_table(const SectorHost& a, const SectorHost& b, int orbital, int create, std::vector<int32_t>& tab) {
  const uint32_t bit = 1u << orbital;
  tab.assign((size_t)b.dimdw, SP_DEAD);
  for (int c = 0; c < b.dimdw; ++c) {
    uint32_t m_from;
    int neg;
    if (!source_of(b.map_dw[c], bit, create, m_from, neg)) continue;
    const int j = rank_in(a.map_dw, m_from);
    if (j < 0) continue;
    tab[c] = (int32_t)((uint32_t)j | ((uint32_t)neg << 31));
  }
}

std::string spin_pair_key(const SectorHost& a, int create_up, int create_dw) {
  std::string k = std::to_string(a.ns) + ":" + std::to_string(a.nup) + ":" + std::to_string(a.ndw) + ":" + (create_up ? "1" : "0") + (create_dw ? "1" : "0") + ":";
  for (int32_t p : a.up_pos) k += std::to_string(p) + ",";  // empty: the reference's row order
  return k;
}

}  // namespace hxv
