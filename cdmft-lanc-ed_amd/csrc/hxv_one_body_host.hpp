// Host side of hxv_apply_one_body: the term plan and the per-(spin, i, j) tables (hxv_one_body_tables.cpp, pure C++), shared by the entry
// point (hxv_one_body.hip) and the stand-alone check (tests/host/one_body_tables_check.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "hxv_internal.hpp"

namespace hxv {

constexpr int OB_PLAN_MAX_TERMS = 32;  // = HXV_MAX_ONE_BODY_TERMS

// The term list as the kernel wants it: the DISTINCT (spin, i, j) in order of first appearance (one table each, however often a triple
// repeats) and, per term, which of them it uses.  A triple is packed as spin << 16 | i << 8 | j (one_body_triple).
struct ObPlan {
  int nterms = 0, ntab = 0;
  uint32_t tab[OB_PLAN_MAX_TERMS];     // [ntab] distinct triples
  uint8_t t_tab[OB_PLAN_MAX_TERMS];    // [nterms] term -> position in tab
  double coef[2 * OB_PLAN_MAX_TERMS];  // [nterms] complex, interleaved
};
inline uint32_t one_body_triple(int spin, int orb_to, int orb_from) { return (uint32_t)spin << 16 | (uint32_t)orb_to << 8 | (uint32_t)orb_from; }
inline int triple_spin(uint32_t t) { return (int)(t >> 16); }
inline int triple_to(uint32_t t) { return (int)(t >> 8 & 0xFFu); }
inline int triple_from(uint32_t t) { return (int)(t & 0xFFu); }
// "" or what is wrong with the arguments (term count, a spin that is not 0 or 1, an orbital outside [0, ns), a coefficient that is not finite)
std::string one_body_plan(int ns, int nterms, const int32_t* spin, const int32_t* orb_to, const int32_t* orb_from, const double* coef, ObPlan& plan);

// A table entry: -1 = the target is not reached, else source | sign << 31 (sign 1 = minus).
constexpr int32_t OB_DEAD = -1;
// c^dagger_i c_j on spin up inside sector s: tab[s.dimup] by TARGET DEVICE row -> source DEVICE row; sign = (-1)^(occupied up orbitals
// strictly between i and j) times the basis signs of both device rows (SectorHost::up_sign).  i == j: the row itself with sign + where the
// orbital is occupied (the two basis signs are the same one), -1 where it is not.
void one_body_up_table(const SectorHost& s, int orb_to, int orb_from, std::vector<int32_t>& tab);
// the same on spin dw: tab[s.dimdw] by target column -> source column; the columns have no device order, the sign is the parity alone
void one_body_dw_table(const SectorHost& s, int orb_to, int orb_from, std::vector<int32_t>& tab);

}  // namespace hxv
