// Host side of hxv_apply_spin_pair: the term plan and the per-orbital tables (hxv_spin_pair_tables.cpp, pure C++), shared by the entry point
// (hxv_spin_pair.hip) and the stand-alone check (tests/host/spin_pair_tables_check.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "hxv_internal.hpp"

namespace hxv {

constexpr int SP_PLAN_MAX_TERMS = 32;  // = HXV_MAX_SPIN_PAIR_TERMS

// The term list as the kernel wants it: the DISTINCT up and dw orbitals in order of first appearance (one table each, however often an
// orbital repeats) and, per term, which of them it uses.
struct SpPlan {
  int nterms = 0, nuq = 0, ndq = 0;
  uint8_t uq_orb[SP_PLAN_MAX_TERMS];  // [nuq] distinct up orbitals
  uint8_t dq_orb[SP_PLAN_MAX_TERMS];  // [ndq] distinct dw orbitals
  uint8_t t_uq[SP_PLAN_MAX_TERMS];    // [nterms] term -> position in uq_orb
  uint8_t t_dq[SP_PLAN_MAX_TERMS];    // [nterms] term -> position in dq_orb
  double coef[2 * SP_PLAN_MAX_TERMS]; // [nterms] complex, interleaved
};
// "" or what is wrong with the arguments (term count, an orbital outside [0, ns), a coefficient that is not finite)
std::string spin_pair_plan(int ns, int nterms, const int32_t* orb_up, const int32_t* orb_dw, const double* coef, SpPlan& plan);

// A table entry: -1 = the target is not reached, else source | sign << 31 (sign 1 = minus).
constexpr int32_t SP_DEAD = -1;
// c (create 0) / c^dagger (1) on `orbital` of spin up from sector a into sector b = (a.nup -+ 1, .): tab[b.dimup] by TARGET DEVICE row ->
// source DEVICE row of a; sign = (-1)^(occupied up orbitals below `orbital`) times the basis signs of both device rows (SectorHost::up_sign).
void spin_pair_up_table(const SectorHost& a, const SectorHost& b, int orbital, int create, std::vector<int32_t>& tab);
// the same on spin dw: tab[b.dimdw] by target column -> source column of a; the columns have no device order, the sign is the parity alone
void spin_pair_dw_table(const SectorHost& a, const SectorHost& b, int orbital, int create, std::vector<int32_t>& tab);
// what the tables of (a -> b, flags) depend on besides b itself: a's sector and its device row order
std::string spin_pair_key(const SectorHost& a, int create_up, int create_dw);

}  // namespace hxv
