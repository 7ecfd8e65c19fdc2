// The group enumerations of the two partial traces (hxv_partial_trace_host.hpp: PtGroups).  The order of the groups fixes the order of the
// sums, and so the bits of the result.  Host C++ only: no device, no HIP runtime call.
//   cluster_dm_groups   rho_imp = Tr_bath |psi><psi| (density_matrix_impurity, ED_OBSERVABLES.f90:465-582).  A spin configuration is
//                       a + 2^Nimp * b (impurity bits low, bath bits high, :539-562) and the basis maps are sorted by that integer, so the rows
//                       that share the bath configuration b are a contiguous run of the reference's order: the groups are those runs, by
//                       ascending b.  No sign but the basis signs of the device row order.
//   reduced_dm_groups   rho_S = Tr_env |psi><psi|, env = every orbital outside the subset S of the impurity orbitals (the reference's
//                       ed_get_reduced_density_matrix_single, ED_IO/get_reduced_dm.f90:68-212, without the dense cluster matrix it traces).  A
//                       configuration m splits into the bits of S (compressed, ascending orbital order) and e = m & ~S; the rows of one e are
//                       no run any more.  Up groups by their lowest device row, dw groups by their lowest column.
//                       fermi_sign 0: the plain partial trace, what the reference computes (its get_sign, :170-191, depends on the traced
//                       bits alone, which the two states of a contributing pair share, :145).  fermi_sign 1: every basis state carries
//                       (-1)^n, n = sum over the occupied r in S of the occupied orbitals outside S below r: the Jordan-Wigner string of
//                       moving the operators of S in front of the others; a factor per row times a factor per column.
#include <algorithm>

#include "hxv_internal.hpp"
#include "hxv_partial_trace_host.hpp"

namespace hxv {
namespace {
// the device row of reference row i, with its basis sign
uint32_t row_entry(const SectorHost& s, int i) {
  if (!s.row_order()) return (uint32_t)i;
  const uint32_t r = (uint32_t)s.up_perm[i];
  return r | (s.up_sign[r] ? 0x80000000u : 0u);
}

// 1: the configuration carries a minus sign in the fermi_sign = 1 convention
uint32_t fermi_bit(uint32_t m, uint32_t S) {
  int n = 0;
  for (uint32_t b = S & m; b; b &= b - 1) n += __builtin_popcount(m & ~S & ((b & (0u - b)) - 1u));
  return (uint32_t)(n & 1);
}

// the groups of one spin: indices of a sorted basis map that share m & ~S, members in ascending order (= ascending compressed S bits)
struct Group {
  uint32_t env;
  std::vector<int32_t> idx;
};
std::vector<Group> env_groups(const std::vector<uint32_t>& map, uint32_t S) {
  std::vector<int32_t> order(map.size());
  for (size_t i = 0; i < map.size(); ++i) order[i] = (int32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return (map[a] & ~S) < (map[b] & ~S); });
  std::vector<Group> g;
  for (int32_t i : order) {
    if (g.empty() || g.back().env != (map[i] & ~S)) g.push_back(Group{map[i] & ~S, {}});
    g.back().idx.push_back(i);
  }
  return g;
}
}  // namespace

std::string cluster_dm_groups(const SectorHost& s, int nimp, PtGroups& up, PtGroups& dw) {
  const int nbath = s.ns - nimp;
  up.assign(nbath + 1, {});
  dw.assign(nbath + 1, {});
  // runs of equal bath configuration in a sorted basis map
  auto runs = [&](const std::vector<uint32_t>& map, int npart, bool rows, PtGroups& out) {
    for (size_t i = 0, j; i < map.size(); i = j) {
      for (j = i + 1; j < map.size() && (map[j] >> nimp) == (map[i] >> nimp); ++j) {
      }
      const int k = __builtin_popcount(map[i] >> nimp);
      if (k > nbath || (int64_t)(j - i) != binom(nimp, npart - k)) return false;
      for (size_t m = i; m < j; ++m) out[k].push_back(rows ? row_entry(s, (int)m) : (uint32_t)m);
    }
    return true;
  };
  if (!runs(s.map_up, s.nup, true, up)) return "cluster density matrix: the up basis is not sorted by bath configuration";
  if (!runs(s.map_dw, s.ndw, false, dw)) return "cluster density matrix: the dw basis is not sorted by bath configuration";
  return std::string();
}

std::string reduced_dm_groups(const SectorHost& s, uint32_t S, int fermi_sign, PtGroups& up, PtGroups& dw) {
  const int nred = __builtin_popcount(S), kmax = s.ns - nred;
  up.assign(kmax + 1, {});
  dw.assign(kmax + 1, {});
  struct Keyed {
    uint32_t first;
    std::vector<uint32_t> e;
  };
  std::vector<std::vector<Keyed>> byk(kmax + 1);
  for (const Group& g : env_groups(s.map_up, S)) {
    const int k = __builtin_popcount(g.env);
    if (k > kmax || (int64_t)g.idx.size() != binom(nred, s.nup - k)) return "reduced density matrix: the up basis does not hold every configuration of the subset";
    Keyed kd{0xffffffffu, {}};
    for (int32_t i : g.idx) {
      const uint32_t r = row_entry(s, i);
      kd.e.push_back(fermi_sign && fermi_bit(s.map_up[i], S) ? r ^ 0x80000000u : r);
      kd.first = std::min(kd.first, r & 0x7fffffffu);
    }
    byk[k].push_back(std::move(kd));
  }
  for (int k = 0; k <= kmax; ++k) {
    std::sort(byk[k].begin(), byk[k].end(), [](const Keyed& a, const Keyed& b) { return a.first < b.first; });
    for (const Keyed& kd : byk[k]) up[k].insert(up[k].end(), kd.e.begin(), kd.e.end());
  }
  std::vector<Group> dg = env_groups(s.map_dw, S);
  std::sort(dg.begin(), dg.end(), [](const Group& a, const Group& b) { return a.idx[0] < b.idx[0]; });
  for (const Group& g : dg) {
    const int k = __builtin_popcount(g.env);
    if (k > kmax || (int64_t)g.idx.size() != binom(nred, s.ndw - k)) return "reduced density matrix: the dw basis does not hold every configuration of the subset";
    for (int32_t c : g.idx) dw[k].push_back((uint32_t)c | ((fermi_sign ? fermi_bit(s.map_dw[c], S) : 0u) << 31));
  }
  return std::string();
}
}  // namespace hxv
