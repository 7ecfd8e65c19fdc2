// TEST-ONLY, stand-alone: the host tables of hxv_apply_spin_pair (csrc/hxv_spin_pair_tables.cpp) over sectors built by the engine's own
// builder (csrc/hxv_sector.cpp), no HIP runtime call, no device.  For every pair of sectors of Ns = 4 and 6 with all four flag combinations
// and every orbital, and for a sample at Ns = 8 with a device row order forced on neither side, on the source, on the target and on both:
//   every entry is -1 or a source inside the source sector; the live entries are a bijection between the targets that hold (creation) /
//   lack (destruction) the orbital and the sources that lack / hold it; the sign equals a parity counted bit by bit here, times the basis
//   signs of both device rows; the term plan makes one table of a repeated orbital and refuses bad term lists.
// Prints one CASE line per sector pair and "OK"; exit status 1 with a message on the first failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "hxv_spin_pair_host.hpp"

using namespace hxv;

#define REQUIRE(cond, ...)                   \
  do {                                       \
    if (!(cond)) {                           \
      std::fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);     \
      std::fprintf(stderr, "\n");            \
      std::exit(1);                          \
    }                                        \
  } while (0)

namespace {
// two sites and Ns/2 - 1 bath levels per site, in the array order of hxv_model
struct Model {
  std::vector<double> hloc, hbath, vbath;
  hxv_model m{};
  explicit Model(int ns) {
    const int nlat = 2, nbath = ns / 2 - 1;
    hloc.assign(2 * nlat * nlat, 0.0);
    hloc[2 * (0 + nlat * 1)] = hloc[2 * (1 + nlat * 0)] = -0.25;
    hbath.assign((size_t)2 * nlat * nlat * nbath, 0.0);
    vbath.assign((size_t)nlat * nbath, 0.0);
    for (int ib = 0; ib < nbath; ++ib) {
      for (int i = 0; i < nlat; ++i) {
        hbath[2 * (i + nlat * i + nlat * nlat * ib)] = 0.3 * (ib + 1) - 0.5;
        hbath[2 * (i + nlat * (1 - i) + nlat * nlat * ib)] = -0.25;
        vbath[i + nlat * ib] = 0.5;
      }
    }
    m.nlat = nlat, m.norb = 1, m.nspin = 1, m.nbath = nbath, m.hfmode = 1;
    m.uloc[0] = 2.0;
    m.imphloc = hloc.data(), m.hbath = hbath.data(), m.vbath = vbath.data();
  }
};

int parity_below(uint32_t cfg, int orbital) {
  int p = 0;
  for (int b = 0; b < orbital; ++b) p ^= (int)((cfg >> b) & 1u);
  return p;
}
int find(const std::vector<uint32_t>& map, uint32_t cfg) {
  for (size_t k = 0; k < map.size(); ++k)
    if (map[k] == cfg) return (int)k;
  return -1;
}

// one spin of one (a -> b, orbital, create): tab by target (device row for spin up, column for spin dw)
void check_table(const SectorHost& a, const SectorHost& b, int spin, int orbital, int create, const std::vector<int32_t>& tab, const char* tag) {
  const std::vector<uint32_t>&ma = spin == 0 ? a.map_up : a.map_dw, &mb = spin == 0 ? b.map_up : b.map_dw;
  const int dim_a = (int)ma.size(), dim_b = (int)mb.size();
  REQUIRE((int)tab.size() == dim_b, "%s: table of %zu entries for %d targets", tag, tab.size(), dim_b);
  const uint32_t bit = 1u << orbital;
  std::vector<int> hit((size_t)dim_a, 0);
  int live = 0;
  for (int i = 0; i < dim_b; ++i) {
    const int ref_b = (spin == 0 && b.row_order()) ? b.up_iperm[i] : i;
    const uint32_t cfg = mb[ref_b];
    const bool reached = ((cfg & bit) != 0u) == (create != 0);
    if (!reached) {
      REQUIRE(tab[i] == SP_DEAD, "%s: target %d cannot be reached but its entry is %d", tag, i, tab[i]);
      continue;
    }
    REQUIRE(tab[i] != SP_DEAD, "%s: target %d is reached but its entry is dead", tag, i);
    const int src = tab[i] & 0x7FFFFFFF, neg = (int)((uint32_t)tab[i] >> 31);
    REQUIRE(src >= 0 && src < dim_a, "%s: target %d has source %d outside [0, %d)", tag, i, src, dim_a);
    const int ref_a = find(ma, cfg ^ bit);
    REQUIRE(ref_a >= 0, "%s: the source configuration of target %d is not in the source sector", tag, i);
    const int dev_a = (spin == 0 && a.row_order()) ? a.up_perm[ref_a] : ref_a;
    REQUIRE(src == dev_a, "%s: target %d has source %d, expected %d", tag, i, src, dev_a);
    int want = parity_below(cfg ^ bit, orbital);
    if (spin == 0 && a.row_order()) want ^= (int)a.up_sign[dev_a];
    if (spin == 0 && b.row_order()) want ^= (int)b.up_sign[i];
    REQUIRE(neg == want, "%s: target %d has sign bit %d, the parity count gives %d", tag, i, neg, want);
    REQUIRE(hit[src]++ == 0, "%s: source %d is named twice", tag, src);
    ++live;
  }
  int sources = 0;
  for (int j = 0; j < dim_a; ++j) sources += (((ma[j] & bit) != 0u) != (create != 0)) ? 1 : 0;
  REQUIRE(live == sources, "%s: %d live entries for %d sources that can be moved", tag, live, sources);
}

int64_t check_pair(const SectorHost& a, const SectorHost& b, int cu, int cd) {
  int64_t n = 0;
  std::vector<int32_t> tab;
  char tag[160];
  for (int o = 0; o < a.ns; ++o) {
    std::snprintf(tag, sizeof tag, "Ns=%d (%d,%d)->(%d,%d) up orbital %d create %d orders %d%d", a.ns, a.nup, a.ndw, b.nup, b.ndw, o, cu, (int)a.row_order(), (int)b.row_order());
    spin_pair_up_table(a, b, o, cu, tab);
    check_table(a, b, 0, o, cu, tab, tag);
    n += (int64_t)tab.size();
    std::snprintf(tag, sizeof tag, "Ns=%d (%d,%d)->(%d,%d) dw orbital %d create %d", a.ns, a.nup, a.ndw, b.nup, b.ndw, o, cd);
    spin_pair_dw_table(a, b, o, cd, tab);
    check_table(a, b, 1, o, cd, tab, tag);
    n += (int64_t)tab.size();
  }
  return n;
}

SectorHost open_sector(const Model& mod, int nup, int ndw, bool order) {
  setenv("HXV_ROW_ORDER", order ? "1" : "0", 1);
  SectorHost s;
  const std::string e = build_sector_from_model(mod.m, nup, ndw, 0, 1, s);
  REQUIRE(e.empty(), "build_sector_from_model (%d,%d): %s", nup, ndw, e.c_str());
  return s;
}

void check_plan() {
  const int32_t ou[5] = {1, 1, 0, 1, 3}, od[5] = {2, 3, 2, 2, 2};
  double cf[10];
  for (int k = 0; k < 10; ++k) cf[k] = 0.5 * k - 1.0;
  SpPlan p;
  REQUIRE(spin_pair_plan(4, 5, ou, od, cf, p).empty(), "plan refused a good list");
  REQUIRE(p.nterms == 5 && p.nuq == 3 && p.ndq == 2, "plan: %d terms, %d up tables, %d dw tables", p.nterms, p.nuq, p.ndq);
  REQUIRE(p.uq_orb[0] == 1 && p.uq_orb[1] == 0 && p.uq_orb[2] == 3 && p.dq_orb[0] == 2 && p.dq_orb[1] == 3, "plan: order of first appearance");
  const int tu[5] = {0, 0, 1, 0, 2}, td[5] = {0, 1, 0, 0, 0};
  for (int t = 0; t < 5; ++t) {
    REQUIRE(p.t_uq[t] == tu[t] && p.t_dq[t] == td[t], "plan: term %d uses tables %d, %d", t, p.t_uq[t], p.t_dq[t]);
    REQUIRE(p.coef[2 * t] == cf[2 * t] && p.coef[2 * t + 1] == cf[2 * t + 1], "plan: coefficient %d", t);
  }
  // 32 terms on one orbital pair: one table each
  std::vector<int32_t> same(32, 2);
  std::vector<double> c32(64, 1.0);
  REQUIRE(spin_pair_plan(4, 32, same.data(), same.data(), c32.data(), p).empty() && p.nuq == 1 && p.ndq == 1, "plan: 32 repeats");
  REQUIRE(!spin_pair_plan(4, 0, ou, od, cf, p).empty() && !spin_pair_plan(4, 33, ou, od, cf, p).empty(), "plan: term count");
  REQUIRE(!spin_pair_plan(3, 5, ou, od, cf, p).empty(), "plan: orbital 3 with Ns = 3");
  const int32_t neg[1] = {-1}, zero[1] = {0};
  REQUIRE(!spin_pair_plan(4, 1, neg, zero, cf, p).empty() && !spin_pair_plan(4, 1, zero, neg, cf, p).empty(), "plan: negative orbital");
  double bad[2] = {std::numeric_limits<double>::quiet_NaN(), 0.0};
  REQUIRE(!spin_pair_plan(4, 1, zero, zero, bad, p).empty(), "plan: NaN coefficient");
  bad[0] = 0.0, bad[1] = std::numeric_limits<double>::infinity();
  REQUIRE(!spin_pair_plan(4, 1, zero, zero, bad, p).empty(), "plan: infinite coefficient");
}
}  // namespace

int main() {
  check_plan();
  int64_t entries = 0;
  for (int ns : {4, 6}) {
    Model mod(ns);
    int pairs = 0;
    for (int nup = 0; nup <= ns; ++nup)
      for (int ndw = 0; ndw <= ns; ++ndw) {
        const SectorHost a = open_sector(mod, nup, ndw, true);
        for (int cu = 0; cu < 2; ++cu)
          for (int cd = 0; cd < 2; ++cd) {
            const int tu = nup + (cu ? 1 : -1), td = ndw + (cd ? 1 : -1);
            if (tu < 0 || tu > ns || td < 0 || td > ns) continue;
            const SectorHost b = open_sector(mod, tu, td, true);
            entries += check_pair(a, b, cu, cd);
            ++pairs;
          }
      }
    std::printf("CASE Ns=%d sector pairs x flags = %d\n", ns, pairs);
  }
  // Ns = 8 with the device row order forced (the suite's hooks): on neither side, on the source, on the target, on both
  setenv("HXV_ROW_ORDER_MIN_DIMUP", "16", 1);
  setenv("HXV_ROW_ORDER_BITS", "4", 1);
  Model mod(8);
  int with_order = 0;
  for (int nup : {3, 4})
    for (int cu = 0; cu < 2; ++cu)
      for (int cd = 0; cd < 2; ++cd)
        for (int oa = 0; oa < 2; ++oa)
          for (int ob = 0; ob < 2; ++ob) {
            const int ndw = 4;
            const SectorHost a = open_sector(mod, nup, ndw, oa != 0), b = open_sector(mod, nup + (cu ? 1 : -1), ndw + (cd ? 1 : -1), ob != 0);
            REQUIRE(a.row_order() == (oa != 0) && b.row_order() == (ob != 0), "Ns=8 (%d,%d): row order %d%d asked, %d%d built", nup, ndw, oa, ob,
                    (int)a.row_order(), (int)b.row_order());
            REQUIRE((spin_pair_key(a, cu, cd) == spin_pair_key(open_sector(mod, nup, ndw, oa == 0), cu, cd)) == false,
                    "Ns=8: the cache key does not tell the two row orders of the source apart");
            entries += check_pair(a, b, cu, cd);
            with_order += oa + ob;
          }
  std::printf("CASE Ns=8 with a forced row order: %d sides\n", with_order);
  std::printf("entries checked: %lld\nOK\n", (long long)entries);
  return 0;
}
