// TEST-ONLY, stand-alone: the host tables of hxv_apply_one_body (csrc/hxv_one_body_tables.cpp) over sectors built by the engine's own
// builder (csrc/hxv_sector.cpp), no HIP runtime call, no device.  For every (spin, i, j) of sector (2,2) of Ns = 4, (4,3) of Ns = 6 and
// (6,6) of Ns = 12, the last with and without a forced device row order, against brute force on the bit strings:
//   every entry is -1 or a source inside the sector; a target is live exactly when it holds orbital i and (for i != j) lacks orbital j;
//   its source is the configuration with the particle moved back, at its device row; the sign is a parity counted bit by bit strictly
//   between i and j, times the basis signs of both device rows; no source is named twice; i == j names the row itself with sign +.
// Then the empty reach (nup = 0 and nup = Ns), the plan's deduplication and its argument errors.
// Prints one CASE line per sector and "OK"; exit status 1 with a message on the first failure.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "hxv_one_body_host.hpp"

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

SectorHost open_sector(const Model& mod, int nup, int ndw, bool order) {
  setenv("HXV_ROW_ORDER", order ? "1" : "0", 1);
  SectorHost s;
  const std::string e = build_sector_from_model(mod.m, nup, ndw, 0, 1, s);
  REQUIRE(e.empty(), "build_sector_from_model (%d,%d): %s", nup, ndw, e.c_str());
  return s;
}

// position of cfg in an ascending list, or -1
int find(const std::vector<uint32_t>& map, uint32_t cfg) {
  const auto it = std::lower_bound(map.begin(), map.end(), cfg);
  return it != map.end() && *it == cfg ? (int)(it - map.begin()) : -1;
}

// one table of sector s against the bit strings; -> its live entries
int check_table(const SectorHost& s, int spin, int i, int j, const std::vector<int32_t>& tab) {
  const std::vector<uint32_t>& map = spin == 0 ? s.map_up : s.map_dw;
  const bool order = spin == 0 && s.row_order();
  const int dim = (int)map.size();
  char tag[128];
  std::snprintf(tag, sizeof tag, "Ns=%d (%d,%d) order %d spin %d c+_%d c_%d", s.ns, s.nup, s.ndw, (int)s.row_order(), spin, i, j);
  REQUIRE((int)tab.size() == dim, "%s: table of %zu entries for %d targets", tag, tab.size(), dim);
  std::vector<int> hit((size_t)dim, 0);
  int live = 0;
  for (int r = 0; r < dim; ++r) {
    const uint32_t cfg = map[order ? s.up_iperm[r] : r];
    const bool has_i = (cfg >> i & 1u) != 0u, has_j = (cfg >> j & 1u) != 0u;
    const bool reached = has_i && (i == j || !has_j);
    if (!reached) {
      REQUIRE(tab[r] == OB_DEAD, "%s: target %d cannot be reached but its entry is %d", tag, r, tab[r]);
      continue;
    }
    REQUIRE(tab[r] != OB_DEAD, "%s: target %d is reached but its entry is dead", tag, r);
    const int src = tab[r] & 0x7FFFFFFF, neg = (int)((uint32_t)tab[r] >> 31);
    REQUIRE(src < dim, "%s: target %d has source %d outside [0, %d)", tag, r, src, dim);
    uint32_t from = cfg;
    if (i != j) from = (cfg & ~(1u << i)) | (1u << j);
    const int ref = find(map, from);
    REQUIRE(ref >= 0, "%s: the source configuration of target %d is not in the sector", tag, r);
    const int dev = order ? s.up_perm[ref] : ref;
    REQUIRE(src == dev, "%s: target %d has source %d, expected %d", tag, r, src, dev);
    int want = 0;
    for (int b = std::min(i, j) + 1; b < std::max(i, j); ++b) want ^= (int)(cfg >> b & 1u);
    if (order) want ^= (int)s.up_sign[dev] ^ (int)s.up_sign[r];
    REQUIRE(neg == want, "%s: target %d has sign bit %d, the parity count gives %d", tag, r, neg, want);
    if (i == j) REQUIRE(src == r && neg == 0, "%s: the occupation entry of target %d is %d", tag, r, tab[r]);
    REQUIRE(hit[src]++ == 0, "%s: source %d is named twice", tag, src);
    ++live;
  }
  return live;
}

int64_t check_sector(const SectorHost& s) {
  int64_t live = 0;
  std::vector<int32_t> tab;
  for (int i = 0; i < s.ns; ++i)
    for (int j = 0; j < s.ns; ++j) {
      one_body_up_table(s, i, j, tab);
      live += check_table(s, 0, i, j, tab);
      one_body_dw_table(s, i, j, tab);
      live += check_table(s, 1, i, j, tab);
    }
  return live;
}

void check_plan() {
  // (spin, i, j): term 3 repeats term 0, term 4 differs from term 1 in the spin alone, term 5 is term 2 backwards
  const int32_t sp[6] = {0, 1, 0, 0, 0, 0}, oi[6] = {1, 1, 2, 1, 1, 3}, oj[6] = {2, 2, 3, 2, 2, 2};
  double cf[12];
  for (int k = 0; k < 12; ++k) cf[k] = 0.5 * k - 1.0;
  ObPlan p;
  REQUIRE(one_body_plan(4, 6, sp, oi, oj, cf, p).empty(), "plan refused a good list");
  REQUIRE(p.nterms == 6 && p.ntab == 4, "plan: %d terms, %d tables", p.nterms, p.ntab);
  const uint32_t want[4] = {one_body_triple(0, 1, 2), one_body_triple(1, 1, 2), one_body_triple(0, 2, 3), one_body_triple(0, 3, 2)};
  for (int k = 0; k < 4; ++k) {
    REQUIRE(p.tab[k] == want[k], "plan: table %d is not in order of first appearance", k);
    REQUIRE(one_body_triple(triple_spin(p.tab[k]), triple_to(p.tab[k]), triple_from(p.tab[k])) == p.tab[k], "plan: triple %d does not unpack", k);
  }
  const int tt[6] = {0, 1, 2, 0, 0, 3};
  for (int t = 0; t < 6; ++t) {
    REQUIRE(p.t_tab[t] == tt[t], "plan: term %d uses table %d", t, p.t_tab[t]);
    REQUIRE(p.coef[2 * t] == cf[2 * t] && p.coef[2 * t + 1] == cf[2 * t + 1], "plan: coefficient %d", t);
  }
  // 32 terms on one triple: one table
  std::vector<int32_t> same(32, 2), zeros(32, 0);
  std::vector<double> c32(64, 1.0);
  REQUIRE(one_body_plan(4, 32, zeros.data(), same.data(), same.data(), c32.data(), p).empty() && p.ntab == 1, "plan: 32 repeats");
  REQUIRE(!one_body_plan(4, 0, sp, oi, oj, cf, p).empty() && !one_body_plan(4, 33, sp, oi, oj, cf, p).empty(), "plan: term count");
  REQUIRE(!one_body_plan(3, 6, sp, oi, oj, cf, p).empty(), "plan: orbital 3 with Ns = 3");
  const int32_t neg[1] = {-1}, zero[1] = {0}, two[1] = {2};
  REQUIRE(!one_body_plan(4, 1, zero, neg, zero, cf, p).empty() && !one_body_plan(4, 1, zero, zero, neg, cf, p).empty(), "plan: negative orbital");
  REQUIRE(!one_body_plan(4, 1, two, zero, zero, cf, p).empty() && !one_body_plan(4, 1, neg, zero, zero, cf, p).empty(), "plan: spin 2 / -1");
  double bad[2] = {std::numeric_limits<double>::quiet_NaN(), 0.0};
  REQUIRE(!one_body_plan(4, 1, zero, zero, zero, bad, p).empty(), "plan: NaN coefficient");
  bad[0] = 0.0, bad[1] = std::numeric_limits<double>::infinity();
  REQUIRE(!one_body_plan(4, 1, zero, zero, zero, bad, p).empty(), "plan: infinite coefficient");
}
}  // namespace

int main() {
  check_plan();
  setenv("HXV_ROW_ORDER_MIN_DIMUP", "16", 1);  // (the suite's hooks: a row order on a sector this small)
  setenv("HXV_ROW_ORDER_BITS", "8", 1);
  int64_t live = 0;
  const struct {
    int ns, nup, ndw, order;
  } cases[] = {{4, 2, 2, 0}, {6, 4, 3, 0}, {12, 6, 6, 0}, {12, 6, 6, 1}};
  for (const auto& c : cases) {
    Model mod(c.ns);
    const SectorHost s = open_sector(mod, c.nup, c.ndw, c.order != 0);
    REQUIRE(s.row_order() == (c.order != 0), "Ns=%d (%d,%d): row order %d asked, %d built", c.ns, c.nup, c.ndw, c.order, (int)s.row_order());
    const int64_t n = check_sector(s);
    // a hop c+_i c_j, i != j, is live on C(ns-2, n-1) configurations, an occupation on C(ns-1, n-1)
    REQUIRE(n > 0, "no live entry");
    std::printf("CASE Ns=%d (%d,%d) row order %d: %lld live entries\n", c.ns, c.nup, c.ndw, c.order, (long long)n);
    live += n;
  }
  // the empty reach: no up particle (every up table dead), every up orbital full (hops dead, occupations the identity)
  Model mod(4);
  for (int nup : {0, 4}) {
    const SectorHost s = open_sector(mod, nup, 2, false);
    std::vector<int32_t> tab;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        one_body_up_table(s, i, j, tab);
        REQUIRE(tab.size() == 1, "Ns=4 nup=%d: %zu up rows", nup, tab.size());
        const int32_t want = (nup == 4 && i == j) ? 0 : OB_DEAD;
        REQUIRE(tab[0] == want && check_table(s, 0, i, j, tab) == (want == 0 ? 1 : 0), "Ns=4 nup=%d c+_%d c_%d: entry %d", nup, i, j, tab[0]);
      }
    std::printf("CASE Ns=4 nup=%d: the empty reach\n", nup);
  }
  std::printf("live entries checked: %lld\nOK\n", (long long)live);
  return 0;
}
