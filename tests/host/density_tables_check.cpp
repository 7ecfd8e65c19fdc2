// TEST-ONLY, stand-alone: the host tables of hxv_observables_accumulate and hxv_apply_density_ops (csrc/hxv_observables_tables.cpp,
// csrc/hxv_density_ops_tables.cpp) over sectors built by the engine's own builder (csrc/hxv_sector.cpp), no HIP runtime call, no device.
// Ring models of Nimp sites with Nbath levels per site, Ns = Nimp (Nbath + 1) from 4 to 10 and Nimp in {1, 3, 4, 5, 6, 10 = Ns}; every
// sector in the reference's row order and in a forced device row order, whole and split over 2 and 3 ranks (every rank's tables), and split
// over DimDw + 2 ranks, where the last two own no column (the sector builder refuses such a split -- the driver shrinks the communicator
// first -- so the split is re-done on the sector by dw_split and make_vcol, which is all the table builders read of it); sectors with
// DimUp = 1 and with DimDw = 1.  Every table is rebuilt by brute force from the bit strings:
//   observables  each device row sits in exactly one W bin, the bin of its low Nimp bits, as (r, r, +1); a pair group p = is + Nimp js with
//                is < js holds exactly the rows with js occupied and is empty, once each, the partner row is the device row of the
//                configuration with the particle moved, the sign is the parity counted bit by bit strictly between is and js times both
//                basis signs; groups with is >= js are empty; each column's dw pairs name distinct p, exactly the applicable ones, and a
//                slot that decodes to the owner rank and the index in its slab of the moved configuration; dwbin_cols is a permutation of
//                this rank's columns, grouped by dw bits.
//   density ops  occ_up is the low Nimp bits by device row and zero on the pad rows, occ_dw the same by local column; nchunk * rows >= pitch
//                with the fewest chunks of at most DOP_CHUNK rows, rows % 8 == 0; nitems = qdw * nchunk; grid = clamp(nitems, 1, 8 ncu) for
//                several ncu.  The chunking of pitches beyond 2048 rows on sectors that hold nothing but their sizes.
// Prints one CASE line per sector and "OK"; exit status 1 with a message on the first failure.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "hxv_density_host.hpp"

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
// nlat sites on a ring (a chain below three sites), nbath levels under every site, one orbital, one spin block: the array order of hxv_model
struct Model {
  std::vector<double> hloc, hbath, vbath;
  hxv_model m{};
  Model(int nlat, int nbath) {
    hloc.assign((size_t)2 * nlat * nlat, 0.0);
    for (int i = 0; i + 1 < nlat; ++i) hloc[2 * (i + nlat * (i + 1))] = hloc[2 * ((i + 1) + nlat * i)] = -0.25;
    if (nlat >= 3) hloc[2 * (0 + nlat * (nlat - 1))] = hloc[2 * ((nlat - 1) + nlat * 0)] = -0.25;
    hbath.assign((size_t)2 * nlat * nlat * std::max(nbath, 1), 0.0);
    vbath.assign((size_t)nlat * std::max(nbath, 1), 0.0);
    for (int ib = 0; ib < nbath; ++ib)
      for (int i = 0; i < nlat; ++i) {
        hbath[2 * (i + nlat * i + (size_t)nlat * nlat * ib)] = 0.3 * (ib + 1) - 0.5;
        vbath[i + nlat * ib] = 0.5;
      }
    m.nlat = nlat, m.norb = 1, m.nspin = 1, m.nbath = nbath, m.hfmode = 1;
    m.uloc[0] = 2.0;
    m.imphloc = hloc.data(), m.hbath = hbath.data(), m.vbath = vbath.data();
  }
};

// the block bits that make plan_row_order move an orbital: the bath of site 0 (not tied to a high orbital) ahead of the sites 1.. (tied to
// their baths); without a bath the ring's closing hop ties orbital 0 to the last one
int order_bits(int nlat, int nbath) { return nbath > 0 ? nlat + 1 : nlat - 2; }

SectorHost open_sector(const Model& mod, int nup, int ndw, bool order, int rank, int nranks) {
  setenv("HXV_ROW_ORDER", order ? "1" : "0", 1);
  setenv("HXV_ROW_ORDER_MIN_DIMUP", "2", 1);
  setenv("HXV_ROW_ORDER_BITS", std::to_string(order_bits(mod.m.nlat, mod.m.nbath)).c_str(), 1);
  SectorHost s;
  const std::string e = build_sector_from_model(mod.m, nup, ndw, rank, nranks, s);
  REQUIRE(e.empty(), "build_sector_from_model (%d,%d) rank %d of %d: %s", nup, ndw, rank, nranks, e.c_str());
  return s;
}

int find(const std::vector<uint32_t>& map, uint32_t cfg) {
  const auto it = std::lower_bound(map.begin(), map.end(), cfg);
  return it != map.end() && *it == cfg ? (int)(it - map.begin()) : -1;
}
// (-1)^(occupied orbitals strictly between a and b), counted bit by bit, as 0 / 1
int parity_between(uint32_t cfg, int a, int b) {
  int par = 0;
  for (int k = std::min(a, b) + 1; k < std::max(a, b); ++k) par ^= (int)(cfg >> k & 1u);
  return par;
}
// the reference bit string of device row r
uint32_t cfg_of(const SectorHost& s, int r) { return s.map_up[s.row_order() ? s.up_iperm[r] : r]; }

int64_t check_observables(const SectorHost& s, int nimp, const char* tag) {
  ObsHostTables t;
  const std::string err = obs_build_tables(s, nimp, t);
  REQUIRE(err.empty(), "%s: obs_build_tables: %s", tag, err.c_str());
  const int nw = 1 << nimp, np = nimp * nimp, qdw = std::max(s.qdw, 0);
  const uint32_t mask = (uint32_t)nw - 1u;
  REQUIRE(t.nimp == nimp && t.nw == nw && t.np == np && t.gtot == nw + 2 * np, "%s: sizes %d %d %d %d", tag, t.nimp, t.nw, t.np, t.gtot);
  const int64_t nent = (int64_t)t.ent_a.size();
  REQUIRE((int)t.seg_ptr.size() == nw + np + 1 && t.seg_ptr[0] == 0 && t.seg_ptr[nw + np] == nent, "%s: seg_ptr ends", tag);
  REQUIRE((int64_t)t.ent_b.size() == nent && (int64_t)t.ent_s.size() == nent, "%s: entry arrays of different lengths", tag);
  for (int g = 0; g < nw + np; ++g) REQUIRE(t.seg_ptr[g] <= t.seg_ptr[g + 1], "%s: seg_ptr decreases at group %d", tag, g);
  for (int64_t e = 0; e < nent; ++e)
    REQUIRE(t.ent_a[e] >= 0 && t.ent_a[e] < s.dimup && t.ent_b[e] >= 0 && t.ent_b[e] < s.dimup && (t.ent_s[e] == 1 || t.ent_s[e] == -1),
            "%s: entry %lld (%d, %d, %d) outside the column", tag, (long long)e, t.ent_a[e], t.ent_b[e], (int)t.ent_s[e]);
  // W bins
  std::vector<int> seen((size_t)s.dimup, 0);
  for (int g = 0; g < nw; ++g)
    for (int e = t.seg_ptr[g]; e < t.seg_ptr[g + 1]; ++e) {
      const int r = t.ent_a[e];
      REQUIRE(t.ent_b[e] == r && t.ent_s[e] == 1, "%s: W bin %d holds (%d, %d, %d)", tag, g, r, t.ent_b[e], (int)t.ent_s[e]);
      REQUIRE((cfg_of(s, r) & mask) == (uint32_t)g, "%s: row %d with impurity bits %u sits in W bin %d", tag, r, cfg_of(s, r) & mask, g);
      ++seen[r];
    }
  REQUIRE(t.seg_ptr[nw] == s.dimup, "%s: %d rows in the W bins of %d", tag, t.seg_ptr[nw], s.dimup);
  for (int r = 0; r < s.dimup; ++r) REQUIRE(seen[r] == 1, "%s: row %d sits in %d W bins", tag, r, seen[r]);
  // pair groups
  for (int p = 0; p < np; ++p) {
    const int is = p % nimp, js = p / nimp, e0 = t.seg_ptr[nw + p], e1 = t.seg_ptr[nw + p + 1];
    if (is >= js) {
      REQUIRE(e0 == e1, "%s: pair group (%d,%d) holds %d entries", tag, is, js, e1 - e0);
      continue;
    }
    std::fill(seen.begin(), seen.end(), 0);
    for (int e = e0; e < e1; ++e) {
      const int a = t.ent_a[e], b = t.ent_b[e];
      const uint32_t ca = cfg_of(s, a);
      REQUIRE((ca >> js & 1u) && !(ca >> is & 1u), "%s: pair (%d,%d) names row %d, which it does not act on", tag, is, js, a);
      REQUIRE(seen[a]++ == 0, "%s: pair (%d,%d) names row %d twice", tag, is, js, a);
      const uint32_t cb = (ca & ~(1u << js)) | (1u << is);
      const int ref = find(s.map_up, cb);
      REQUIRE(ref >= 0, "%s: the image of row %d is not in the sector", tag, a);
      const int dev = s.row_order() ? s.up_perm[ref] : ref;
      REQUIRE(b == dev, "%s: pair (%d,%d) row %d: partner %d, expected %d", tag, is, js, a, b, dev);
      int neg = parity_between(ca, is, js);
      if (s.row_order()) neg ^= (int)s.up_sign[a] ^ (int)s.up_sign[dev];
      REQUIRE(t.ent_s[e] == (neg ? -1 : 1), "%s: pair (%d,%d) row %d: sign %d, the parity count gives %d", tag, is, js, a, (int)t.ent_s[e], neg ? -1 : 1);
    }
    for (int r = 0; r < s.dimup; ++r) {
      const uint32_t c = cfg_of(s, r);
      const bool want = (c >> js & 1u) && !(c >> is & 1u);
      REQUIRE(seen[r] == (want ? 1 : 0), "%s: pair (%d,%d) %s row %d", tag, is, js, want ? "misses" : "names", r);
    }
  }
  // dw pairs
  std::vector<int> first(s.nranks + 1, 0), count(s.nranks, 0);
  for (int o = 0; o < s.nranks; ++o) dw_split(s.dimdw, o, s.nranks, count[o], first[o]);
  const int64_t ndwp = (int64_t)t.dwp_slot.size();
  REQUIRE((int)t.dwp_ptr.size() == qdw + 1 && t.dwp_ptr[0] == 0 && t.dwp_ptr[qdw] == ndwp, "%s: dwp_ptr ends", tag);
  REQUIRE((int64_t)t.dwp_p.size() == ndwp && (int64_t)t.dwp_s.size() == ndwp, "%s: dw pair arrays of different lengths", tag);
  std::vector<int> named((size_t)np);
  for (int c = 0; c < qdw; ++c) {
    REQUIRE(t.dwp_ptr[c] <= t.dwp_ptr[c + 1], "%s: dwp_ptr decreases at column %d", tag, c);
    const uint32_t m = s.map_dw[s.dw0 + c];
    std::fill(named.begin(), named.end(), 0);
    for (int k = t.dwp_ptr[c]; k < t.dwp_ptr[c + 1]; ++k) {
      const int p = t.dwp_p[k];
      REQUIRE(p >= 0 && p < np, "%s: column %d names pair %d", tag, c, p);
      const int is = p % nimp, js = p / nimp;
      REQUIRE(is < js && (m >> js & 1u) && !(m >> is & 1u), "%s: column %d names pair (%d,%d), which does not act on it", tag, c, is, js);
      REQUIRE(named[p]++ == 0, "%s: column %d names pair %d twice", tag, c, p);
      const int cj = find(s.map_dw, (m & ~(1u << js)) | (1u << is));
      REQUIRE(cj >= 0, "%s: the image of column %d is not in the sector", tag, c);
      const int slot = t.dwp_slot[k];
      if (s.nranks == 1) {
        REQUIRE(slot == cj, "%s: column %d pair %d: slot %d, expected column %d", tag, c, p, slot, cj);
      } else {
        REQUIRE(slot >= 0 && slot < s.nranks * s.cmax, "%s: column %d pair %d: slot %d outside the gathered copy", tag, c, p, slot);
        const int o = slot / s.cmax, idx = slot % s.cmax;
        REQUIRE(idx < count[o] && first[o] + idx == cj, "%s: column %d pair %d: slot %d = rank %d index %d is not column %d", tag, c, p, slot, o,
                idx, cj);
      }
      REQUIRE(t.dwp_s[k] == (parity_between(m, is, js) ? -1 : 1), "%s: column %d pair %d: sign %d", tag, c, p, (int)t.dwp_s[k]);
    }
    for (int p = 0; p < np; ++p) {
      const int is = p % nimp, js = p / nimp;
      const bool want = is < js && (m >> js & 1u) && !(m >> is & 1u);
      REQUIRE(named[p] == (want ? 1 : 0), "%s: column %d %s pair %d", tag, c, want ? "misses" : "names", p);
    }
  }
  // dw bins
  REQUIRE((int)t.dwbin_ptr.size() == nw + 1 && t.dwbin_ptr[0] == 0 && t.dwbin_ptr[nw] == qdw && (int)t.dwbin_cols.size() == qdw, "%s: dwbin ends", tag);
  std::vector<int> cseen((size_t)qdw, 0);
  for (int g = 0; g < nw; ++g) {
    REQUIRE(t.dwbin_ptr[g] <= t.dwbin_ptr[g + 1], "%s: dwbin_ptr decreases at bin %d", tag, g);
    for (int k = t.dwbin_ptr[g]; k < t.dwbin_ptr[g + 1]; ++k) {
      const int c = t.dwbin_cols[k];
      REQUIRE(c >= 0 && c < qdw && cseen[c]++ == 0, "%s: dw bin %d names column %d (outside the slab or twice)", tag, g, c);
      REQUIRE((s.map_dw[s.dw0 + c] & mask) == (uint32_t)g, "%s: column %d sits in dw bin %d", tag, c, g);
    }
  }
  return nent + ndwp + qdw;
}

void check_chunking(const DopHostTables& t, int pitch, int qdw, int ncu, const char* tag) {
  REQUIRE(t.nchunk >= 1 && t.rows >= 8 && t.rows % 8 == 0 && t.rows <= DOP_CHUNK, "%s: nchunk %d rows %d", tag, t.nchunk, t.rows);
  REQUIRE((int64_t)t.nchunk * t.rows >= pitch, "%s: %d chunks of %d rows do not cover the pitch %d", tag, t.nchunk, t.rows, pitch);
  REQUIRE((int64_t)(t.nchunk - 1) * DOP_CHUNK < pitch, "%s: %d chunks for a pitch of %d", tag, t.nchunk, pitch);
  REQUIRE((int64_t)(t.nchunk - 1) * t.rows < pitch, "%s: the last of %d chunks of %d rows lies beyond the pitch %d", tag, t.nchunk, t.rows, pitch);
  REQUIRE(t.nitems == (int64_t)std::max(qdw, 0) * t.nchunk, "%s: %lld work items", tag, (long long)t.nitems);
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>(t.nitems, (int64_t)DOP_WG_PER_CU * ncu));
  REQUIRE(t.grid == want, "%s: grid %d with %d CUs, expected %lld", tag, t.grid, ncu, (long long)want);
}

void check_density_ops(const SectorHost& s, int nimp, const char* tag) {
  const uint32_t mask = (1u << nimp) - 1u;
  for (int ncu : {1, 4, 256, 304}) {
    DopHostTables t;
    const std::string err = dop_build_tables(s, nimp, ncu, t);
    REQUIRE(err.empty(), "%s: dop_build_tables: %s", tag, err.c_str());
    REQUIRE((int)t.occ_up.size() == s.pitch && (int)t.occ_dw.size() == std::max(s.qdw, 1), "%s: occupation lists of %zu and %zu words", tag,
            t.occ_up.size(), t.occ_dw.size());
    for (int r = 0; r < s.pitch; ++r)
      REQUIRE(t.occ_up[r] == (r < s.dimup ? cfg_of(s, r) & mask : 0u), "%s: occ_up[%d] = %u", tag, r, t.occ_up[r]);
    for (int c = 0; c < (int)t.occ_dw.size(); ++c)
      REQUIRE(t.occ_dw[c] == (c < s.qdw ? s.map_dw[s.dw0 + c] & mask : 0u), "%s: occ_dw[%d] = %u", tag, c, t.occ_dw[c]);
    check_chunking(t, s.pitch, s.qdw, ncu, tag);
  }
}

// the chunking of a pitch no small sector has: a sector that holds nothing but its sizes and two lists of words
void check_large_pitch(int dimup, int qdw, int want_nchunk, int want_rows) {
  SectorHost s;
  s.ns = 24, s.dimup = dimup, s.pitch = (dimup + 7) & ~7, s.dimdw = s.qdw = qdw, s.cmax = qdw;
  s.map_up.resize((size_t)dimup);
  for (int r = 0; r < dimup; ++r) s.map_up[r] = (uint32_t)r * 2654435761u >> 8;
  s.map_dw.resize((size_t)qdw);
  for (int c = 0; c < qdw; ++c) s.map_dw[c] = 1000u + 37u * (uint32_t)c;
  char tag[96];
  std::snprintf(tag, sizeof tag, "DimUp %d x %d columns", dimup, qdw);
  for (int ncu : {1, 256}) {
    DopHostTables t;
    REQUIRE(dop_build_tables(s, 10, ncu, t).empty(), "%s: dop_build_tables", tag);
    REQUIRE(t.nchunk == want_nchunk && t.rows == want_rows, "%s: %d chunks of %d rows, expected %d of %d", tag, t.nchunk, t.rows, want_nchunk, want_rows);
    check_chunking(t, s.pitch, qdw, ncu, tag);
    for (int r = 0; r < s.pitch; ++r) REQUIRE(t.occ_up[r] == (r < dimup ? s.map_up[r] & 1023u : 0u), "%s: occ_up[%d]", tag, r);
  }
  std::printf("CASE %s: pitch %d in %d chunks of %d rows\n", tag, s.pitch, want_nchunk, want_rows);
}
}  // namespace

int main() {
  const struct {
    int nlat, nbath, nup, ndw;
  } cases[] = {
      {1, 3, 2, 2}, {1, 3, 0, 2}, {1, 3, 4, 1}, {1, 3, 2, 0}, {1, 3, 2, 4},  // Ns 4, Nimp 1; DimUp = 1 (empty, full), DimDw = 1
      {5, 0, 2, 3},                                                            // Ns 5, Nimp 5 = Ns
      {3, 1, 3, 2}, {6, 0, 3, 3}, {6, 0, 2, 4},                                // Ns 6, Nimp 3 and 6 = Ns
      {1, 6, 3, 4},                                                            // Ns 7, Nimp 1
      {4, 1, 4, 3},                                                            // Ns 8, Nimp 4
      {3, 2, 4, 3},                                                            // Ns 9, Nimp 3
      {5, 1, 5, 4}, {10, 0, 5, 4}, {10, 0, 0, 5}, {10, 0, 5, 10},              // Ns 10, Nimp 5 and 10 = Ns; DimUp = 1, DimDw = 1
  };
  int64_t total = 0;
  int ordered = 0;
  for (const auto& c : cases) {
    const Model mod(c.nlat, c.nbath);
    const int nimp = c.nlat, ns = c.nlat * (c.nbath + 1);
    int64_t n = 0;
    int norders = 0;
    for (int order = 0; order < 2; ++order) {
      const SectorHost whole = open_sector(mod, c.nup, c.ndw, order != 0, 0, 1);
      REQUIRE(nimp_of(whole) == nimp && whole.ns == ns, "Ns=%d Nimp=%d: the sector says Ns=%d Nimp=%d", ns, nimp, whole.ns, nimp_of(whole));
      if (order && !whole.row_order()) {
        REQUIRE(whole.dimup < 4, "Ns=%d Nimp=%d (%d,%d): no device row order on %d up rows", ns, nimp, c.nup, c.ndw, whole.dimup);
        continue;  // (one or two rows: nothing to reorder)
      }
      REQUIRE(whole.row_order() == (order != 0), "Ns=%d (%d,%d): row order %d asked", ns, c.nup, c.ndw, order);
      if (order) {
        bool moved = false, minus = false;
        for (int r = 0; r < whole.dimup; ++r) moved = moved || whole.up_iperm[r] != r, minus = minus || whole.up_sign[r] != 0;
        REQUIRE(moved, "Ns=%d (%d,%d): the forced row order moves no row", ns, c.nup, c.ndw);
        if (minus) ++ordered;
      }
      ++norders;
      char tag[128];
      for (int nranks = 1; nranks <= 3 && nranks <= whole.dimdw; ++nranks)
        for (int rank = 0; rank < nranks; ++rank) {
          const SectorHost s = nranks == 1 ? whole : open_sector(mod, c.nup, c.ndw, order != 0, rank, nranks);
          std::snprintf(tag, sizeof tag, "Ns=%d Nimp=%d (%d,%d) order %d rank %d/%d", ns, nimp, c.nup, c.ndw, order, rank, nranks);
          n += check_observables(s, nimp, tag);
          check_density_ops(s, nimp, tag);
        }
      // more ranks than columns: the last two own none
      SectorHost s = whole;
      s.nranks = whole.dimdw + 2;
      int empty = 0;
      for (int rank = 0; rank < s.nranks; ++rank) {
        s.rank = rank;
        dw_split(s.dimdw, rank, s.nranks, s.qdw, s.dw0);
        make_vcol(s);
        REQUIRE(s.cmax == 1, "%d ranks on %d columns: cmax %d", s.nranks, s.dimdw, s.cmax);
        empty += s.qdw == 0;
        std::snprintf(tag, sizeof tag, "Ns=%d Nimp=%d (%d,%d) order %d rank %d/%d", ns, nimp, c.nup, c.ndw, order, rank, s.nranks);
        n += check_observables(s, nimp, tag);
        check_density_ops(s, nimp, tag);
      }
      REQUIRE(empty == 2, "%d ranks on %d columns: %d own none", s.nranks, s.dimdw, empty);
    }
    REQUIRE(n > 0, "nothing checked");
    std::printf("CASE Ns=%d Nimp=%d (%d,%d): %d row orders, 1..3 ranks and DimDw+2 ranks: %lld table entries\n", ns, nimp, c.nup, c.ndw, norders,
                (long long)n);
    total += n;
  }
  REQUIRE(ordered >= 8, "only %d sectors had a device row order with a minus sign in it", ordered);
  check_large_pitch(2041, 3, 1, 2048);
  check_large_pitch(2049, 2, 2, 1032);
  check_large_pitch(4097, 3, 3, 1368);
  check_large_pitch(6150, 1, 4, 1544);
  std::printf("table entries checked: %lld\nOK\n", (long long)total);
  return 0;
}
