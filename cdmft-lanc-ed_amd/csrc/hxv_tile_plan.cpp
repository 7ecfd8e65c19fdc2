// Host side of the tiled product: the tile-plan builder, the geometry of the pipelined job kernel and the decisions
// the launchers take from (DevSector, TilePlan, flags).  No device code and no HIP runtime call: the launchers are in hxv_tiled.hip and
// hxv_jobs.hip, and tests/host/plan_check.cpp links this file and hxv_sector.cpp alone.
#include <algorithm>
#include <map>
#include <numeric>

#include "hxv_internal.hpp"
#include "hxv_tiles.hpp"

namespace hxv {

namespace {

int64_t binom64(int n, int k) {
  if (k < 0 || k > n) return 0;
  k = std::min(k, n - k);
  int64_t r = 1;
  for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;
  return r;
}

int choose_lowbits(int ns, int npart, int width, int budget_bytes, int max_block) {
  // largest number of low orbitals whose biggest block fits width x 16 B in the budget
  for (int L = ns; L >= 0; --L) {
    int64_t mx = 0;
    for (int p = 0; p <= ns - L; ++p) mx = std::max(mx, binom64(L, npart - p));
    if (mx * width * 16 <= budget_bytes && mx <= max_block) return L;
  }
  return 0;
}

struct HostTiles {
  std::vector<uint32_t> start, perm, gstart, gmax, ell_in, ell16, tstart;
  std::vector<uint32_t> bh_ptr, bh, rs_ptr, rs_off, rs_tab, rs_base, rs_neg, order, order_pc, rs16, rs16_off;
};

// sorted_out: outer table indexed by sorted position (pass A) or by natural index (pass B)
// tile_rows: rows of pass B's tile (its LDS layout decides which in-block gathers collide), 0 = pass A
void build_spin_tiles(const SpinOp& op, const std::vector<uint32_t>& map, int lowbits, int chunk, const std::vector<uint32_t>* vcol,
                      int sort_mode, bool sorted_out, int tile_rows, bool spread_banks, SpinTiles& t, HostTiles& h) {
  const int dim = op.dim;
  h.start.clear();
  if (!map.empty()) {
    uint32_t prev = 0xFFFFFFFFu;
    for (int i = 0; i < dim; ++i) {
      uint32_t hi = lowbits >= 32 ? 0u : (map[i] >> lowbits);
      if (hi != prev) {
        h.start.push_back((uint32_t)i);
        prev = hi;
      }
    }
  } else {
    for (int i = 0; i < dim; i += chunk) h.start.push_back((uint32_t)i);
  }
  h.start.push_back((uint32_t)dim);
  t.start = h.start;
  t.lowbits = lowbits;
  t.nblocks = (int)h.start.size() - 1;
  t.max_block = 0;
  std::vector<uint32_t> block_of(dim);
  for (int k = 0; k < t.nblocks; ++k) {
    t.max_block = std::max<int>(t.max_block, (int)(h.start[k + 1] - h.start[k]));
    for (uint32_t i = h.start[k]; i < h.start[k + 1]; ++i) block_of[i] = (uint32_t)k;
  }
  std::vector<int> cin(dim, 0), cout(dim, 0);
  t.n_in = t.n_out = 0;
  for (int i = 0; i < dim; ++i) {
    for (int64_t p = op.rowptr[i]; p < op.rowptr[i + 1]; ++p) (block_of[op.cols[p]] == block_of[i] ? cin[i] : cout[i])++;
    t.n_in += cin[i];
    t.n_out += cout[i];
  }
  const int kin = *std::max_element(cin.begin(), cin.end()), kout = *std::max_element(cout.begin(), cout.end());
  auto pad4 = [](int k) { return std::max(HOP_CHUNK, (k + HOP_CHUNK - 1) / HOP_CHUNK * HOP_CHUNK); };
  // one extra all-empty chunk on the natural-order outer table terminates its "all lanes empty" loop
  t.k_in = pad4(kin);
  t.k_in_real = kin;
  t.k_out = pad4(kout) + (sorted_out ? 0 : HOP_CHUNK);
  // visiting order inside each block
  h.perm.resize(dim);
  std::iota(h.perm.begin(), h.perm.end(), 0u);
  for (int k = 0; k < t.nblocks; ++k) {
    auto first = h.perm.begin() + h.start[k], last = h.perm.begin() + h.start[k + 1];
    if (sort_mode == 1)
      std::stable_sort(first, last, [&](uint32_t a, uint32_t b) { return cin[a] > cin[b]; });
    else if (sort_mode == 2)
      std::stable_sort(first, last, [&](uint32_t a, uint32_t b) { return cout[a] != cout[b] ? cout[a] > cout[b] : cin[a] > cin[b]; });
  }
  // 64-position groups and their loop bounds
  h.gstart.assign(t.nblocks + 1, 0);
  h.gmax.clear();
  double sl_in = 0, sl_out = 0;
  for (int k = 0; k < t.nblocks; ++k) {
    h.gstart[k] = (uint32_t)h.gmax.size();
    for (uint32_t a = h.start[k]; a < h.start[k + 1]; a += 64) {
      int mi = 0, mo = 0;
      const uint32_t bnd = std::min<uint32_t>(a + 64, h.start[k + 1]);
      for (uint32_t q = a; q < bnd; ++q) {
        mi = std::max(mi, cin[h.perm[q]]);
        mo = std::max(mo, cout[h.perm[q]]);
      }
      h.gmax.push_back((uint32_t)mi | ((uint32_t)mo << 16));
      sl_in += (double)(bnd - a) * ((mi + HOP_CHUNK - 1) / HOP_CHUNK * HOP_CHUNK);
      sl_out += (double)(bnd - a) * ((mo + HOP_CHUNK - 1) / HOP_CHUNK * HOP_CHUNK);
    }
  }
  h.gstart[t.nblocks] = (uint32_t)h.gmax.size();
  t.slots_in = sl_in / dim;
  t.slots_out = sl_out / dim;
  // tables
  const uint32_t emptyz = (uint32_t)(2 * op.coef.size()) << TILE_COEF_SHIFT;
  h.ell_in.assign((size_t)t.k_in * dim, emptyz);
  std::vector<uint32_t> pos_of(dim);
  for (int q = 0; q < dim; ++q) pos_of[h.perm[q]] = (uint32_t)q;
  for (int i = 0; i < dim; ++i) {
    int a = 0, b = 0, k = 0;
    const size_t qi = pos_of[i];
    for (int64_t p = op.rowptr[i]; p < op.rowptr[i + 1]; ++p, ++k) {
      const uint32_t e = op.ell[(size_t)k * dim + i];  // same order as the CSR row
      const uint32_t src = e & ELL_SRC_MASK;
      const uint32_t ci = (2u * ((e >> ELL_SRC_BITS) & ELL_COEF_MASK) + (e >> 31)) << TILE_COEF_SHIFT;
      if (block_of[src] == block_of[i])
        h.ell_in[(size_t)(a++) * dim + qi] = ci | (src - h.start[block_of[i]]);
      else
        ++b;  // out-of-block entry: handled by the structured part below
    }
  }
  // LDS bank spreading.  Slot k of a wave's 64 rows mixes different hops, so its 64 gather addresses are close to random: a
  // ds_read_b128 is served 16 lanes at a time and 16 random 16-byte bank quads collide (scripts/lds_conflicts.py: half of the
  // in-block LDS cycles are conflicts; 0.68 for uniformly random addresses).  The ORDER of a row's hops is free, so each wave's
  // lists are re-dealt slot by slot: every lane takes, among its remaining hops, the one whose bank unit is least loaded within
  // its lane group (MI355X_MICROARCH.md, LDS), for the complex-vector layouts (ds_read_b128: groups {0-3,12-15,20-27},
  // {4-11,16-19,28-31} and the same +32; 16 quads of 16 bytes; pass A lds[column*n + row] -> row & 15; pass B [column][R rows]
  // with the row position XOR-swizzled).  (real_layout: ds_read_b64, groups {0-31}, {32-63}, 32 pairs of 8 bytes -- see below.)
  auto spread = [&](std::vector<uint32_t>& tab, bool real_layout) {
    auto lane_group = [&](int l) -> int {
      if (real_layout) return l >> 5;
      const int m = l & 31;
      return ((l >> 5) << 1) | (((m >= 4 && m < 12) || (m >= 16 && m < 20) || m >= 28) ? 1 : 0);
    };
    const int units = real_layout ? 32 : 16;
    const int rows = real_layout ? 8 : tile_rows;  // (real vectors run pass B on 8-row tiles of doubles)
    int lsw = 2, rmask = 3, lr = 2;
    if (rows == 2) lsw = 3, rmask = 1, lr = 1;
    if (rows == 8) lsw = real_layout ? 2 : 1, rmask = 7, lr = 3;
    auto unit = [&](uint32_t off) -> int {
      return tile_rows == 0 ? (int)(off & (uint32_t)(units - 1)) : (int)(((off << lr) + ((off >> lsw) & (uint32_t)rmask)) & (uint32_t)(units - 1));
    };
    std::vector<std::vector<uint32_t>> rem(64);
    for (int k = 0; k < t.nblocks; ++k) {
      for (uint32_t a = h.start[k]; a < h.start[k + 1]; a += 64) {
        const int nl = (int)std::min<uint32_t>(64, h.start[k + 1] - a);
        int kmax = 0;
        for (int l = 0; l < nl; ++l) {
          rem[l].clear();
          const int cnt = cin[h.perm[a + l]];
          for (int q = 0; q < cnt; ++q) rem[l].push_back(tab[(size_t)q * dim + a + l]);
          kmax = std::max(kmax, cnt);
        }
        for (int slot = 0; slot < kmax; ++slot) {
          int load[4][32] = {{0}};
          uint32_t seen[4][32][4];  // distinct addresses already on a unit (identical ones broadcast): the first few are enough
          for (int l = 0; l < nl; ++l) {
            if (rem[l].empty()) continue;
            const int g = lane_group(l);
            size_t best = 0;
            int best_load = 1 << 30;
            for (size_t j = 0; j < rem[l].size(); ++j) {
              const uint32_t off = rem[l][j] & TILE_OFF_MASK;
              const int qd = unit(off);
              int ld = load[g][qd];
              for (int u = 0; u < std::min(ld, 4); ++u)
                if (seen[g][qd][u] == off) {
                  ld = -1;  // the same address is already being read: a broadcast, free
                  break;
                }
              if (ld < best_load) best_load = ld, best = j;
            }
            const uint32_t w = rem[l][best];
            rem[l].erase(rem[l].begin() + (long)best);
            tab[(size_t)slot * dim + a + l] = w;
            const uint32_t off = w & TILE_OFF_MASK;
            const int qd = unit(off);
            if (best_load >= 0) {
              if (load[g][qd] < 4) seen[g][qd][load[g][qd]] = off;
              ++load[g][qd];
            }
          }
        }
      }
    }
  };
  // (A second deal for the real-vector layouts was built and measured: no gain on the real-vector Lanczos iteration, 4.005 against
  //  4.007 ms at C3, and it costs the bit-for-bit agreement of the real product with the real part of the complex one.  One table.)
  if (spread_banks) spread(h.ell_in, false);
  // Half-size copy of the in-block table: two hops per word, each (coefficient index << p16_bits) | offset, whenever the
  // block offsets and the signed-coefficient indices fit 16 bits together (C3: 10 + 3 bits; blocks of 14 low orbitals: 12 + 3).
  // Half the table bytes to keep in L2 and half the loads; the 32-bit table stays for the job kernel, which packs its words once per job.
  h.ell16.clear();
  t.p16_bits = 0;
  {
    int ob = 1, cb = 1;
    while ((1 << ob) < t.max_block) ++ob;
    while ((1u << cb) < 2 * op.coef.size() + 1) ++cb;
    if (ob + cb <= 16 && t.k_in % 2 == 0) {
      t.p16_bits = std::max(ob, 10);  // (10 when it fits: the split the kernels were tuned with)
      if (t.p16_bits + cb > 16) t.p16_bits = ob;
      const uint32_t om = (1u << t.p16_bits) - 1u;
      auto pack = [&](const std::vector<uint32_t>& src, std::vector<uint32_t>& dst) {
        dst.assign((size_t)(t.k_in / 2) * dim, 0u);
        for (int a = 0; a < t.k_in; ++a)
          for (int q = 0; q < dim; ++q) {
            const uint32_t e = src[(size_t)a * dim + q];
            const uint32_t half = ((e >> TILE_COEF_SHIFT) << t.p16_bits) | (e & om);
            dst[(size_t)(a / 2) * dim + q] |= half << (16 * (a & 1));
          }
      };
      pack(h.ell_in, h.ell16);
    }
  }
  // Blocks whose high orbitals hold the same NUMBER of particles contain the same low-orbital patterns, and hops among the
  // low orbitals see nothing else: their in-block tables (words, visiting order, loop bounds) are identical.  Every block
  // reads the tables of the first block that equals it (compared, not assumed), so the hot table set shrinks from one
  // slice per block to one per class (C3: 5 instead of 16) and stays in L2 between the workgroups that use it.
  h.tstart.assign(t.nblocks, 0);
  t.table_classes = 0;
  for (int k = 0; k < t.nblocks; ++k) {
    h.tstart[k] = h.start[k];
    const uint32_t nk = h.start[k + 1] - h.start[k];
    bool found = false;
    for (int c = 0; c < k && !found; ++c) {
      if (h.tstart[c] != h.start[c] || h.start[c + 1] - h.start[c] != nk) continue;  // (only first-of-class blocks are candidates)
      bool same = true;
      for (uint32_t q = 0; q < nk && same; ++q) same = h.perm[h.start[k] + q] - h.start[k] == h.perm[h.start[c] + q] - h.start[c];
      const uint32_t ng = (nk + 63) / 64;
      for (uint32_t q = 0; q < ng && same; ++q) same = (h.gmax[h.gstart[k] + q] & 0xFFFFu) == (h.gmax[h.gstart[c] + q] & 0xFFFFu);  // (the kernels read the in-block bound only)
      for (int a = 0; a < t.k_in && same; ++a)
        same = std::equal(h.ell_in.begin() + (size_t)a * dim + h.start[k], h.ell_in.begin() + (size_t)a * dim + h.start[k] + nk,
                          h.ell_in.begin() + (size_t)a * dim + h.start[c]);
      if (same) {
        h.tstart[k] = h.start[c];
        h.gstart[k] = h.gstart[c];
        found = true;
      }
    }
    if (!found) ++t.table_classes;
  }
  // ---- structured out-of-block part: group by (block, source block)
  h.bh_ptr.assign(t.nblocks + 1, 0);
  h.rs_ptr.assign(t.nblocks + 1, 0);
  h.bh.clear();
  h.rs_off.clear();
  h.rs_tab.clear();
  h.rs_base.clear();
  h.rs_neg.clear();
  double bh_rows = 0, rs_rows = 0;
  struct Ent {
    uint32_t off, src, ci;
  };
  std::vector<std::vector<Ent>> by_src(t.nblocks);
  std::vector<int> touched;
  for (int k = 0; k < t.nblocks; ++k) {
    const uint32_t b0 = h.start[k], nb = h.start[k + 1] - b0;
    touched.clear();
    for (uint32_t i = b0; i < b0 + nb; ++i) {
      int kk = 0;
      for (int64_t p = op.rowptr[i]; p < op.rowptr[i + 1]; ++p, ++kk) {
        const uint32_t e = op.ell[(size_t)kk * dim + i];
        const uint32_t src = e & ELL_SRC_MASK;
        const uint32_t sb = block_of[src];
        if ((int)sb == k) continue;
        if (by_src[sb].empty()) touched.push_back((int)sb);
        by_src[sb].push_back({i - b0, src, 2u * ((e >> ELL_SRC_BITS) & ELL_COEF_MASK) + (e >> 31)});
      }
    }
    std::sort(touched.begin(), touched.end());
    h.bh_ptr[k] = (uint32_t)(h.bh.size() / 2);
    h.rs_ptr[k] = (uint32_t)h.rs_off.size();
    for (int sb : touched) {
      auto& ents = by_src[sb];
      const uint32_t s0 = h.start[sb], ns = h.start[sb + 1] - s0;
      bool uniform = ents.size() == nb && ns == nb;
      if (uniform)
        for (const Ent& en : ents)
          if (en.src - s0 != en.off || en.ci != ents[0].ci) {
            uniform = false;
            break;
          }
      // the source run must also be contiguous in the (possibly padded) gather layout
      if (uniform && vcol)
        for (uint32_t q = 0; q < ns; ++q)
          if ((*vcol)[s0 + q] != (*vcol)[s0] + q) {
            uniform = false;
            break;
          }
      if (uniform) {
        h.bh.push_back(vcol ? (*vcol)[s0] : s0);
        h.bh.push_back(ents[0].ci);
        bh_rows += nb;
      } else {
        // as many slots as the busiest row has entries from this source block
        std::vector<int> mult(nb, 0);
        int nsl = 0;
        for (const Ent& en : ents) nsl = std::max(nsl, ++mult[en.off]);
        // Table words hold the source RELATIVE to its block when the block's slots are contiguous in the gather layout
        // (always on an unsplit sector); the slot's base is a per-slot constant.  Relative tables repeat between blocks of
        // the same class up to one overall sign, and are shared below.
        bool contig = true;
        if (vcol)
          for (uint32_t q = 0; q < ns && contig; ++q) contig = (*vcol)[s0 + q] == (*vcol)[s0] + q;
        const size_t base = h.rs_tab.size();
        h.rs_tab.resize(base + (size_t)nsl * nb, emptyz);
        std::fill(mult.begin(), mult.end(), 0);
        for (const Ent& en : ents) {
          const int sl = mult[en.off]++;
          const uint32_t where = contig ? en.src - s0 : (vcol ? (*vcol)[en.src] : en.src);
          h.rs_tab[base + (size_t)sl * nb + en.off] = (en.ci << TILE_COEF_SHIFT) | where;
        }
        for (int sl = 0; sl < nsl; ++sl) {
          h.rs_off.push_back((uint32_t)(base + (size_t)sl * nb));
          h.rs_base.push_back(contig ? (vcol ? (*vcol)[s0] : s0) : 0u);
          h.rs_neg.push_back(0u);
        }
        rs_rows += (double)nsl * nb;
      }
      ents.clear();
    }
  }
  h.bh_ptr[t.nblocks] = (uint32_t)(h.bh.size() / 2);
  h.rs_ptr[t.nblocks] = (uint32_t)h.rs_off.size();
  // share row-slot tables that are equal up to an overall sign (a coefficient index is 2*amplitude + sign): a slot reads
  // the first table that equals its own after normalising the sign of its first entry, and negates if it had to flip
  {
    std::map<std::vector<uint32_t>, uint32_t> seen;  // normalised table -> offset of its first copy
    t.rs_tables = 0;
    for (int k = 0; k < t.nblocks; ++k) {
      const uint32_t nb = h.start[k + 1] - h.start[k];
      for (uint32_t sl = h.rs_ptr[k]; sl < h.rs_ptr[k + 1]; ++sl) {
        std::vector<uint32_t> tab(h.rs_tab.begin() + h.rs_off[sl], h.rs_tab.begin() + h.rs_off[sl] + nb);
        uint32_t flip = 0;
        for (uint32_t w : tab)
          if (w != emptyz) {
            flip = (w >> TILE_COEF_SHIFT) & 1u;
            break;
          }
        if (flip)
          for (uint32_t& w : tab)
            if (w != emptyz) w ^= 1u << TILE_COEF_SHIFT;
        auto it = seen.find(tab);
        if (it == seen.end()) {
          std::copy(tab.begin(), tab.end(), h.rs_tab.begin() + h.rs_off[sl]);  // stored normalised
          seen.emplace(std::move(tab), h.rs_off[sl]);
          ++t.rs_tables;
        } else {
          h.rs_off[sl] = it->second;
        }
        h.rs_neg[sl] = flip;
      }
    }
  }
  // Half-size row-slot tables, two slots of a block per 32-bit word ((coefficient index << p16_bits) | source offset relative to
  // the slot's block, the split of the half-size in-block table): half the table loads and bytes of the out-of-block phases.
  // Needs block-relative words (contiguous gather slots: always on an unsplit sector).  Pairs are shared like the single tables.
  h.rs16.clear();
  h.rs16_off.assign(h.rs_off.size(), 0u);
  if (t.p16_bits > 0 && !h.rs_off.empty()) {
    bool ok = true;
    // (absolute words appear only with non-contiguous gather slots: their offsets do not fit the field)
    const uint32_t om = (1u << t.p16_bits) - 1u;
    for (int k = 0; k < t.nblocks && ok; ++k) {
      const uint32_t nb = h.start[k + 1] - h.start[k];
      for (uint32_t sl = h.rs_ptr[k]; sl < h.rs_ptr[k + 1] && ok; ++sl)
        for (uint32_t q = 0; q < nb && ok; ++q) ok = (h.rs_tab[h.rs_off[sl] + q] & TILE_OFF_MASK) <= om;
    }
    if (ok) {
      std::map<std::pair<uint32_t, uint32_t>, uint32_t> seen;  // (table of the first slot, table of the second slot or ~0) -> packed offset
      const uint32_t e16 = (uint32_t)(2 * op.coef.size()) << t.p16_bits;  // empty slot: (offset 0, zero coefficient)
      for (int k = 0; k < t.nblocks; ++k) {
        const uint32_t nb = h.start[k + 1] - h.start[k];
        for (uint32_t sl = h.rs_ptr[k]; sl < h.rs_ptr[k + 1]; sl += 2) {
          const bool two = sl + 1 < h.rs_ptr[k + 1];
          const auto key = std::make_pair(h.rs_off[sl], two ? h.rs_off[sl + 1] : 0xFFFFFFFFu);
          auto it = seen.find(key);
          if (it == seen.end()) {
            const uint32_t base = (uint32_t)h.rs16.size();
            h.rs16.resize(base + nb);
            for (uint32_t q = 0; q < nb; ++q) {
              const uint32_t a = h.rs_tab[h.rs_off[sl] + q];
              const uint32_t lo = ((a >> TILE_COEF_SHIFT) << t.p16_bits) | (a & om);
              uint32_t hi = e16;
              if (two) {
                const uint32_t bb = h.rs_tab[h.rs_off[sl + 1] + q];
                hi = ((bb >> TILE_COEF_SHIFT) << t.p16_bits) | (bb & om);
              }
              h.rs16[base + q] = lo | (hi << 16);
            }
            it = seen.emplace(key, base).first;
          }
          h.rs16_off[sl] = it->second;
        }
      }
    }
  }
  t.rs16_on = !h.rs16.empty();
  if (h.rs16.empty()) h.rs16.assign(1, 0u);
  if (h.rs16_off.empty()) h.rs16_off.assign(1, 0u);
  if (h.bh.empty()) h.bh.assign(2, 0);
  if (h.rs_off.empty()) {
    h.rs_off.assign(1, 0);
    h.rs_base.assign(1, 0);
    h.rs_neg.assign(1, 0);
  }
  if (h.rs_tab.empty()) h.rs_tab.assign(1, emptyz);
  t.bh_per_row = bh_rows / dim;
  t.rs_per_row = rs_rows / dim;
  t.max_outer = 0;
  for (int k = 0; k < t.nblocks; ++k) {
    t.max_outer = std::max<int>(t.max_outer, (int)(h.bh_ptr[k + 1] - h.bh_ptr[k]) + (int)(h.rs_ptr[k + 1] - h.rs_ptr[k]));
  }
  h.order.resize(t.nblocks);
  std::iota(h.order.begin(), h.order.end(), 0u);
  std::stable_sort(h.order.begin(), h.order.end(),
                   [&](uint32_t a, uint32_t b) { return h.start[a + 1] - h.start[a] > h.start[b + 1] - h.start[b]; });
  // Dispatch order of the tile kernels for LARGE sectors (TileOptions::block_order): blocks by the particle number of their high
  // orbitals, natural order inside.  Two blocks are coupled when their high patterns differ by one hop among the high orbitals (same
  // particle number) or by one particle (a hop between a low and a high orbital): sorting the patterns of a hypercube by weight, then by
  // value, is the order that keeps every such pair closest (Harper), and blocks of one weight share their in-block tables anyway.
  h.order_pc.resize(t.nblocks);
  std::iota(h.order_pc.begin(), h.order_pc.end(), 0u);
  if (!map.empty() && lowbits < 32)
    std::stable_sort(h.order_pc.begin(), h.order_pc.end(), [&](uint32_t a, uint32_t b) {
      return __builtin_popcount(map[h.start[a]] >> lowbits) < __builtin_popcount(map[h.start[b]] >> lowbits);
    });
}

std::vector<double2> signed_coefs(const SpinOp& op) {
  std::vector<double2> sc(2 * op.coef.size() + 1);
  for (size_t i = 0; i < op.coef.size(); ++i) {
    sc[2 * i] = make_double2(op.coef[i].real(), op.coef[i].imag());
    sc[2 * i + 1] = make_double2(-op.coef[i].real(), -op.coef[i].imag());
  }
  sc.back() = make_double2(0.0, 0.0);
  return sc;
}

}  // namespace

// the block bits pass A gets from the DEFAULT options (what make_tile_plan's `build` computes for the up spin): the device row order of a
// sector is chosen for them once, when the sector is built, and does not follow later option changes (device vectors outlive those)
int default_lowbits_up(int ns, int npart, int ncoef) {
  const TileOptions o;
  const int budget = o.lds_budget_kb_up * 1024 - 16 * (2 * ncoef + 1);
  return o.force_bits_up >= 0 ? std::min(o.force_bits_up, ns) : choose_lowbits(ns, npart, o.cols_per_tile, budget, o.threads_up);
}

std::string make_tile_plan(const SectorHost& s, TilePlan& plan, const PlanUploader& up) {
  TileOptions& o = plan.opt;
  if (o.cols_per_tile != 2 && o.cols_per_tile != 4 && o.cols_per_tile != 8) return "cols_per_tile must be 2, 4 or 8";
  // Large sectors (Ns=18): two neighbouring 4-row panels of DimDw columns are 128 B x DimDw = 6 MB of lines, more than an XCD's
  // L2, and nearly every out-of-block gather of pass B then leaves the XCD: eight rows per tile (whole lines; smaller blocks
  // to stay within the LDS budget) measured 40.8 ms against 47.4 ms per pass B there (Ns=16: 2.25 against 2.22 ms).
  if (o.rows_per_tile == 0) o.rows_per_tile = (int64_t)128 * s.dimdw > ((int64_t)4 << 20) ? 8 : 4;
  if (o.rows_per_tile != 2 && o.rows_per_tile != 4 && o.rows_per_tile != 8) return "rows_per_tile must be 0 (automatic), 2, 4 or 8";
  if (o.lds_budget_kb_up < 8 || o.lds_budget_kb_up > 144 || o.lds_budget_kb_dw < 8 || o.lds_budget_kb_dw > 144)
    return "lds_budget_kb must be in [8,144]";
  for (int th : {o.threads_up, o.threads_dw})
    if (th != 256 && th != 512 && th != 1024) return "threads must be 256, 512 or 1024";
  if (o.sort_mode < 0 || o.sort_mode > 2) return "sort_mode must be 0, 1 or 2";
  if (o.wt_cols != 2 && o.wt_cols != 4 && o.wt_cols != 8 && o.wt_cols != 16) return "wt_cols must be 2, 4, 8 or 16";
  if (o.job_cols != 1 && o.job_cols != 2) return "job_cols must be 1 or 2";
  if (o.job_groups < 1 || o.job_groups > 65536) return "job_groups must be in [1,65536]";
  if (o.job_stages < 2 || o.job_stages > 8) return "job_stages must be in [2,8]";
  plan.ncoef_up = (int)s.dev_up().coef.size();
  plan.ncoef_dw = (int)s.dw.coef.size();
  plan.usable = plan.ncoef_up <= TILE_MAX_COEF && plan.ncoef_dw <= TILE_MAX_COEF;
  if (!plan.usable) return "";
  // the two spins' tables are independent: built on one host thread each, handed to the uploader afterwards (it is not re-entrant)
  HostTiles hu, hd;
  auto build = [&](const SpinOp& op, const std::vector<uint32_t>& map, int npart, int width, int force, int budget_kb, int max_block,
                   const std::vector<uint32_t>* vcol, bool sorted_out, int sort_mode, SpinTiles& t, HostTiles& h) -> std::string {
    const int tile_rows = sorted_out ? 0 : width;
    const int budget = budget_kb * 1024 - 16 * (2 * (int)op.coef.size() + 1);
    int L = 32, chunk = std::max(1, std::min(budget / (16 * width), max_block));
    if (!map.empty()) L = force >= 0 ? std::min(force, s.ns) : choose_lowbits(s.ns, npart, width, budget, max_block);
    build_spin_tiles(op, map, L, chunk, vcol, sort_mode, sorted_out, tile_rows, o.spread_banks != 0, t, h);
    if ((int64_t)t.max_block * width * 16 + 16 * (2 * (int64_t)op.coef.size() + 1) > 160 * 1024) return "tile does not fit the 160 KB LDS";
    if (t.max_block > max_block) return "block larger than the workgroup (one thread per block row/column)";
    return "";
  };
  auto send = [&](HostTiles& h, SpinTiles& t) -> std::string {
    if (up.u32(h.start, &t.d_start) != hipSuccess || up.u32(h.perm, &t.d_perm) != hipSuccess ||
        up.u32(h.gstart, &t.d_gstart) != hipSuccess || up.u32(h.gmax, &t.d_gmax) != hipSuccess ||
        up.u32(h.ell_in, &t.d_ell_in) != hipSuccess || up.u32(h.tstart, &t.d_tstart) != hipSuccess ||
        (!h.ell16.empty() && up.u32(h.ell16, &t.d_ell16) != hipSuccess) ||
        up.u32(h.bh_ptr, &t.d_bh_ptr) != hipSuccess || up.u32(h.bh, &t.d_bh) != hipSuccess ||
        up.u32(h.rs_ptr, &t.d_rs_ptr) != hipSuccess || up.u32(h.rs_off, &t.d_rs_off) != hipSuccess ||
        up.u32(h.rs_tab, &t.d_rs_tab) != hipSuccess || up.u32(h.order, &t.d_order) != hipSuccess || up.u32(h.order_pc, &t.d_order_pc) != hipSuccess ||
        up.u32(h.rs_base, &t.d_rs_base) != hipSuccess || up.u32(h.rs_neg, &t.d_rs_neg) != hipSuccess ||
        up.u32(h.rs16, &t.d_rs16) != hipSuccess || up.u32(h.rs16_off, &t.d_rs16_off) != hipSuccess)
      return "upload of tile tables failed";
    return "";
  };
  static const std::vector<uint32_t> no_map;  // panel handles have no up basis: plain index chunks (pass A never runs)
  std::string e_up, e;
  GuardedThread th;   // (an exception on either side comes back as an error string; the thread is joined on every path -- ADVICE r5)
  th.run([&] {
    e_up = build(s.dev_up(), s.panel_rows > 0 ? no_map : s.dev_key_up(), s.nup, o.cols_per_tile, o.force_bits_up, o.lds_budget_kb_up, o.threads_up, nullptr, true, 0,
                 plan.up, hu);
  });
  // pass B sorts by the inner count only: its outer table is read in natural column order
  try {
    e = build(s.dw, s.map_dw, s.ndw, o.rows_per_tile, o.force_bits_dw, o.lds_budget_kb_dw, o.threads_dw, &s.vcol, false, o.sort_mode_dw ? 1 : 0, plan.dw,
              hd);
  } catch (const std::exception& ex) {
    e = std::string("tile plan of H_dw: ") + ex.what();
  }
  th.join();
  if (!th.err.empty()) return "tile plan of H_up: " + th.err;
  if (!e_up.empty()) return e_up;
  if (!e.empty()) return e;
  e = send(hu, plan.up);
  if (!e.empty()) return e;
  e = send(hd, plan.dw);
  if (!e.empty()) return e;
  if (up.d2(signed_coefs(s.dev_up()), &plan.d_scoef_up) != hipSuccess || up.d2(signed_coefs(s.dw), &plan.d_scoef_dw) != hipSuccess)
    return "upload of coefficient tables failed";
  return "";
}

int64_t tiled_wt_elems(const DevSector& s, const TilePlan& plan) {
  const int wc = std::max(plan.opt.cols_per_tile, plan.opt.wt_cols);
  return (int64_t)((s.qdw + wc - 1) / wc) * wc * ((s.dimup + 15) & ~15);  // (whole patches of up to 8 complex / 16 real rows per group)
}

bool job_up_usable(const DevSector& s, const TilePlan& plan) {
  const SpinTiles& u = plan.up;
  return plan.usable && s.diag.mode == 0 && u.max_block <= 64 * JOB_LOADER && u.k_in <= JOB_KIN && u.max_outer <= JOB_KO &&
         u.d_order != nullptr && s.dimup < 65536 &&  // (packed out-of-block words: hxv_up_job)
         u.nblocks <= plan.opt.job_max_blocks && plan.opt.job_cols == 1;
}

void job_up_geometry(const DevSector& s, const TilePlan& plan, bool lz_xm, int wc, JobUp& jb, int& lds_bytes, int64_t& nwg) {
  const int C = plan.opt.job_cols;
  jb.ngroups = (s.qdw + C - 1) / C;
  jb.gpx = (jb.ngroups + 7) / 8;
  jb.gc = std::max(1, plan.opt.job_groups);
  jb.chunks = std::max(1, (jb.gpx + jb.gc / 2) / jb.gc);  // about job_groups groups per job, all jobs of an XCD equally long
  jb.ns = (plan.up.max_block + 63) & ~63;
  jb.stage_bytes = (1 + (lz_xm ? 1 : 0)) * C * jb.ns * 16;
  jb.wt_bytes = jb.ns * std::max(wc, 1) * 16;
  const int tab = (((2 * plan.ncoef_up + 1) * 16 + 255) & ~255) + 256;  // coefficients, loader bookkeeping words
  jb.nst = std::min(std::min(plan.opt.job_stages, JOB_MAX_STAGES), (160 * 1024 - tab - 2 * jb.wt_bytes) / jb.stage_bytes);
  lds_bytes = jb.nst * jb.stage_bytes + 2 * jb.wt_bytes + tab;
  jb.kin_rows = std::min(plan.up.k_in, (plan.up.k_in_real + 3) & ~3);
  jb.max_outer = plan.up.max_outer;
  jb.debug = plan.opt.job_debug;
  jb.order = plan.up.d_order;
  nwg = (int64_t)8 * jb.chunks * plan.up.nblocks;
}

int64_t job_up_workgroups(const DevSector& s, const TilePlan& plan) {
  JobUp jb{};
  int lds = 0;
  int64_t nwg = 0;
  job_up_geometry(s, plan, false, 0, jb, lds, nwg);
  return nwg;
}

bool job_up_fits(const DevSector& s, const TilePlan& plan, bool lz, int wc) {
  // (the Lanczos epilogue streams the previous vector's tile as well: decided for the worst case so that the choice of
  //  kernel -- and the number of per-workgroup partial sums -- does not change from one iteration to the next)
  if (wc > 0 && wc % plan.opt.job_cols != 0) return false;
  JobUp jb{};
  int lds = 0;
  int64_t nwg = 0;
  job_up_geometry(s, plan, lz, wc, jb, lds, nwg);
  return jb.nst >= 2;
}

// Real-vector mode runs the same plans with twice the columns (pass A) / rows (pass B) per tile: the same tile bytes.
int real_cols(const TilePlan& plan) { return std::min(8, 2 * plan.opt.cols_per_tile); }
// Complex vectors: at most four columns per pass-A tile.  The eight-column kernels need far more than the 64 registers two
// workgroups per CU leave (they spill 30 - 140 of them, scalar registers as well), were 35 % slower when they were measured, and
// one of them (complex H, Lanczos epilogue) came out of hipcc computing wrong sums after an unrelated two-pointer growth of
// the kernel arguments: "cols_per_tile" = 8 keeps its meaning for the plan (block size) and for real vectors only.
int cplx_cols(const TilePlan& plan) { return std::min(4, plan.opt.cols_per_tile); }
int real_rows(const TilePlan& plan) { return std::min(8, 2 * plan.opt.rows_per_tile); }
int real_wc(const TilePlan& plan) { return std::max(real_cols(plan), std::min(16, 2 * plan.opt.wt_cols)); }

// The plan's own part of that decision, for scratch groups of wc columns (option "job_up_active" reports it for job_up = 1, a plain
// product and the configured width)
bool job_up_planned(const DevSector& s, const TilePlan& plan, bool lz, int wc) {
  return plan.opt.sort_mode == 0 && job_up_usable(s, plan) && job_up_fits(s, plan, lz, wc);
}

// Pass A runs as jobs (hxv_jobs.hip) when the plan allows it and the tile ring fits the LDS; wc_out = scratch group width.
bool use_job_up(const DevSector& s, const TilePlan& plan, bool real_vec, bool lz, bool wt_natural, int* wc_out) {
  if (real_vec || !plan.opt.job_up || plan.opt.debug != 0) return false;
  if (s.nd.active) return false;  // (the spH0nd block rides on the one-tile-per-workgroup kernel only)
  // job_up = 2 (default): jobs for the fused Lanczos product only.  With the in-block tables shared between blocks of a class
  // the one-tile-per-workgroup kernel is 2 % faster for the plain product (2.22 against 2.27 ms at C3), the job kernel 2.5 %
  // faster with the Lanczos epilogue, whose second input vector it streams through the tile ring (6.29 against 6.45 ms).
  if (plan.opt.job_up == 2 && !lz) return false;
  int wc = wt_natural ? 0 : std::max(plan.opt.job_cols, plan.opt.wt_cols);
  if (!job_up_planned(s, plan, lz, wc)) {
    // the Lanczos epilogue streams a third vector through the tile ring: narrower scratch groups (two buffers of
    // wc columns each sit beside the ring) can make room for it
    if (wt_natural || wc <= 2 || plan.opt.job_cols > 2 || !job_up_planned(s, plan, lz, 2)) return false;
    wc = 2;
  }
  if (wc_out) *wc_out = wc;
  return true;
}

int64_t tiled_pass_up_workgroups(const DevSector& s, const TilePlan& plan, bool real_vec, bool pieces) {
  // (both epilogues run on the same kernel: jobs where they apply, else one tile per workgroup; a dw part handed over in pieces --
  //  exchange mode 2 -- always goes through the tile kernel)
  if (!pieces && use_job_up(s, plan, real_vec, true, false)) return job_up_workgroups(s, plan);
  const int C = real_vec ? real_cols(plan) : cplx_cols(plan);
  const int ngroups = (s.qdw + C - 1) / C;
  return (int64_t)((ngroups + 7) / 8) * 8 * plan.up.nblocks;
}

}  // namespace hxv
