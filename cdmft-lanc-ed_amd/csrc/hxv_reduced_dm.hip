// Reduced density matrix of a subset S of the impurity orbitals of a device-resident state (include/hxv.h: hxv_reduced_dm_accumulate).
//
// rho_S = Tr_env |psi><psi|, env = every orbital outside S (the bath and the traced impurity orbitals); the reference's
// ed_get_reduced_density_matrix_single (ED_IO/get_reduced_dm.f90:68-212) without the dense cluster_density_matrix it traces, so without a limit on
// Nimp.  A spin configuration m splits into a = the bits of S (compressed, ascending orbital order) and e = m & ~S; the rows of one e are a
// GROUP of dU = C(Nred, nup - |e|) rows -- no run of the reference's order any more, the group tables name every row -- and rho_S is a sum of
// Hermitian rank-1 updates x x^+, one per pair (e_up, e_dw).  The pairs fall into CLASSES (|e_up|, |e_dw|), each with one dU*dD x dU*dD block.
//   fermi_sign 0: the plain partial trace.  This is what the reference computes: its get_sign (:170-191) depends on the traced bits alone, which
//                 the two states of a contributing pair share (:145), so its sign product is +1 throughout.
//   fermi_sign 1: every basis state carries (-1)^n, n = sum over the occupied r in S of the occupied orbitals outside S below r: the
//                 Jordan-Wigner string of moving the operators of S in front of the others.  It is a factor per row times a factor per column,
//                 folded into the sign bit of the table entries.
// Kernels:
//   rdm_pair_kernel    classes with n = dU*dD <= 4 (every class of a one- or two-orbital mask): one thread per pair, its at most four amplitudes
//                      loaded straight from the vector (16 bytes each) and the upper triangle of x x^+ kept in registers; consecutive threads take
//                      consecutive up groups of one dw group, and the up groups of a class are listed by their lowest device row.  The workgroup
//                      sums its threads in a fixed order (xor butterfly inside a wave, then wave 0..3) and writes one partial block.
//   rdm_tile_kernel    the other classes (n <= 36): the table-driven register-tile scheme of cdm_accumulate_kernel (hxv_cluster_dm.hip) with
//                      2 x 2 tiles, a batch of pairs staged through LDS, columns signed as well as rows.
//   rdm_reduce_kernel  one thread per class-block element: the partials of its class, summed in list order.
// No floating-point atomics: the same vector on the same handle gives the same bits on every call.  The tables are built on the host in
// device-row numbering and cached with the sector image by (mask, fermi_sign).  On a split sector a dw group belongs to the rank that owns its
// lowest column and reads the gathered copy; the class blocks are all-reduced.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "hxv_handle.hpp"

using namespace hxv;

namespace {
constexpr int RDM_THREADS = 256;
constexpr int RDM_XS = 2048;       // LDS staging area of the tile kernel, amplitudes (32 KB)
constexpr int RDM_PAIR_COST = 36;  // work-list balance of the tile kernel: a pair costs one trip of its wave's register loop however small its block
constexpr int RDM_LOADS = 4;       // 16-byte loads a thread has in flight while staging
constexpr int RDM_MAX_NRED = 4;    // 256 x 256, blocks up to 36 x 36
constexpr int RDM_SMALL_N = 4;     // classes up to this block size take the pair kernel
constexpr int RDM_WG_PER_CU = 4;   // work items per compute unit the list is cut for
constexpr size_t RDM_CACHE = 8;    // tables kept per sector image: the masks of one solve (sites, pairs of sites), both conventions

struct RdmClass {
  int32_t du, dd, n;      // block shape: n = du*dd
  int32_t nt, ntiles;     // 2 x 2 tiles per side, tiles of the upper triangle
  int32_t batch, stride;  // tile kernel: pairs staged at once; LDS elements between the dw components of the staged amplitudes
  int32_t ngu;            // up groups of the class
  int32_t rows_off;       // into rows: [ngu][du] device row | sign << 31
  int32_t cols_off;       // into cols: [local dw groups][dd] column slot | sign << 31
  int32_t tile_off;       // into tiles: ti | tj << 16
  int32_t nrep;           // partial blocks an item writes: 4 (tile kernel, the block's tiles fit one wave: one per wave) or 1
};
struct RdmItem {
  int32_t cls, p0, p1, pad;  // pairs [p0, p1) of the class, pair = (local dw group) * ngu + (up group)
  int64_t out_off;           // its partial block(s) in the partial buffer (elements)
};
struct RdmClassHost {
  int64_t out_off = 0;           // the class block in the reduced output (elements), ntiles*4 of them
  std::vector<uint32_t> au, ad;  // compressed S configurations of the block's up / dw components
  std::vector<uint32_t> tiles;
};
}  // namespace

namespace hxv {
struct SectorImage::RdmTables {
  int nred = 0;
  std::vector<RdmClass> cls;
  std::vector<RdmClassHost> hcls;
  int nitems[2] = {0, 0};  // items of the pair kernel, then of the tile kernel
  int64_t partial_elems = 0, out_elems = 0;
  RdmClass* d_cls = nullptr;
  RdmItem* d_items = nullptr;
  uint32_t *d_rows = nullptr, *d_cols = nullptr, *d_tiles = nullptr;
  int32_t *d_el_cnt = nullptr, *d_el_stride = nullptr;
  int64_t* d_el_src = nullptr;
  void* base = nullptr;
  int device = -1;
  int64_t bytes = 0;
  ~RdmTables() {
    if (!base) return;
    int cur = -1;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(device);
    (void)hipFree(base);
    if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
  }
};
}  // namespace hxv

namespace {
using RdmTables = SectorImage::RdmTables;

int64_t binom(int n, int k) {
  if (k < 0 || k > n) return 0;
  int64_t r = 1;
  for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;
  return r;
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

// small_n: RDM_SMALL_N, or 0 to send every class to the tile kernel (the A/B hook HXV_RDM_PAIR_KERNEL=0 of scripts/reduced_dm_bench.py)
std::string build_tables(const SectorHost& s, uint32_t S, int fermi, int small_n, int device, int ncu, RdmTables& t) {
  const int nred = __builtin_popcount(S);
  t.nred = nred;
  t.device = device;
  const bool ro = s.row_order();
  const int kmax = s.ns - nred;  // env particle numbers 0 .. kmax
  // owner of a dw column / its slot in the gathered copy (the padded all-gather layout)
  std::vector<int32_t> rfirst(s.nranks + 1, 0);
  for (int p = 0; p < s.nranks; ++p) {
    int q, c0;
    dw_split(s.dimdw, p, s.nranks, q, c0);
    rfirst[p] = c0;
  }
  rfirst[s.nranks] = s.dimdw;
  auto slot_of = [&](int c) -> uint32_t {
    if (s.nranks == 1) return (uint32_t)c;
    const int o = (int)(std::upper_bound(rfirst.begin(), rfirst.end(), c) - rfirst.begin()) - 1;
    return (uint32_t)(o * s.cmax + (c - rfirst[o]));
  };
  // per env particle number: the up groups' rows (groups by their lowest device row), this rank's dw groups' columns (by lowest column)
  std::vector<std::vector<uint32_t>> urows(kmax + 1), dcols(kmax + 1);
  std::vector<int32_t> ungrp(kmax + 1, 0), dngrp(kmax + 1, 0), dngrp_all(kmax + 1, 0);
  {
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
        const uint32_t r = (uint32_t)(ro ? s.up_perm[i] : i);
        const uint32_t sg = ((ro && s.up_sign[r]) ? 1u : 0u) ^ (fermi ? fermi_bit(s.map_up[i], S) : 0u);
        kd.e.push_back(r | (sg << 31));
        kd.first = std::min(kd.first, r);
      }
      byk[k].push_back(std::move(kd));
    }
    for (int k = 0; k <= kmax; ++k) {
      std::sort(byk[k].begin(), byk[k].end(), [](const Keyed& a, const Keyed& b) { return a.first < b.first; });
      for (const Keyed& kd : byk[k]) urows[k].insert(urows[k].end(), kd.e.begin(), kd.e.end());
      ungrp[k] = (int32_t)byk[k].size();
    }
  }
  {
    std::vector<Group> dg = env_groups(s.map_dw, S);
    std::sort(dg.begin(), dg.end(), [](const Group& a, const Group& b) { return a.idx[0] < b.idx[0]; });
    for (const Group& g : dg) {
      const int k = __builtin_popcount(g.env);
      if (k > kmax || (int64_t)g.idx.size() != binom(nred, s.ndw - k)) return "reduced density matrix: the dw basis does not hold every configuration of the subset";
      ++dngrp_all[k];
      if (g.idx[0] < s.dw0 || g.idx[0] >= s.dw0 + s.qdw) continue;  // the rank that owns the lowest column takes the group
      for (int32_t c : g.idx) dcols[k].push_back(slot_of(c) | ((fermi ? fermi_bit(s.map_dw[c], S) : 0u) << 31));
      ++dngrp[k];
    }
  }
  std::vector<uint32_t> rows, cols, tiles;
  std::vector<int32_t> rows_off(kmax + 1, 0), cols_off(kmax + 1, 0);
  for (int k = 0; k <= kmax; ++k) {
    rows_off[k] = (int32_t)rows.size();
    rows.insert(rows.end(), urows[k].begin(), urows[k].end());
    cols_off[k] = (int32_t)cols.size();
    cols.insert(cols.end(), dcols[k].begin(), dcols[k].end());
  }
  // classes: every (up, dw) env particle number pair of the WHOLE sector, the same list on every rank; the pair kernel's classes first
  std::vector<int32_t> cls_ngd;
  for (int pass = 0; pass < 2; ++pass)
    for (int ku = 0; ku <= kmax; ++ku)
      for (int kd = 0; kd <= kmax; ++kd) {
        if (!ungrp[ku] || !dngrp_all[kd]) continue;
        RdmClass c{};
        c.du = (int32_t)binom(nred, s.nup - ku);
        c.dd = (int32_t)binom(nred, s.ndw - kd);
        c.n = c.du * c.dd;
        if ((c.n <= small_n) != (pass == 0)) continue;
        c.nt = (c.n + 1) / 2;
        c.ntiles = c.nt * (c.nt + 1) / 2;
        if (c.ntiles > RDM_THREADS) return "reduced density matrix: a class block exceeds the register tiles";
        c.nrep = (pass == 1 && c.ntiles <= 64) ? RDM_THREADS / 64 : 1;
        // LDS of the tile kernel: component (iu, id) of pair b of the batch at id*stride + b*du + iu, stride = du (mod 16) so that the
        // components of one pair fall on consecutive 16-byte bank slots
        for (c.batch = RDM_XS / c.n; c.batch >= 1; --c.batch) {
          c.stride = c.batch * c.du;
          while (c.stride % 16 != c.du % 16) ++c.stride;
          if ((int64_t)c.dd * c.stride <= RDM_XS) break;
        }
        if (c.batch < 1) return "reduced density matrix: a class block exceeds the staging area";
        c.ngu = ungrp[ku];
        c.rows_off = rows_off[ku];
        c.cols_off = cols_off[kd];
        c.tile_off = (int32_t)tiles.size();
        RdmClassHost h;
        for (int tj = 0; tj < c.nt; ++tj)
          for (int ti = 0; ti <= tj; ++ti) h.tiles.push_back((uint32_t)ti | ((uint32_t)tj << 16));
        tiles.insert(tiles.end(), h.tiles.begin(), h.tiles.end());
        for (uint32_t a = 0; a < (1u << nred); ++a) {
          if (__builtin_popcount(a) == s.nup - ku) h.au.push_back(a);
          if (__builtin_popcount(a) == s.ndw - kd) h.ad.push_back(a);
        }
        h.out_off = t.out_elems;
        t.out_elems += (int64_t)c.ntiles * 4;
        t.cls.push_back(c);
        t.hcls.push_back(h);
        cls_ngd.push_back(dngrp[kd]);
      }
  // work list: each class's pairs cut into slices of about (local amplitudes) / (RDM_WG_PER_CU * compute units) amplitudes; the pair kernel
  // takes a workgroup's width of pairs at least, a pair of the tile kernel counts for at least RDM_PAIR_COST / nrep amplitudes
  const int64_t local = (int64_t)s.dimup * std::max(s.qdw, 0);
  const int64_t chunk = std::max<int64_t>(1, local / std::max(1, RDM_WG_PER_CU * ncu));
  std::vector<RdmItem> items;
  const size_t ncls = t.cls.size();
  std::vector<int64_t> first_off(ncls, 0);
  std::vector<int32_t> nparts(ncls, 0);
  for (size_t ci = 0; ci < ncls; ++ci) {
    const RdmClass& c = t.cls[ci];
    const bool small = c.n <= small_n;
    const int64_t npairs = (int64_t)c.ngu * cls_ngd[ci], sz = (int64_t)c.ntiles * 4 * c.nrep;
    if (npairs >= INT32_MAX - RDM_THREADS) return "reduced density matrix: too many pairs";
    const int64_t per = small ? std::max<int64_t>(RDM_THREADS, chunk / c.n) : std::max<int64_t>(1, chunk / std::max(c.n, RDM_PAIR_COST / c.nrep));
    first_off[ci] = t.partial_elems;
    for (int64_t p = 0; p < npairs; p += per) {
      RdmItem it{};
      it.cls = (int32_t)ci;
      it.p0 = (int32_t)p;
      it.p1 = (int32_t)std::min(npairs, p + per);
      it.out_off = t.partial_elems;
      t.partial_elems += sz;
      items.push_back(it);
      ++nparts[ci];
    }
    t.nitems[small ? 0 : 1] += nparts[ci];
  }
  if (items.size() >= (size_t)INT32_MAX) return "reduced density matrix: too many work items";
  std::vector<int64_t> el_src((size_t)t.out_elems);
  std::vector<int32_t> el_cnt((size_t)t.out_elems), el_stride((size_t)t.out_elems);
  for (size_t ci = 0; ci < ncls; ++ci) {
    const int64_t sz = (int64_t)t.cls[ci].ntiles * 4;  // (an item of the class holds nrep partial blocks in a row)
    for (int64_t e = 0; e < sz; ++e) {
      el_src[(size_t)(t.hcls[ci].out_off + e)] = first_off[ci] + e;
      el_cnt[(size_t)(t.hcls[ci].out_off + e)] = nparts[ci] * t.cls[ci].nrep;
      el_stride[(size_t)(t.hcls[ci].out_off + e)] = (int32_t)sz;
    }
  }
  TableArena ar;
  (void)ar.add(t.cls, &t.d_cls);
  (void)ar.add(items, &t.d_items);
  (void)ar.add(rows, &t.d_rows);
  (void)ar.add(cols, &t.d_cols);
  (void)ar.add(tiles, &t.d_tiles);
  (void)ar.add(el_src, &t.d_el_src);
  (void)ar.add(el_cnt, &t.d_el_cnt);
  (void)ar.add(el_stride, &t.d_el_stride);
  hipError_t e = ar.commit(&t.base, &t.bytes);
  if (e != hipSuccess) return std::string("reduced density matrix tables: ") + hipGetErrorString(e);
  return std::string();
}

// src: the column slots the dw groups name ([nranks*cmax][pitch] gathered copy, or this rank's slab itself); pad rows are never read.
// One thread per pair of a class with n <= 4; component k = iu + du*id of the pair is x[k], components past n are zero.
__global__ void __launch_bounds__(RDM_THREADS) rdm_pair_kernel(const double2* __restrict__ src, int pitch, const RdmClass* __restrict__ cls,
                                                               const RdmItem* __restrict__ items, const uint32_t* __restrict__ rows,
                                                               const uint32_t* __restrict__ cols, const uint32_t* __restrict__ tiles,
                                                               double2* __restrict__ partial) {
  constexpr int N = RDM_SMALL_N;
  __shared__ double2 red[RDM_THREADS / 64][N * N];
  const RdmItem it = items[blockIdx.x];
  const RdmClass c = cls[it.cls];
  const int tid = threadIdx.x;
  const uint32_t* __restrict__ crow = rows + c.rows_off;
  const uint32_t* __restrict__ ccol = cols + c.cols_off;
  double2 acc[N][N];  // the upper triangle is used
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) acc[i][j] = make_double2(0.0, 0.0);
  for (int base = it.p0; base < it.p1; base += RDM_THREADS) {
    const int p = base + tid;
    if (p < it.p1) {
      const int gd = p / c.ngu, g = p - gd * c.ngu;
      uint32_t sg[N];
      double2 x[N];
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const int kk = min(k, c.n - 1);  // past the block: a repeated load, zeroed below
        const uint32_t r = crow[g * c.du + kk % c.du], cc = ccol[gd * c.dd + kk / c.du];
        sg[k] = (r ^ cc) >> 31;
        x[k] = src[(int64_t)(cc & 0x7fffffffu) * pitch + (int64_t)(r & 0x7fffffffu)];
      }
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const double f = k < c.n ? (sg[k] ? -1.0 : 1.0) : 0.0;
        x[k] = make_double2(f * x[k].x, f * x[k].y);
      }
#pragma unroll
      for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j) {
          acc[i][j].x += x[i].x * x[j].x + x[i].y * x[j].y;  // x_i * conj(x_j)
          acc[i][j].y += x[i].y * x[j].x - x[i].x * x[j].y;
        }
    }
  }
  // the workgroup's sum in a fixed order: xor butterfly inside each wave (every lane ends with the same bits), then wave 0, 1, 2, 3
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = i; j < N; ++j) {
      double re = acc[i][j].x, im = acc[i][j].y;
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        re += __shfl_xor(re, m, 64);
        im += __shfl_xor(im, m, 64);
      }
      if ((tid & 63) == 0) red[tid >> 6][i * N + j] = make_double2(re, im);
    }
  __syncthreads();
  if (tid < c.ntiles * 4) {
    const uint32_t pk = tiles[c.tile_off + (tid >> 2)];
    const int i = (int)(pk & 0xffffu) * 2 + ((tid >> 1) & 1), j = (int)(pk >> 16) * 2 + (tid & 1);
    double2 v = make_double2(0.0, 0.0);
    if (i <= j && j < N)
      for (int w = 0; w < RDM_THREADS / 64; ++w) {
        v.x += red[w][i * N + j].x;
        v.y += red[w][i * N + j].y;
      }
    partial[it.out_off + tid] = v;
  }
}

// The register-tile scheme of cdm_accumulate_kernel<2, 1> (hxv_cluster_dm.hip), columns carrying a sign bit as the rows do.
__global__ void __launch_bounds__(RDM_THREADS) rdm_tile_kernel(const double2* __restrict__ src, int pitch, const RdmClass* __restrict__ cls,
                                                               const RdmItem* __restrict__ items, const uint32_t* __restrict__ rows,
                                                               const uint32_t* __restrict__ cols, const uint32_t* __restrict__ tiles,
                                                               double2* __restrict__ partial) {
  constexpr int T = 2;
  __shared__ double2 xs[RDM_XS];
  const RdmItem it = items[blockIdx.x];
  const RdmClass c = cls[it.cls];
  const int tid = threadIdx.x;
  // this thread's tile: LDS offsets of its T row and T column components (indices past the block edge repeat the last component: those
  // elements are computed, stored and never used)
  const int tile = c.nrep > 1 ? (tid & 63) : tid;
  const bool live = tile < c.ntiles;
  int offi[T], offj[T];
  double2 acc[T][T];
  {
    const uint32_t pk = tiles[c.tile_off + (live ? tile : 0)];
    const int ti = (int)(pk & 0xffffu), tj = (int)(pk >> 16);
#pragma unroll
    for (int a = 0; a < T; ++a) {
      const int i = min(ti * T + a, c.n - 1), j = min(tj * T + a, c.n - 1);
      offi[a] = (i / c.du) * c.stride + (i % c.du);
      offj[a] = (j / c.du) * c.stride + (j % c.du);
#pragma unroll
      for (int b = 0; b < T; ++b) acc[a][b] = make_double2(0.0, 0.0);
    }
  }
  const uint32_t* __restrict__ crow = rows + c.rows_off;
  const uint32_t* __restrict__ ccol = cols + c.cols_off;
  const int gd0 = it.p0 / c.ngu, gd1 = (it.p1 - 1) / c.ngu;
  for (int gd = gd0; gd <= gd1; ++gd) {
    const int lo = gd == gd0 ? it.p0 - gd0 * c.ngu : 0, hi = gd == gd1 ? it.p1 - gd1 * c.ngu : c.ngu;
    for (int g0 = lo; g0 < hi; g0 += c.batch) {
      const int bc = min(c.batch, hi - g0), nk = bc * c.du;
      __syncthreads();
      for (int k0 = 0; k0 < nk; k0 += RDM_THREADS) {
        const int k = k0 + tid;  // k = b * du + iu: the position in the row table and in the staging area
        if (k < nk) {
          const uint32_t r = crow[g0 * c.du + k];
          const int64_t row = (int64_t)(r & 0x7fffffffu);
          for (int id0 = 0; id0 < c.dd; id0 += RDM_LOADS) {
            double2 x[RDM_LOADS];
            uint32_t sg[RDM_LOADS];
#pragma unroll
            for (int u = 0; u < RDM_LOADS; ++u) {
              const uint32_t cc = ccol[gd * c.dd + min(id0 + u, c.dd - 1)];
              sg[u] = (r ^ cc) >> 31;
              x[u] = src[(int64_t)(cc & 0x7fffffffu) * pitch + row];
            }
#pragma unroll
            for (int u = 0; u < RDM_LOADS; ++u)
              if (id0 + u < c.dd) {
                const double f = sg[u] ? -1.0 : 1.0;
                xs[(id0 + u) * c.stride + k] = make_double2(f * x[u].x, f * x[u].y);
              }
          }
        }
      }
      __syncthreads();
      if (live)
        for (int b = c.nrep > 1 ? (tid >> 6) : 0; b < bc; b += c.nrep) {
          const int o = b * c.du;
          double2 xi[T], xj[T];
#pragma unroll
          for (int a = 0; a < T; ++a) {
            xi[a] = xs[offi[a] + o];
            xj[a] = xs[offj[a] + o];
          }
#pragma unroll
          for (int a = 0; a < T; ++a)
#pragma unroll
            for (int q = 0; q < T; ++q) {
              acc[a][q].x += xi[a].x * xj[q].x + xi[a].y * xj[q].y;  // x_i * conj(x_j)
              acc[a][q].y += xi[a].y * xj[q].x - xi[a].x * xj[q].y;
            }
        }
    }
  }
  if (live) {
    double2* __restrict__ out = partial + it.out_off + (c.nrep > 1 ? (int64_t)(tid >> 6) * c.ntiles * (T * T) : 0);
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
      for (int q = 0; q < T; ++q) out[(int64_t)tile * (T * T) + a * T + q] = acc[a][q];
  }
}

// out[e] = the partial blocks' element, summed in work-list order (cnt may be 0: a rank without dw groups of the class)
__global__ void __launch_bounds__(RDM_THREADS) rdm_reduce_kernel(const double2* __restrict__ partial, const int64_t* __restrict__ el_src,
                                                                 const int32_t* __restrict__ el_cnt, const int32_t* __restrict__ el_stride,
                                                                 int64_t nel, double2* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * RDM_THREADS + threadIdx.x;
  if (e >= nel) return;
  const double2* __restrict__ p = partial + el_src[e];
  const int n = el_cnt[e];
  const int64_t st = el_stride[e];
  double2 acc = make_double2(0.0, 0.0);
  for (int k = 0; k < n; ++k) {
    const double2 v = p[k * st];
    acc.x += v.x;
    acc.y += v.y;
  }
  out[e] = acc;
}

// class blocks -> the dense matrix, element (io,jo) at 2*(io + 4^Nred*jo); weight * raw is rounded before it is added, so that an
// accumulated matrix equals the sum of the single results bit for bit
void scatter(const RdmTables& t, const std::vector<double2>& raw, double weight, bool accumulate, double* rdm) {
#pragma clang fp contract(off)
  const int64_t nn = (int64_t)1 << (2 * t.nred);
  if (!accumulate) std::memset(rdm, 0, (size_t)(2 * nn * nn) * sizeof(double));
  for (size_t ci = 0; ci < t.cls.size(); ++ci) {
    const RdmClass& c = t.cls[ci];
    const RdmClassHost& h = t.hcls[ci];
    auto orb = [&](int i) -> int64_t { return (int64_t)h.au[i % c.du] + ((int64_t)h.ad[i / c.du] << t.nred); };
    for (int tile = 0; tile < c.ntiles; ++tile) {
      const int ti = (int)(h.tiles[tile] & 0xffffu), tj = (int)(h.tiles[tile] >> 16);
      for (int a = 0; a < 2; ++a)
        for (int q = 0; q < 2; ++q) {
          const int i = ti * 2 + a, j = tj * 2 + q;
          if (i > j || j >= c.n) continue;
          const double2 v = raw[(size_t)(h.out_off + (int64_t)tile * 4 + a * 2 + q)];
          const double re = weight * v.x, im = i == j ? 0.0 : weight * v.y;
          const int64_t io = orb(i), jo = orb(j);
          rdm[2 * (io + nn * jo)] += re;
          rdm[2 * (io + nn * jo) + 1] += im;
          if (i != j) {
            rdm[2 * (jo + nn * io)] += re;
            rdm[2 * (jo + nn * io) + 1] -= im;
          }
        }
    }
  }
}

bool has_maps(const hxv_handle* h) { return !h->host.map_up.empty() && !h->host.map_dw.empty() && h->host.panel_rows == 0; }
}  // namespace

extern "C" {

int64_t hxv_reduced_dm_elems(const hxv_handle* h, uint32_t orbital_mask) {
  if (!h || !has_maps(h)) return 0;
  const int n = nimp_of(h->host);
  if (n < 1 || n > h->host.ns || n > 32) return 0;
  const int nred = __builtin_popcount(orbital_mask);
  if (nred < 1 || nred > RDM_MAX_NRED || (n < 32 && (orbital_mask >> n))) return 0;
  return (int64_t)2 << (4 * nred);
}

int hxv_reduced_dm_accumulate(hxv_handle* h, const void* d_psi, uint32_t orbital_mask, int32_t fermi_sign, double weight, int32_t accumulate,
                              double* rdm) {
  if (!h || !d_psi || !rdm) return fail(HXV_ERR_ARG, "hxv_reduced_dm_accumulate: NULL argument");
  if (fermi_sign != 0 && fermi_sign != 1) return fail(HXV_ERR_ARG, "hxv_reduced_dm_accumulate: fermi_sign is 0 or 1");
  if (!orbital_mask) return fail(HXV_ERR_ARG, "hxv_reduced_dm_accumulate: empty orbital mask");
  const SectorHost& s = h->host;
  if (!has_maps(h)) return fail(HXV_ERR_STATE, "hxv_reduced_dm_accumulate needs a handle built from a model (basis maps)");
  const int nimp = nimp_of(s);
  if (nimp < 1 || nimp > s.ns || nimp > 32) return fail(HXV_ERR_STATE, "hxv_reduced_dm_accumulate: the handle carries no impurity size");
  if (nimp < 32 && (orbital_mask >> nimp)) return fail(HXV_ERR_ARG, "hxv_reduced_dm_accumulate: the orbital mask names bits outside the Nimp impurity orbitals");
  if (__builtin_popcount(orbital_mask) > RDM_MAX_NRED) return fail(HXV_ERR_UNSUPPORTED, "hxv_reduced_dm_accumulate: more than 4 orbitals in the mask");
  const bool split = s.nranks > 1;
  if (split && !comm_ready(h)) return fail(HXV_ERR_STATE, "hxv_reduced_dm_accumulate on a split sector needs the communicator (hxv_comm_init after opening it)");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  // rank-local preparation: tables (cached by mask and convention in the sector image), scratch; every rank learns whether all could go on
  int rc_local = HXV_OK;
  std::shared_ptr<RdmTables> t;
  {
    const char* ab = std::getenv("HXV_RDM_PAIR_KERNEL");
    const int small_n = (ab && ab[0] == '0' && !ab[1]) ? 0 : RDM_SMALL_N;
    const uint64_t key = (uint64_t)orbital_mask | ((uint64_t)fermi_sign << 32) | ((uint64_t)(small_n == 0) << 33);
    std::lock_guard<std::mutex> lk(h->img->rdm_mu);
    auto& cache = h->img->rdm;
    for (size_t i = 0; i < cache.size() && !t; ++i)
      if (cache[i].first == key) {
        t = cache[i].second;
        std::rotate(cache.begin() + i, cache.begin() + i + 1, cache.end());  // most recently used last
      }
    if (!t) {
      int ncu = 0;
      if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || ncu < 1) ncu = 256;
      auto nt = std::make_shared<RdmTables>();
      const std::string err = build_tables(s, orbital_mask, fermi_sign, small_n, h->device, ncu, *nt);
      if (err.empty()) {
        if (cache.size() >= RDM_CACHE) cache.erase(cache.begin());  // a call under way keeps its tables alive through its own reference
        cache.emplace_back(key, nt);
        t = nt;
      } else
        rc_local = fail(err.rfind("reduced density matrix tables", 0) == 0 ? HXV_ERR_HIP : HXV_ERR_STATE, err);
    }
  }
  double2 *d_part = nullptr, *d_out = nullptr, *d_full = nullptr;
  if (rc_local == HXV_OK) {
    hipError_t e1 = pool_alloc(h->device, std::max<size_t>((size_t)t->partial_elems, 1) * sizeof(double2), (void**)&d_part);
    hipError_t e2 = pool_alloc(h->device, std::max<size_t>((size_t)t->out_elems, 1) * sizeof(double2), (void**)&d_out);
    hipError_t e3 = split ? pool_alloc(h->device, std::max<size_t>((size_t)s.nranks * s.cmax * s.pitch, 1) * sizeof(double2), (void**)&d_full) : hipSuccess;
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) rc_local = fail(HXV_ERR_HIP, "hxv_reduced_dm_accumulate: scratch buffers");
  }
  auto release = [&]() {
    (void)hipStreamSynchronize(st);
    if (d_part) pool_free(h->device, d_part);
    if (d_out) pool_free(h->device, d_out);
    if (d_full) pool_free(h->device, d_full);
  };
  int rc = split ? comm_agree(h, rc_local) : rc_local;
  if (rc) {
    release();
    return rc;
  }
  const double2* psi = (const double2*)d_psi;
  if (split) {
    rc = comm_allgather_slab(h, psi, d_full, st);
    if (rc) {
      release();
      return rc;
    }
  }
  const double2* src = split ? (const double2*)d_full : psi;
  if (t->nitems[0] > 0)
    hipLaunchKernelGGL(rdm_pair_kernel, dim3((unsigned)t->nitems[0]), dim3(RDM_THREADS), 0, st, src, s.pitch, t->d_cls, t->d_items, t->d_rows,
                       t->d_cols, t->d_tiles, d_part);
  if (t->nitems[1] > 0)
    hipLaunchKernelGGL(rdm_tile_kernel, dim3((unsigned)t->nitems[1]), dim3(RDM_THREADS), 0, st, src, s.pitch, t->d_cls,
                       t->d_items + t->nitems[0], t->d_rows, t->d_cols, t->d_tiles, d_part);
  hipLaunchKernelGGL(rdm_reduce_kernel, dim3((unsigned)((t->out_elems + RDM_THREADS - 1) / RDM_THREADS)), dim3(RDM_THREADS), 0, st,
                     (const double2*)d_part, t->d_el_src, t->d_el_cnt, t->d_el_stride, t->out_elems, d_out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    release();
    return fail(HXV_ERR_HIP, std::string("reduced density matrix kernels: ") + hipGetErrorString(e));
  }
  if (split) {
    rc = comm_allreduce_sum(h, (double*)d_out, (size_t)(2 * t->out_elems), st);
    if (rc) {
      release();
      return rc;
    }
  }
  std::vector<double2> raw((size_t)t->out_elems);
  e = hipMemcpyAsync(raw.data(), d_out, (size_t)t->out_elems * sizeof(double2), hipMemcpyDeviceToHost, st);
  release();
  if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("hxv_reduced_dm_accumulate: ") + hipGetErrorString(e));
  scatter(*t, raw, weight, accumulate != 0, rdm);
  return HXV_OK;
}

}  // extern "C"
