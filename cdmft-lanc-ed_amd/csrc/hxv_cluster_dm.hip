// Cluster reduced density matrix of a device-resident state (include/hxv.h: hxv_cluster_dm_accumulate).
//
// rho_imp = Tr_bath |psi><psi| (density_matrix_impurity, ED_OBSERVABLES.f90:465-582):
//   rho(io,jo) += peso * sum_{b_up,b_dw} psi(a_up,b_up ; a_dw,b_dw) * conj psi(a'_up,b_up ; a'_dw,b_dw),   io = a_up + 2^Nimp a_dw  (0-based)
// A spin configuration is a + 2^Nimp * b (impurity bits low, bath bits high, :539-562) and the reference's basis maps are sorted by that
// integer, so the up rows that share the bath configuration b_up are a contiguous run of dU = C(Nimp, nup - |b_up|) rows of the reference's
// order and the dw columns that share b_dw a contiguous run of dD columns.  rho is therefore a sum of Hermitian rank-1 updates x x^+, one
// per pair (b_up, b_dw), x the (dU*dD)-vector of that pair's amplitudes, and it is block-diagonal in the impurity particle numbers: the
// pairs fall into CLASSES (|b_up|, |b_dw|), each with one dU*dD x dU*dD block.
//   cdm_accumulate_kernel<T,NT>  one workgroup per item of a host-built work list; an item is a slice of one class's pairs (the list is cut
//                      by amplitude count, with a floor per pair).  The workgroup stages the amplitudes of a batch of pairs through LDS
//                      (16-byte loads; a batch takes consecutive up groups of the class, whose rows are runs of the reference's order
//                      within a group and runs of the device row order of C3 across groups: one load instruction covers either) and
//                      keeps the upper triangle of the class block in registers, NT tiles of T x T elements per thread; it writes one
//                      partial block (four, one per wave, where the block's tiles fit one wave and the waves share out a batch's pairs).
//   cdm_reduce_kernel  one thread per class-block element: the partials of its class, summed in list order.
// No floating-point atomics: the same vector on the same handle gives the same bits on every call.  The group tables are built on the host in
// device-row numbering (the basis signs of the device row order folded into the row entry) and cached with the sector image.  On a split
// sector a dw group belongs to the rank that owns its first column and reads the gathered copy; the class blocks are all-reduced.  The host
// scatters the class blocks into the dense matrix and fills the lower triangle by conjugation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "hxv_handle.hpp"

using namespace hxv;

namespace {
constexpr int CDM_THREADS = 256;
constexpr int CDM_XS = 2048;      // LDS staging area, amplitudes (32 KB)
constexpr int CDM_PAIR_COST = 36;  // work-list balance: a pair costs one trip of its wave's register loop however small its block, about
                                   // what a pair of 36 amplitudes costs in all (the tail of a list cut by amplitudes alone: 1 x 1 blocks)
constexpr int CDM_LOADS = 4;       // 16-byte loads a thread has in flight while staging
constexpr int CDM_MAX_NIMP = 5;   // the dense matrix: 16 MB at Nimp 5, 268 MB at Nimp 6
constexpr int CDM_WG_PER_CU = 4;  // work items per compute unit the list is cut for

struct CdmClass {
  int32_t du, dd, n;       // block shape: n = du*dd
  int32_t t, nt, ntiles;   // tile edge, tiles per side, tiles of the upper triangle
  int32_t batch, stride;   // pairs staged at once; LDS elements between the dw components of the staged amplitudes
  int32_t ngu;             // up groups of the class
  int32_t rows_off;        // into rows: [ngu][du] device row | sign << 31
  int32_t cols_off;        // into cols: [local dw groups][dd] column slot
  int32_t tile_off;        // into tiles: ti | tj << 16
  int32_t nrep;            // 4: the block's tiles fit one wave, so each of the four waves takes every fourth pair of a batch and writes a
                           // partial block of its own; 1: the tiles are spread over the workgroup
};
struct CdmItem {
  int32_t cls, p0, p1, pad;  // pairs [p0, p1) of the class, pair = (local dw group) * ngu + (up group)
  int64_t out_off;           // its partial block in the partial buffer (elements)
};
struct CdmClassHost {
  int64_t out_off = 0;                // the class block in the reduced output (elements), ntiles*t*t of them
  std::vector<uint32_t> au, ad;       // impurity configurations of the block's up / dw components
  std::vector<uint32_t> tiles;
};
}  // namespace

namespace hxv {
struct SectorImage::CdmTables {
  int nimp = 0;
  std::vector<CdmClass> cls;
  std::vector<CdmClassHost> hcls;
  int nitems[2] = {0, 0};   // items of the T = 2 classes, then of the T = 4 classes
  int64_t partial_elems = 0, out_elems = 0;
  CdmClass* d_cls = nullptr;
  CdmItem* d_items = nullptr;
  uint32_t *d_rows = nullptr, *d_tiles = nullptr;
  int32_t *d_cols = nullptr, *d_el_cnt = nullptr, *d_el_stride = nullptr;
  int64_t* d_el_src = nullptr;
  void* base = nullptr;
  int device = -1;
  int64_t bytes = 0;
  ~CdmTables() {
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
using CdmTables = SectorImage::CdmTables;

int64_t binom(int n, int k) {
  if (k < 0 || k > n) return 0;
  int64_t r = 1;
  for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;
  return r;
}

// runs of equal bath configuration in a sorted basis map: (first index, bath particle number) per group
void bath_groups(const std::vector<uint32_t>& map, int nimp, std::vector<int32_t>& first, std::vector<int32_t>& nb) {
  for (size_t i = 0; i < map.size(); ++i)
    if (i == 0 || (map[i] >> nimp) != (map[i - 1] >> nimp)) {
      first.push_back((int32_t)i);
      nb.push_back(__builtin_popcount(map[i] >> nimp));
    }
  first.push_back((int32_t)map.size());
}

std::string build_tables(const SectorHost& s, int nimp, int device, int ncu, CdmTables& t) {
  t.nimp = nimp;
  t.device = device;
  const uint32_t mask = (1u << nimp) - 1u;
  const bool ro = s.row_order();
  std::vector<int32_t> ufirst, unb, dfirst, dnb;
  bath_groups(s.map_up, nimp, ufirst, unb);
  bath_groups(s.map_dw, nimp, dfirst, dnb);
  const int nbath = s.ns - nimp;
  // owner of a dw column / its slot in the gathered copy (the padded all-gather layout), as the observables' dw pairs
  std::vector<int32_t> rfirst(s.nranks + 1, 0);
  for (int p = 0; p < s.nranks; ++p) {
    int q, c0;
    dw_split(s.dimdw, p, s.nranks, q, c0);
    rfirst[p] = c0;
  }
  rfirst[s.nranks] = s.dimdw;
  auto slot_of = [&](int c) -> int32_t {
    if (s.nranks == 1) return c;
    const int o = (int)(std::upper_bound(rfirst.begin(), rfirst.end(), c) - rfirst.begin()) - 1;
    return o * s.cmax + (c - rfirst[o]);
  };
  // per bath particle number: the up groups' rows, this rank's dw groups' columns
  std::vector<std::vector<uint32_t>> urows(nbath + 1);
  std::vector<std::vector<int32_t>> dcols(nbath + 1);
  std::vector<int32_t> ungrp(nbath + 1, 0), dngrp(nbath + 1, 0), dngrp_all(nbath + 1, 0);
  for (size_t g = 0; g + 1 < ufirst.size(); ++g) {
    const int k = unb[g], du = ufirst[g + 1] - ufirst[g];
    if (k > nbath || du != binom(nimp, s.nup - k)) return "cluster density matrix: the up basis is not sorted by bath configuration";
    for (int i = ufirst[g]; i < ufirst[g + 1]; ++i) {
      const int r = ro ? s.up_perm[i] : i;
      urows[k].push_back((uint32_t)r | ((ro && s.up_sign[r]) ? 0x80000000u : 0u));
    }
    ++ungrp[k];
  }
  for (size_t g = 0; g + 1 < dfirst.size(); ++g) {
    const int k = dnb[g], dd = dfirst[g + 1] - dfirst[g];
    if (k > nbath || dd != binom(nimp, s.ndw - k)) return "cluster density matrix: the dw basis is not sorted by bath configuration";
    ++dngrp_all[k];
    if (dfirst[g] < s.dw0 || dfirst[g] >= s.dw0 + s.qdw) continue;  // the rank that owns the first column takes the group
    for (int c = dfirst[g]; c < dfirst[g + 1]; ++c) dcols[k].push_back(slot_of(c));
    ++dngrp[k];
  }
  // classes: every (up, dw) bath particle number pair of the WHOLE sector, the same list on every rank; T = 2 classes first
  std::vector<uint32_t> rows, tiles;
  std::vector<int32_t> cols;
  std::vector<int32_t> rows_off(nbath + 1, 0), cols_off(nbath + 1, 0);
  for (int k = 0; k <= nbath; ++k) {
    rows_off[k] = (int32_t)rows.size();
    rows.insert(rows.end(), urows[k].begin(), urows[k].end());
    cols_off[k] = (int32_t)cols.size();
    cols.insert(cols.end(), dcols[k].begin(), dcols[k].end());
  }
  std::vector<int32_t> cls_ngd;
  for (int pass = 0; pass < 2; ++pass)
    for (int ku = 0; ku <= nbath; ++ku)
      for (int kd = 0; kd <= nbath; ++kd) {
        if (!ungrp[ku] || !dngrp_all[kd]) continue;
        CdmClass c{};
        c.du = (int32_t)binom(nimp, s.nup - ku);
        c.dd = (int32_t)binom(nimp, s.ndw - kd);
        c.n = c.du * c.dd;
        const int nt2 = (c.n + 1) / 2;
        c.t = nt2 * (nt2 + 1) / 2 <= CDM_THREADS ? 2 : 4;
        if ((c.t == 2) != (pass == 0)) continue;
        c.nt = (c.n + c.t - 1) / c.t;
        c.ntiles = c.nt * (c.nt + 1) / 2;
        if (c.ntiles > 2 * CDM_THREADS) return "cluster density matrix: a class block exceeds the register tiles";
        c.nrep = c.ntiles <= 64 ? CDM_THREADS / 64 : 1;
        // LDS: component (iu, id) of pair b of the batch at id*stride + b*du + iu, stride = du (mod 16) so that the components of one pair
        // fall on consecutive 16-byte bank slots
        for (c.batch = CDM_XS / c.n; c.batch >= 1; --c.batch) {
          c.stride = c.batch * c.du;
          while (c.stride % 16 != c.du % 16) ++c.stride;
          if ((int64_t)c.dd * c.stride <= CDM_XS) break;
        }
        if (c.batch < 1) return "cluster density matrix: a class block exceeds the staging area";
        c.ngu = ungrp[ku];
        c.rows_off = rows_off[ku];
        c.cols_off = cols_off[kd];
        c.tile_off = (int32_t)tiles.size();
        CdmClassHost h;
        for (int tj = 0; tj < c.nt; ++tj)
          for (int ti = 0; ti <= tj; ++ti) h.tiles.push_back((uint32_t)ti | ((uint32_t)tj << 16));
        tiles.insert(tiles.end(), h.tiles.begin(), h.tiles.end());
        for (uint32_t a = 0; a <= mask; ++a) {
          if (__builtin_popcount(a) == s.nup - ku) h.au.push_back(a);
          if (__builtin_popcount(a) == s.ndw - kd) h.ad.push_back(a);
        }
        h.out_off = t.out_elems;
        t.out_elems += (int64_t)c.ntiles * c.t * c.t;
        t.cls.push_back(c);
        t.hcls.push_back(h);
        cls_ngd.push_back(dngrp[kd]);
      }
  // work list: each class's pairs cut into slices of about (local amplitudes) / (CDM_WG_PER_CU * compute units) amplitudes, a pair counting
  // for at least CDM_PAIR_COST / nrep of them
  const int64_t local = (int64_t)s.dimup * std::max(s.qdw, 0);
  const int64_t chunk = std::max<int64_t>(1, local / std::max(1, CDM_WG_PER_CU * ncu));
  std::vector<CdmItem> items;
  const size_t ncls = t.cls.size();
  std::vector<int64_t> first_off(ncls, 0);
  std::vector<int32_t> nparts(ncls, 0);
  for (size_t ci = 0; ci < ncls; ++ci) {
    const CdmClass& c = t.cls[ci];
    const int64_t npairs = (int64_t)c.ngu * cls_ngd[ci], sz = (int64_t)c.ntiles * c.t * c.t * c.nrep;
    if (npairs >= INT32_MAX) return "cluster density matrix: too many bath pairs";
    const int64_t per = std::max<int64_t>(1, chunk / std::max(c.n, CDM_PAIR_COST / c.nrep));
    first_off[ci] = t.partial_elems;
    for (int64_t p = 0; p < npairs; p += per) {
      CdmItem it{};
      it.cls = (int32_t)ci;
      it.p0 = (int32_t)p;
      it.p1 = (int32_t)std::min(npairs, p + per);
      it.out_off = t.partial_elems;
      t.partial_elems += sz;
      items.push_back(it);
      ++nparts[ci];
    }
    t.nitems[c.t == 2 ? 0 : 1] += nparts[ci];
  }
  if (items.size() >= (size_t)INT32_MAX) return "cluster density matrix: too many work items";
  std::vector<int64_t> el_src((size_t)t.out_elems);
  std::vector<int32_t> el_cnt((size_t)t.out_elems), el_stride((size_t)t.out_elems);
  for (size_t ci = 0; ci < ncls; ++ci) {
    const int64_t sz = (int64_t)t.cls[ci].ntiles * t.cls[ci].t * t.cls[ci].t;  // (an item of the class holds nrep partial blocks in a row)
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
  if (e != hipSuccess) return std::string("cluster density matrix tables: ") + hipGetErrorString(e);
  return std::string();
}

// src: the column slots the dw groups name ([nranks*cmax][pitch] gathered copy, or this rank's slab itself); pad rows are never read
template <int T, int NT>
__global__ void __launch_bounds__(CDM_THREADS) cdm_accumulate_kernel(const double2* __restrict__ src, int pitch, const CdmClass* __restrict__ cls,
                                                                     const CdmItem* __restrict__ items, const uint32_t* __restrict__ rows,
                                                                     const int32_t* __restrict__ cols, const uint32_t* __restrict__ tiles,
                                                                     double2* __restrict__ partial) {
  __shared__ double2 xs[CDM_XS];
  const CdmItem it = items[blockIdx.x];
  const CdmClass c = cls[it.cls];
  const int tid = threadIdx.x;
  // this thread's tiles: LDS offsets of their T row and T column components (indices past the block edge repeat the last component: those
  // elements are computed, stored and never used)
  int offi[NT][T], offj[NT][T];
  bool live[NT];
  double2 acc[NT][T][T];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int tile = (c.nrep > 1 ? (tid & 63) : tid) + t * CDM_THREADS;
    live[t] = tile < c.ntiles;
    const uint32_t pk = tiles[c.tile_off + (live[t] ? tile : 0)];
    const int ti = (int)(pk & 0xffffu), tj = (int)(pk >> 16);
#pragma unroll
    for (int a = 0; a < T; ++a) {
      const int i = min(ti * T + a, c.n - 1), j = min(tj * T + a, c.n - 1);
      offi[t][a] = (i / c.du) * c.stride + (i % c.du);
      offj[t][a] = (j / c.du) * c.stride + (j % c.du);
#pragma unroll
      for (int b = 0; b < T; ++b) acc[t][a][b] = make_double2(0.0, 0.0);
    }
  }
  const uint32_t* __restrict__ crow = rows + c.rows_off;
  const int32_t* __restrict__ ccol = cols + c.cols_off;
  const int gd0 = it.p0 / c.ngu, gd1 = (it.p1 - 1) / c.ngu;
  for (int gd = gd0; gd <= gd1; ++gd) {
    const int lo = gd == gd0 ? it.p0 - gd0 * c.ngu : 0, hi = gd == gd1 ? it.p1 - gd1 * c.ngu : c.ngu;
    for (int g0 = lo; g0 < hi; g0 += c.batch) {
      const int bc = min(c.batch, hi - g0), nk = bc * c.du;
      __syncthreads();
      for (int k = tid; k < nk; k += CDM_THREADS) {
        const uint32_t r = crow[g0 * c.du + k];  // k = b * du + iu: the position in the row table and in the staging area
        const int64_t row = (int64_t)(r & 0x7fffffffu);
        const double sg = (r >> 31) ? -1.0 : 1.0;
        for (int id0 = 0; id0 < c.dd; id0 += CDM_LOADS) {
          double2 x[CDM_LOADS];
#pragma unroll
          for (int u = 0; u < CDM_LOADS; ++u) x[u] = src[(int64_t)ccol[gd * c.dd + min(id0 + u, c.dd - 1)] * pitch + row];
#pragma unroll
          for (int u = 0; u < CDM_LOADS; ++u)
            if (id0 + u < c.dd) xs[(id0 + u) * c.stride + k] = make_double2(sg * x[u].x, sg * x[u].y);
        }
      }
      __syncthreads();
      for (int b = c.nrep > 1 ? (tid >> 6) : 0; b < bc; b += c.nrep) {
        const int o = b * c.du;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if (!live[t]) continue;
          double2 xi[T], xj[T];
#pragma unroll
          for (int a = 0; a < T; ++a) {
            xi[a] = xs[offi[t][a] + o];
            xj[a] = xs[offj[t][a] + o];
          }
#pragma unroll
          for (int a = 0; a < T; ++a)
#pragma unroll
            for (int q = 0; q < T; ++q) {
              acc[t][a][q].x += xi[a].x * xj[q].x + xi[a].y * xj[q].y;  // x_i * conj(x_j)
              acc[t][a][q].y += xi[a].y * xj[q].x - xi[a].x * xj[q].y;
            }
        }
      }
    }
  }
  double2* __restrict__ out = partial + it.out_off + (c.nrep > 1 ? (int64_t)(tid >> 6) * c.ntiles * (T * T) : 0);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int tile = (c.nrep > 1 ? (tid & 63) : tid) + t * CDM_THREADS;
    if (!live[t]) continue;
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
      for (int q = 0; q < T; ++q) out[(int64_t)tile * (T * T) + a * T + q] = acc[t][a][q];
  }
}

// out[e] = the partial blocks' element, summed in work-list order (cnt may be 0: a rank without dw groups of the class)
__global__ void __launch_bounds__(CDM_THREADS) cdm_reduce_kernel(const double2* __restrict__ partial, const int64_t* __restrict__ el_src,
                                                                 const int32_t* __restrict__ el_cnt, const int32_t* __restrict__ el_stride,
                                                                 int64_t nel, double2* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * CDM_THREADS + threadIdx.x;
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

// class blocks -> the dense matrix, element (io,jo) at 2*(io + 4^Nimp*jo); weight * raw is rounded before it is added, so that an
// accumulated matrix equals the sum of the single results bit for bit
void scatter(const CdmTables& t, const std::vector<double2>& raw, double weight, bool accumulate, double* cdm) {
#pragma clang fp contract(off)
  const int64_t nn = (int64_t)1 << (2 * t.nimp);
  if (!accumulate) std::memset(cdm, 0, (size_t)(2 * nn * nn) * sizeof(double));
  for (size_t ci = 0; ci < t.cls.size(); ++ci) {
    const CdmClass& c = t.cls[ci];
    const CdmClassHost& h = t.hcls[ci];
    auto orb = [&](int i) -> int64_t { return (int64_t)h.au[i % c.du] + ((int64_t)h.ad[i / c.du] << t.nimp); };
    for (int tile = 0; tile < c.ntiles; ++tile) {
      const int ti = (int)(h.tiles[tile] & 0xffffu), tj = (int)(h.tiles[tile] >> 16);
      for (int a = 0; a < c.t; ++a)
        for (int q = 0; q < c.t; ++q) {
          const int i = ti * c.t + a, j = tj * c.t + q;
          if (i > j || j >= c.n) continue;
          const double2 v = raw[(size_t)(h.out_off + (int64_t)tile * c.t * c.t + a * c.t + q)];
          const double re = weight * v.x, im = i == j ? 0.0 : weight * v.y;
          const int64_t io = orb(i), jo = orb(j);
          cdm[2 * (io + nn * jo)] += re;
          cdm[2 * (io + nn * jo) + 1] += im;
          if (i != j) {
            cdm[2 * (jo + nn * io)] += re;
            cdm[2 * (jo + nn * io) + 1] -= im;
          }
        }
    }
  }
}
}  // namespace

extern "C" {

int64_t hxv_cluster_dm_elems(const hxv_handle* h) {
  if (!h || h->host.map_up.empty() || h->host.map_dw.empty() || h->host.panel_rows > 0) return 0;
  const int n = nimp_of(h->host);
  if (n < 1 || n > CDM_MAX_NIMP || n > h->host.ns) return 0;
  return (int64_t)2 << (4 * n);
}

int hxv_cluster_dm_accumulate(hxv_handle* h, const void* d_psi, double weight, int32_t accumulate, double* cdm) {
  if (!h || !d_psi || !cdm) return fail(HXV_ERR_ARG, "hxv_cluster_dm_accumulate: NULL argument");
  const SectorHost& s = h->host;
  if (s.map_up.empty() || s.map_dw.empty() || s.panel_rows > 0)
    return fail(HXV_ERR_STATE, "hxv_cluster_dm_accumulate needs a handle built from a model (basis maps)");
  const int nimp = nimp_of(s);
  if (nimp < 1 || nimp > s.ns) return fail(HXV_ERR_STATE, "hxv_cluster_dm_accumulate: the handle carries no impurity size");
  if (nimp > CDM_MAX_NIMP) return fail(HXV_ERR_UNSUPPORTED, "hxv_cluster_dm_accumulate: Nimp > 5 (a dense matrix of 268 MB and more)");
  const bool split = s.nranks > 1;
  if (split && !comm_ready(h)) return fail(HXV_ERR_STATE, "hxv_cluster_dm_accumulate on a split sector needs the communicator (hxv_comm_init after opening it)");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  // rank-local preparation: tables (once per sector image), scratch; every rank learns whether all could go on
  int rc_local = HXV_OK;
  std::shared_ptr<CdmTables> t;
  {
    std::lock_guard<std::mutex> lk(h->img->cdm_mu);
    if (!h->img->cdm) {
      int ncu = 0;
      if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || ncu < 1) ncu = 256;
      auto nt = std::make_shared<CdmTables>();
      const std::string err = build_tables(s, nimp, h->device, ncu, *nt);
      if (err.empty())
        h->img->cdm = nt;
      else
        rc_local = fail(err.rfind("cluster density matrix tables", 0) == 0 ? HXV_ERR_HIP : HXV_ERR_STATE, err);
    }
    t = h->img->cdm;
  }
  double2 *d_part = nullptr, *d_out = nullptr, *d_full = nullptr;
  if (rc_local == HXV_OK) {
    hipError_t e1 = pool_alloc(h->device, std::max<size_t>((size_t)t->partial_elems, 1) * sizeof(double2), (void**)&d_part);
    hipError_t e2 = pool_alloc(h->device, std::max<size_t>((size_t)t->out_elems, 1) * sizeof(double2), (void**)&d_out);
    hipError_t e3 = split ? pool_alloc(h->device, std::max<size_t>((size_t)s.nranks * s.cmax * s.pitch, 1) * sizeof(double2), (void**)&d_full) : hipSuccess;
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) rc_local = fail(HXV_ERR_HIP, "hxv_cluster_dm_accumulate: scratch buffers");
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
    hipLaunchKernelGGL((cdm_accumulate_kernel<2, 1>), dim3((unsigned)t->nitems[0]), dim3(CDM_THREADS), 0, st, src, s.pitch, t->d_cls, t->d_items,
                       t->d_rows, t->d_cols, t->d_tiles, d_part);
  if (t->nitems[1] > 0)
    hipLaunchKernelGGL((cdm_accumulate_kernel<4, 2>), dim3((unsigned)t->nitems[1]), dim3(CDM_THREADS), 0, st, src, s.pitch, t->d_cls,
                       t->d_items + t->nitems[0], t->d_rows, t->d_cols, t->d_tiles, d_part);
  hipLaunchKernelGGL(cdm_reduce_kernel, dim3((unsigned)((t->out_elems + CDM_THREADS - 1) / CDM_THREADS)), dim3(CDM_THREADS), 0, st,
                     (const double2*)d_part, t->d_el_src, t->d_el_cnt, t->d_el_stride, t->out_elems, d_out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    release();
    return fail(HXV_ERR_HIP, std::string("cluster density matrix kernels: ") + hipGetErrorString(e));
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
  if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("hxv_cluster_dm_accumulate: ") + hipGetErrorString(e));
  scatter(*t, raw, weight, accumulate != 0, cdm);
  return HXV_OK;
}

}  // extern "C"
