// The tables of the partial-trace engine (hxv_partial_trace.hip) under hxv_cluster_dm_accumulate and hxv_reduced_dm_accumulate.
//
// rho = Tr_env |psi><psi| is a sum of Hermitian rank-1 updates x x^+, one per pair (up group, dw group): a GROUP is the set of rows (columns)
// that share the traced bits e of their configuration, d = C(nsub, n_spin - |e|) of them, and x the (dU*dD)-vector of the pair's amplitudes.
// rho is block-diagonal in the particle numbers of the kept part: the pairs fall into CLASSES (|e_up|, |e_dw|), each with one
// dU*dD x dU*dD block.  A front end (hxv_partial_trace_groups.cpp) lists the groups of each spin in the order their pairs are to be summed in;
// pt_build turns them into what the kernels read: classes, tile words, a work list of (class, slice of pairs) items and the tables of the
// reduction.  Host C++ only, no HIP: tests/host/partial_trace_check.cpp reads every table on the CPU, under sanitizers.
#pragma once

#include <algorithm>
#include <climits>
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

struct hxv_handle;
namespace hxv {
struct SectorHost;
void dw_split(int dimdw, int rank, int nranks, int& qdw, int& dw0);  // hxv_sector.cpp

constexpr int PT_THREADS = 256;
constexpr int PT_XS = 2048;       // LDS staging area of the tile kernel, amplitudes (32 KB)
constexpr int PT_PAIR_COST = 36;  // work-list balance of the tile kernel: a pair costs one trip of its wave's register loop however small its block,
                                  // about what a pair of 36 amplitudes costs in all (the tail of a list cut by amplitudes alone: 1 x 1 blocks)
constexpr int PT_PAIR_N = 4;      // largest block the pair kernel takes
constexpr int PT_WG_PER_CU = 4;   // work items per compute unit the list is cut for

struct PtClass {
  int32_t du, dd, n;      // block shape: n = du*dd
  int32_t t, nt, ntiles;  // tile edge, tiles per side, tiles of the upper triangle
  int32_t batch, stride;  // tile kernel: pairs staged at once; LDS elements between the dw components of the staged amplitudes
  int32_t ngu;            // up groups of the class
  int32_t rows_off;       // into rows: [ngu][du] device row | sign << 31
  int32_t cols_off;       // into cols: [local dw groups][dd] column slot | sign << 31
  int32_t tile_off;       // into tiles: ti | tj << 16
  int32_t nrep;           // partial blocks an item writes.  4: tile kernel, the block's tiles fit one wave, so each of the four waves takes every
                          // fourth pair of a batch and writes a block of its own; 1: pair kernel, or the tiles are spread over the workgroup
};
struct PtItem {
  int32_t cls, p0, p1, pad;  // pairs [p0, p1) of the class, pair = (local dw group) * ngu + (up group)
  int64_t out_off;           // its partial block(s) in the partial buffer (elements)
};
struct PtClassHost {
  int64_t out_off = 0;           // the class block in the reduced output (elements), ntiles*t*t of them
  int32_t ngd = 0;               // this rank's dw groups of the class
  std::vector<uint32_t> au, ad;  // kept-part configurations (compressed to nsub bits) of the block's up / dw components
  std::vector<uint32_t> tiles;
};
// the host image of the tables
struct PtHostTables {
  int nsub = 0;             // kept orbitals: the dense matrix is 4^nsub x 4^nsub
  std::vector<PtClass> cls;
  std::vector<PtClassHost> hcls;
  int nitems[3] = {0, 0, 0};  // items of the pair kernel, of the 2 x 2 tile classes, of the 4 x 4 tile classes: the work list in that order
  int64_t partial_elems = 0, out_elems = 0;
  std::vector<PtItem> items;
  std::vector<uint32_t> rows, cols, tiles;
  std::vector<int64_t> el_src;  // per output element: its first partial, how many there are, the distance between them
  std::vector<int32_t> el_cnt, el_stride;
};

inline int64_t binom(int n, int k) {
  if (k < 0 || k > n) return 0;
  k = std::min(k, n - k);
  int64_t r = 1;
  for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;
  return r;
}

// owner of a dw column and its slot in the gathered copy (the padded all-gather layout: rank o's columns from slot o*cmax on)
struct DwSlots {
  int cmax;
  std::vector<int32_t> rfirst;  // [nranks + 1] first column of each rank
  DwSlots(int dimdw, int nranks, int cmax_) : cmax(cmax_), rfirst(nranks + 1, dimdw) {
    for (int p = 0, q; p < nranks; ++p) dw_split(dimdw, p, nranks, q, rfirst[p]);
  }
  int owner(int c) const { return (int)(std::upper_bound(rfirst.begin(), rfirst.end(), c) - rfirst.begin()) - 1; }
  uint32_t slot(int c) const {
    if (rfirst.size() == 2) return (uint32_t)c;
    const int o = owner(c);
    return (uint32_t)(o * cmax + (c - rfirst[o]));
  }
};

// what pt_build reads of the sector (SectorHost's members of the same names) beside the groups
struct PtSector {
  int nsub, nup, ndw;  // kept orbitals; particles per spin
  int dimup;
  int dimdw, nranks, cmax, qdw, dw0;  // the dw columns and their split: this rank owns [dw0, dw0 + qdw)
};
// The ordered groups of one spin: [k] = the groups whose traced part holds k particles, flattened [ngroups][d], d = C(nsub, n_spin - k), each
// entry (device row, or column of the sector) | sign << 31, the members of a group by ascending kept configuration.  Every group of the WHOLE
// sector is listed on every rank; a dw group belongs to the rank that owns the column of its first entry.
using PtGroups = std::vector<std::vector<uint32_t>>;

// small_n: classes with n <= small_n (at most PT_PAIR_N) go to the pair kernel, the others to the tile kernel; ncu: compute units the work
// list is cut for; name: the head of the error text.  Calls nothing of the HIP runtime.
inline std::string pt_build(const PtSector& s, const PtGroups& up, const PtGroups& dw, int small_n, int ncu, const std::string& name,
                            PtHostTables& t) {
  t = PtHostTables();
  t.nsub = s.nsub;
  const int kmax = (int)up.size() - 1;  // traced particle numbers 0 .. kmax
  const DwSlots slots(s.dimdw, s.nranks, s.cmax);
  // per traced particle number: the up groups' rows, this rank's dw groups' column slots
  std::vector<int32_t> ungrp(kmax + 1, 0), dngrp(kmax + 1, 0), dngrp_all(kmax + 1, 0), rows_off(kmax + 1, 0), cols_off(kmax + 1, 0);
  for (int k = 0; k <= kmax; ++k) {
    const int du = (int)binom(s.nsub, s.nup - k), dd = (int)binom(s.nsub, s.ndw - k);
    rows_off[k] = (int32_t)t.rows.size();
    t.rows.insert(t.rows.end(), up[k].begin(), up[k].end());
    ungrp[k] = du ? (int32_t)(up[k].size() / du) : 0;
    cols_off[k] = (int32_t)t.cols.size();
    dngrp_all[k] = dd ? (int32_t)(dw[k].size() / dd) : 0;
    for (int g = 0; g < dngrp_all[k]; ++g) {
      const uint32_t* e = dw[k].data() + (size_t)g * dd;
      const int first = (int)(e[0] & 0x7fffffffu);
      if (first < s.dw0 || first >= s.dw0 + s.qdw) continue;
      for (int i = 0; i < dd; ++i) t.cols.push_back(slots.slot((int)(e[i] & 0x7fffffffu)) | (e[i] & 0x80000000u));
      ++dngrp[k];
    }
  }
  // classes: every (up, dw) traced particle number pair of the WHOLE sector, the same list on every rank; the pair kernel's classes first, then
  // the tile kernel's by tile edge
  for (int pass = 0; pass < 3; ++pass)
    for (int ku = 0; ku <= kmax; ++ku)
      for (int kd = 0; kd <= kmax; ++kd) {
        if (!ungrp[ku] || !dngrp_all[kd]) continue;
        PtClass c{};
        c.du = (int32_t)binom(s.nsub, s.nup - ku);
        c.dd = (int32_t)binom(s.nsub, s.ndw - kd);
        c.n = c.du * c.dd;
        const bool small = c.n <= small_n;
        const int nt2 = (c.n + 1) / 2;
        c.t = nt2 * (nt2 + 1) / 2 <= PT_THREADS ? 2 : 4;  // 2 x 2 tiles while the upper triangle fits one tile per thread
        if (pass != (small ? 0 : c.t == 2 ? 1 : 2)) continue;
        c.nt = (c.n + c.t - 1) / c.t;
        c.ntiles = c.nt * (c.nt + 1) / 2;
        if (c.ntiles > (c.t == 2 ? 1 : 2) * PT_THREADS) return name + ": a class block exceeds the register tiles";
        c.nrep = (!small && c.ntiles <= 64) ? PT_THREADS / 64 : 1;
        // LDS of the tile kernel: component (iu, id) of pair b of the batch at id*stride + b*du + iu, stride = du (mod 16) so that the
        // components of one pair fall on consecutive 16-byte bank slots
        for (c.batch = PT_XS / c.n; c.batch >= 1; --c.batch) {
          c.stride = c.batch * c.du;
          while (c.stride % 16 != c.du % 16) ++c.stride;
          if ((int64_t)c.dd * c.stride <= PT_XS) break;
        }
        if (c.batch < 1) return name + ": a class block exceeds the staging area";
        c.ngu = ungrp[ku];
        c.rows_off = rows_off[ku];
        c.cols_off = cols_off[kd];
        c.tile_off = (int32_t)t.tiles.size();
        PtClassHost h;
        for (int tj = 0; tj < c.nt; ++tj)
          for (int ti = 0; ti <= tj; ++ti) h.tiles.push_back((uint32_t)ti | ((uint32_t)tj << 16));
        t.tiles.insert(t.tiles.end(), h.tiles.begin(), h.tiles.end());
        for (uint32_t a = 0; a < (1u << s.nsub); ++a) {
          if (__builtin_popcount(a) == s.nup - ku) h.au.push_back(a);
          if (__builtin_popcount(a) == s.ndw - kd) h.ad.push_back(a);
        }
        h.ngd = dngrp[kd];
        h.out_off = t.out_elems;
        t.out_elems += (int64_t)c.ntiles * c.t * c.t;
        t.cls.push_back(c);
        t.hcls.push_back(h);
      }
  // work list: each class's pairs cut into slices of about (local amplitudes) / (PT_WG_PER_CU * compute units) amplitudes; the pair kernel
  // takes a workgroup's width of pairs at least, a pair of the tile kernel counts for at least PT_PAIR_COST / nrep amplitudes
  const int64_t local = (int64_t)s.dimup * std::max(s.qdw, 0);
  const int64_t chunk = std::max<int64_t>(1, local / std::max(1, PT_WG_PER_CU * ncu));
  for (size_t ci = 0; ci < t.cls.size(); ++ci) {
    const PtClass& c = t.cls[ci];
    const bool small = c.n <= small_n;
    const int64_t npairs = (int64_t)c.ngu * t.hcls[ci].ngd;
    const int64_t sz = (int64_t)c.ntiles * c.t * c.t;  // (an item of the class holds nrep partial blocks in a row)
    if (npairs >= INT32_MAX - PT_THREADS) return name + ": too many pairs";
    const int64_t per = small ? std::max<int64_t>(PT_THREADS, chunk / c.n) : std::max<int64_t>(1, chunk / std::max(c.n, PT_PAIR_COST / c.nrep));
    const int64_t first_off = t.partial_elems;
    int32_t nparts = 0;
    for (int64_t p = 0; p < npairs; p += per, ++nparts) {
      PtItem it{};
      it.cls = (int32_t)ci;
      it.p0 = (int32_t)p;
      it.p1 = (int32_t)std::min(npairs, p + per);
      it.out_off = t.partial_elems;
      t.partial_elems += sz * c.nrep;
      t.items.push_back(it);
    }
    t.nitems[small ? 0 : c.t == 2 ? 1 : 2] += nparts;
    for (int64_t e = 0; e < sz; ++e) {
      t.el_src.push_back(first_off + e);
      t.el_cnt.push_back(nparts * c.nrep);
      t.el_stride.push_back((int32_t)sz);
    }
  }
  if (t.items.size() >= (size_t)INT32_MAX) return name + ": too many work items";
  return std::string();
}

// the group enumerations of the two front ends (hxv_partial_trace_groups.cpp); "" or the error text
std::string cluster_dm_groups(const SectorHost& s, int nimp, PtGroups& up, PtGroups& dw);
std::string reduced_dm_groups(const SectorHost& s, uint32_t S, int fermi_sign, PtGroups& up, PtGroups& dw);

// the engine (hxv_partial_trace.hip)
struct PtTables;
// builds the tables of the handle's sector from its groups and uploads them; name: the matrix's ("cluster density matrix"), the head of the
// error text.  HXV_OK, or the failure as recorded
int pt_make_tables(const hxv_handle* h, int nsub, const PtGroups& up, const PtGroups& dw, int small_n, const char* name, std::shared_ptr<PtTables>& out);
// out = the tables of (family, key) kept with the handle's sector image (TableStore, hxv_handle.hpp), the family's `cap` most recently used;
// `build` makes them when they are not there.  HXV_OK, or what build returned: then nothing is stored and out stays null
int pt_stored_tables(hxv_handle* h, const char* family, const std::string& key, size_t cap, std::shared_ptr<PtTables>& out,
                     const std::function<int(std::shared_ptr<PtTables>&)>& build);
// out (+)= weight * rho of the device vector d_psi.  t: the tables, null where this rank could not make them and rc_local says why: every
// rank of a split sector learns of it and returns.  what: the entry point's name, for the error text
int pt_accumulate(hxv_handle* h, const std::shared_ptr<PtTables>& t, int rc_local, const void* d_psi, double weight, bool accumulate, double* out,
                  const char* what);
}  // namespace hxv
