// TEST-ONLY: pt_build of csrc/hxv_partial_trace_host.hpp behind extern "C" entries, on a SYNTHETIC sector: a PtSector and two PtGroups given
// as flat arrays, with small_n and ncu as arguments.  pt_build does not ask where the groups come from, so any class shape and any work-list
// cut can be reached at a few thousand amplitudes.  Every host table is handed back as it is.  Included by
//   tests/host/partial_trace_build.cpp            a host-only shared object (no HIP): tests/test_partial_trace_kernels_ref_cpu.py
//   tests/device/partial_trace_kernels_check.hip  the launcher library, which uploads the tables and runs the kernels on them
// Both export the same ptb_* entries; tests/partial_trace_kernels_ref.py reads either.
#pragma once

#include <cstring>

#include "hxv_partial_trace_host.hpp"

namespace ptb {
constexpr uint64_t MAGIC = 0x7074625f74626c73ull;  // what a table handle starts with
struct Tables {
  uint64_t magic = MAGIC;
  hxv::PtHostTables t;
  void* device = nullptr;  // the launcher library's upload, null in the host-only build
  void (*release)(void*) = nullptr;
};
inline Tables* tables_of(void* h) {
  Tables* p = (Tables*)h;
  return p && p->magic == MAGIC ? p : nullptr;
}
template <class T>
void copy_out(const std::vector<T>& v, void* dst) {
  if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(T));
}
}  // namespace ptb

extern "C" {

// sector[9] = nsub, nup, ndw, dimup, dimdw, nranks, cmax, qdw, dw0.  up / dw: the entries of [0], [1], ... [nk - 1] in a row, len[k] of them.
// Returns the handle, or null with pt_build's error text in err.
void* ptb_build(const int32_t* sector, int nk, const uint32_t* up, const int64_t* up_len, const uint32_t* dw, const int64_t* dw_len, int small_n,
                int ncu, char* err, int errlen) {
  if (err && errlen > 0) err[0] = 0;
  if (!sector || nk < 1 || !up || !up_len || !dw || !dw_len) return nullptr;
  hxv::PtGroups gu((size_t)nk), gd((size_t)nk);
  for (int k = 0; k < nk; ++k) {
    if (up_len[k] < 0 || dw_len[k] < 0) return nullptr;
    gu[k].assign(up, up + up_len[k]);
    gd[k].assign(dw, dw + dw_len[k]);
    up += up_len[k];
    dw += dw_len[k];
  }
  auto* p = new ptb::Tables();
  const hxv::PtSector s{sector[0], sector[1], sector[2], sector[3], sector[4], sector[5], sector[6], sector[7], sector[8]};
  const std::string e = hxv::pt_build(s, gu, gd, small_n, ncu, "synthetic sector", p->t);
  if (!e.empty()) {
    if (err && errlen > 0) {
      std::strncpy(err, e.c_str(), (size_t)errlen - 1);
      err[errlen - 1] = 0;
    }
    delete p;
    return nullptr;
  }
  return p;
}

void ptb_free(void* h) {
  ptb::Tables* p = ptb::tables_of(h);
  if (!p) return;
  if (p->device && p->release) p->release(p->device);
  p->magic = 0;
  delete p;
}

// out[11] = classes, items, rows, cols, tiles, out_elems, partial_elems, nitems[0..2], sizeof(PtClass) | sizeof(PtItem) << 32
int ptb_sizes(void* h, int64_t* out) {
  ptb::Tables* p = ptb::tables_of(h);
  if (!p || !out) return 1;
  const hxv::PtHostTables& t = p->t;
  out[0] = (int64_t)t.cls.size();
  out[1] = (int64_t)t.items.size();
  out[2] = (int64_t)t.rows.size();
  out[3] = (int64_t)t.cols.size();
  out[4] = (int64_t)t.tiles.size();
  out[5] = t.out_elems;
  out[6] = t.partial_elems;
  for (int i = 0; i < 3; ++i) out[7 + i] = t.nitems[i];
  out[10] = (int64_t)sizeof(hxv::PtClass) | ((int64_t)sizeof(hxv::PtItem) << 32);
  return 0;
}

// every table into the caller's arrays (sized by ptb_sizes; el_* hold out_elems entries, cls_out_off and cls_ngd one per class)
int ptb_copy(void* h, void* cls, void* items, uint32_t* rows, uint32_t* cols, uint32_t* tiles, int64_t* el_src, int32_t* el_cnt,
             int32_t* el_stride, int64_t* cls_out_off, int32_t* cls_ngd) {
  ptb::Tables* p = ptb::tables_of(h);
  if (!p) return 1;
  const hxv::PtHostTables& t = p->t;
  ptb::copy_out(t.cls, cls);
  ptb::copy_out(t.items, items);
  ptb::copy_out(t.rows, rows);
  ptb::copy_out(t.cols, cols);
  ptb::copy_out(t.tiles, tiles);
  ptb::copy_out(t.el_src, el_src);
  ptb::copy_out(t.el_cnt, el_cnt);
  ptb::copy_out(t.el_stride, el_stride);
  for (size_t c = 0; c < t.hcls.size(); ++c) {
    if (cls_out_off) cls_out_off[c] = t.hcls[c].out_off;
    if (cls_ngd) cls_ngd[c] = t.hcls[c].ngd;
  }
  return 0;
}

// the kept-part configurations of class c's components (du and dd entries)
int ptb_class_configs(void* h, int c, uint32_t* au, uint32_t* ad) {
  ptb::Tables* p = ptb::tables_of(h);
  if (!p || c < 0 || c >= (int)p->t.hcls.size() || !au || !ad) return 1;
  ptb::copy_out(p->t.hcls[(size_t)c].au, au);
  ptb::copy_out(p->t.hcls[(size_t)c].ad, ad);
  return 0;
}

}  // extern "C"
