// TEST-ONLY: one launcher per kernel of the non-local block spH0nd (csrc/hxv_nonlocal_kernels.hpp: hxv_nonlocal_kernel, hxv_nonlocal_tab,
// hxv_nonlocal_csr), so that tests/test_gpu_nonlocal_kernels.py can run each alone, on tables, slabs and grids no sector passes.  The
// kernels are the header's text, compiled with the engine's flags (build_nonlocal_kernels_check() of __graft_entry__.py); this library is
// never linked into libhxv.so.
//
// Every entry takes device pointers for the DevSector fields its kernel reads, the scalars, and the GRID, fills a DevSector (everything else
// zero), launches on the null stream with the kernel's own block size, waits, and returns the HIP status.  hxv_nonlocal_tab takes rchunks
// instead of a grid: blockIdx.x is an index there without a guard, so its grid IS qdw * rchunks.  Before launching, every entry refuses
// (hipErrorInvalidValue) what could make the kernel reach outside what it was given whatever the tables hold: a dimension below 1, a pitch
// below DimUp or not a multiple of 8, a slab outside the dw dimension, fewer than DimUp rows in a column's chunks, an empty or oversized
// grid, a NULL the kernel would dereference, more orbitals than a 32-bit configuration has bits.  Table CONTENTS are not checked here:
// tests/test_nonlocal_kernels_ref_cpu.py does that for every case the GPU file runs.
#include "hxv_nonlocal_kernels.hpp"

namespace {
int finish() {
  hipError_t e = hipGetLastError();
  hipError_t s = hipStreamSynchronize(nullptr);
  return (int)(e != hipSuccess ? e : s);
}
constexpr int BAD = (int)hipErrorInvalidValue;
bool bad_grid(int64_t g) { return g < 1 || g > 65535; }
bool bad_shape(int dimup, int dimdw, int pitch, int qdw, int dw0) {
  return dimup < 1 || dimdw < 1 || qdw < 1 || pitch < dimup || pitch % 8 != 0 || dw0 < 0 || (int64_t)dw0 + qdw > dimdw;
}
// the orbitals of the impurity sites are bits 0 .. nlat*norb - 1 of a 32-bit configuration; NonLocalParams is built for norb <= 5
bool bad_orbitals(int nlat, int norb) { return nlat < 1 || norb < 1 || norb > 5 || nlat > 16 || nlat * norb > 32; }

hxv::DevSector sector(int dimup, int dimdw, int pitch, int qdw, int dw0) {
  hxv::DevSector s{};
  s.dimup = dimup;
  s.dimdw = dimdw;
  s.pitch = pitch;
  s.qdw = qdw;
  s.dw0 = dw0;
  return s;
}
void coupling(hxv::DevSector& s, int nlat, int norb, double jx, double jp) {
  s.nd.active = 1;
  s.nd.nlat = nlat;
  s.nd.norb = norb;
  s.nd.jx = jx;
  s.nd.jp = jp;
}
}  // namespace

extern "C" {

// v: column slots of pitch elements, hv: [qdw columns][pitch]; map_up: [dimup], map_dw: [dimdw] sorted configurations; vcol: [dimdw]
int nkc_nonlocal_kernel(int gx, const void* v, void* hv, const uint32_t* map_up, const uint32_t* map_dw, const uint32_t* vcol, int dimup, int dimdw,
                        int pitch, int qdw, int dw0, int nlat, int norb, double jx, double jp) {
  if (bad_grid(gx) || bad_shape(dimup, dimdw, pitch, qdw, dw0) || bad_orbitals(nlat, norb) || !v || !hv || !map_up || !map_dw || !vcol) return BAD;
  hxv::DevSector s = sector(dimup, dimdw, pitch, qdw, dw0);
  coupling(s, nlat, norb, jx, jp);
  s.diag.map_up = map_up;
  s.diag.map_dw = map_dw;
  s.vcol = vcol;
  hipLaunchKernelGGL(hxv::hxv_nonlocal_kernel, dim3(gx), dim3(256), 0, nullptr, s, (const double2*)v, (double2*)hv);
  return finish();
}

// nd_up: [nlat*norb*norb][dimup], nd_dw: [nlat*norb*norb][dimdw]; the grid is qdw * rchunks
int nkc_nonlocal_tab(int rchunks, const void* v, void* hv, const uint32_t* nd_up, const uint32_t* nd_dw, int dimup, int dimdw, int pitch, int qdw, int dw0,
                     int nlat, int norb, double jx, double jp) {
  if (bad_shape(dimup, dimdw, pitch, qdw, dw0) || bad_orbitals(nlat, norb) || rchunks < 1 || (int64_t)rchunks * 1024 < dimup ||
      bad_grid((int64_t)qdw * rchunks) || !v || !hv || !nd_up || !nd_dw)
    return BAD;
  hxv::DevSector s = sector(dimup, dimdw, pitch, qdw, dw0);
  coupling(s, nlat, norb, jx, jp);
  s.nd_up = nd_up;
  s.nd_dw = nd_dw;
  hipLaunchKernelGGL(hxv::hxv_nonlocal_tab, dim3(qdw * rchunks), dim3(1024), 0, nullptr, s, (const double2*)v, (double2*)hv, rchunks);
  return finish();
}

// rowptr: [qdw*dimup + 1] over the local rows, cols: 1-based global columns, vals: complex; vcol: [dimdw]
int nkc_nonlocal_csr(int gx, const void* v, void* hv, const int64_t* rowptr, const int32_t* cols, const void* vals, const uint32_t* vcol, int dimup,
                     int dimdw, int pitch, int qdw, int dw0) {
  if (bad_grid(gx) || bad_shape(dimup, dimdw, pitch, qdw, dw0) || !v || !hv || !rowptr || !cols || !vals || !vcol) return BAD;
  hxv::DevSector s = sector(dimup, dimdw, pitch, qdw, dw0);
  s.nd.active = 1;
  s.vcol = vcol;
  s.ndcsr_rowptr = rowptr;
  s.ndcsr_cols = cols;
  s.ndcsr_vals = (const double2*)vals;
  hipLaunchKernelGGL(hxv::hxv_nonlocal_csr, dim3(gx), dim3(256), 0, nullptr, s, (const double2*)v, (double2*)hv);
  return finish();
}

}  // extern "C"
