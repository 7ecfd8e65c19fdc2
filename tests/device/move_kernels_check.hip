// TEST-ONLY: one launcher per kernel that only MOVES amplitudes between layouts -- the twin map (csrc/hxv_twin_kernels.hpp), the ladder
// operators (csrc/hxv_ladder_kernels.hpp), the column packer and the piecewise add of the slab exchanges (csrc/hxv_move_kernels.hpp) and the
// two row-order kernels (csrc/hxv_rows_kernels.hpp) -- so that tests/test_gpu_move_kernels.py can run each alone, on tables and grids no
// sector passes.  The kernels are the headers' text, compiled with the engine's flags (build_move_kernels_check() of __graft_entry__.py);
// this library is never linked into libhxv.so.
//
// Every entry takes device pointers and the GRID (gridDim.x, and gridDim.y where the kernel has one), launches on the null stream with the
// kernel's own block size, waits, and returns the HIP status.  Before launching, every entry refuses (hipErrorInvalidValue) what could make
// the kernel reach outside what it was given whatever the tables hold: a dimension below 1, a pitch or stride below its dimension or not a
// multiple of 8, an empty or oversized grid, a NULL the kernel would dereference.  Where blockIdx itself is an index without a guard
// (pack_columns_kernel's x) the grid IS the column count.  Table CONTENTS are not checked here:
// tests/test_move_kernels_ref_cpu.py does that for every case the GPU file runs.
#include "hxv_ladder_kernels.hpp"
#include "hxv_move_kernels.hpp"
#include "hxv_rows_kernels.hpp"
#include "hxv_twin_kernels.hpp"

#include <vector>

namespace {
int finish() {
  hipError_t e = hipGetLastError();
  hipError_t s = hipStreamSynchronize(nullptr);
  return (int)(e != hipSuccess ? e : s);
}
constexpr int BAD = (int)hipErrorInvalidValue;
bool bad_grid(int g) { return g < 1 || g > 65535; }
bool bad_pitch(int pitch, int dim) { return dim < 1 || pitch < dim || pitch % 8 != 0; }
}  // namespace

extern "C" {

int mkc_tw() { return TW; }
int mkc_tw_threads() { return TW_THREADS; }

// d_a: [dimup_b columns][pitch_a], d_b: [dimup_a columns][pitch_b]; the row-order tables may be NULL (reference order)
int mkc_twin_transpose(int gx, int gy, const void* d_a, int dimup_a, int pitch_a, const int32_t* iperm_a, const uint8_t* sign_a, void* d_b, int dimup_b,
                       int pitch_b, const int32_t* iperm_b, const uint8_t* sign_b) {
  if (bad_grid(gx) || bad_grid(gy) || bad_pitch(pitch_a, dimup_a) || bad_pitch(pitch_b, dimup_b) || !d_a || !d_b) return BAD;
  hipLaunchKernelGGL(twin_transpose_kernel, dim3(gx, gy), dim3(TW_THREADS), 0, nullptr, (const double2*)d_a, dimup_a, pitch_a, iperm_a, sign_a,
                     (double2*)d_b, dimup_b, pitch_b, iperm_b, sign_b);
  return finish();
}

// d_a: [qa columns][pitch_a], send: [dimup_a rows][stride], own: [own_hi - own_lo rows][stride] (may be NULL when the own range is empty)
int mkc_twin_pack(int gx, int gy, const void* d_a, int dimup_a, int pitch_a, int qa, const int32_t* iperm_a, const uint8_t* sign_a, void* send, void* own,
                  int stride, int own_lo, int own_hi) {
  if (bad_grid(gx) || bad_grid(gy) || bad_pitch(pitch_a, dimup_a) || bad_pitch(stride, qa) || !d_a || !send || own_lo < 0 || own_hi < own_lo ||
      own_hi > dimup_a || (own_hi > own_lo && !own))
    return BAD;
  hipLaunchKernelGGL(twin_pack_kernel, dim3(gx, gy), dim3(TW_THREADS), 0, nullptr, (const double2*)d_a, dimup_a, pitch_a, qa, iperm_a, sign_a,
                     (double2*)send, (double2*)own, stride, own_lo, own_hi);
  return finish();
}

// tab (device): [nranks+1] first column of A per rank, [nranks+1] element offset of each rank's block in recv, [nranks] its row stride
int mkc_twin_unpack(int gx, int gy, const void* recv, const int64_t* tab, int nranks, void* d_b, int dimup_b, int pitch_b, int qb, const int32_t* iperm_b,
                    const uint8_t* sign_b) {
  if (bad_grid(gx) || bad_grid(gy) || bad_pitch(pitch_b, dimup_b) || nranks < 1 || qb < 1 || !recv || !tab || !d_b) return BAD;
  hipLaunchKernelGGL(twin_unpack_kernel, dim3(gx, gy), dim3(TW_THREADS), 0, nullptr, (const double2*)recv, tab, nranks, (double2*)d_b, dimup_b, pitch_b,
                     qb, iperm_b, sign_b);
  return finish();
}

// spin 0: map_to [dimup_to], psi [dimdw_to columns][pitch_from] with dim_from rows; spin 1: map_to [dimdw_to], psi [dim_from columns][pitch_from]
// with dimup_to rows.  out: [dimdw_to columns][pitch_to].  perm_from, sign_from, sign_to may be NULL.
int mkc_ladder(int gx, const uint32_t* map_from, int dim_from, const uint32_t* map_to, int pitch_from, int dimup_to, int pitch_to, int dimdw_to,
               int orbital, int spin, int create, const void* psi, void* out, double coef_re, double coef_im, int accumulate,
               const int32_t* perm_from, const uint8_t* sign_from, const uint8_t* sign_to) {
  if (bad_grid(gx) || dim_from < 1 || dimdw_to < 1 || bad_pitch(pitch_to, dimup_to) || spin < 0 || spin > 1 ||
      bad_pitch(pitch_from, spin == 0 ? dim_from : dimup_to) || orbital < 0 || orbital > 31 || !map_from || !map_to || !psi || !out)
    return BAD;
  hipLaunchKernelGGL(ladder_kernel, dim3(gx), dim3(256), 0, nullptr, map_from, dim_from, map_to, pitch_from, dimup_to, pitch_to, dimdw_to, orbital,
                     spin, create, (const double2*)psi, (double2*)out, make_double2(coef_re, coef_im), accumulate, perm_from, sign_from, sign_to);
  return finish();
}

// slot, sign: [ncols]; psi_local, recv: columns of pitch_from elements; out: [ncols columns][pitch_to].  One workgroup per column: the
// blocks past ncols return at once.
int mkc_ladder_cols(int gx, int dimup, int ncols, int pitch_from, int pitch_to, const int32_t* slot, const int32_t* sign, const void* psi_local,
                    const void* recv, void* out, double coef_re, double coef_im, int accumulate) {
  if (bad_grid(gx) || ncols < 1 || bad_pitch(pitch_from, dimup) || bad_pitch(pitch_to, dimup) || !slot || !sign || !psi_local || !recv || !out) return BAD;
  hipLaunchKernelGGL(ladder_cols_kernel, dim3(gx), dim3(256), 0, nullptr, dimup, ncols, pitch_from, pitch_to, slot, sign, (const double2*)psi_local,
                     (const double2*)recv, (double2*)out, make_double2(coef_re, coef_im), accumulate);
  return finish();
}

// cols: [ncols]; the grid is ncols (blockIdx.x indexes cols without a guard)
int mkc_pack_columns(int ncols, const void* in, void* out, const int32_t* cols, int pitch) {
  if (bad_grid(ncols) || bad_pitch(pitch, 1) || !in || !out || !cols) return BAD;
  hipLaunchKernelGGL(hxv::pack_columns_kernel, dim3(ncols), dim3(256), 0, nullptr, (const double2*)in, (double2*)out, cols, pitch);
  return finish();
}

// row0, row1, stride, base: HOST arrays of nwtr entries (base: device pointers), made into the WtRange table here; the gy blocks along y
// loop over the ncols columns (ncols may exceed what a grid holds along y).  real: add_pieces_kernel<double>, otherwise <double2>.
int mkc_add_pieces(int gx, int gy, int ncols, int real, void* hv, int nwtr, const int32_t* row0, const int32_t* row1, const int64_t* stride,
                   const void* const* base, int dimup, int pitch) {
  if (bad_grid(gx) || bad_grid(gy) || ncols < 1 || nwtr < 1 || bad_pitch(pitch, dimup) || !hv || !row0 || !row1 || !stride || !base) return BAD;
  std::vector<hxv::WtRange> tab(nwtr);
  for (int k = 0; k < nwtr; ++k) {
    if (!base[k] || stride[k] < 0) return BAD;
    tab[k] = hxv::WtRange{row0[k], row1[k], stride[k], base[k]};
  }
  hxv::WtRange* d_tab = nullptr;
  hipError_t e = hipMalloc((void**)&d_tab, nwtr * sizeof(hxv::WtRange));
  if (e != hipSuccess) return (int)e;
  e = hipMemcpy(d_tab, tab.data(), nwtr * sizeof(hxv::WtRange), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d_tab);
    return (int)e;
  }
  const dim3 grid(gx, gy);
  if (real)
    hipLaunchKernelGGL(hxv::add_pieces_kernel<double>, grid, dim3(256), 0, nullptr, (double*)hv, d_tab, nwtr, dimup, pitch, ncols);
  else
    hipLaunchKernelGGL(hxv::add_pieces_kernel<double2>, grid, dim3(256), 0, nullptr, (double2*)hv, d_tab, nwtr, dimup, pitch, ncols);
  const int rc = finish();
  (void)hipFree(d_tab);
  return rc;
}

// src: [ncols][dimup] contiguous, dst: [ncols][pitch]; n = pitch * ncols
int mkc_rows_ref_to_dev(int gx, const void* src, void* dst, const int32_t* iperm, const uint8_t* sign, int dimup, int pitch, int ncols) {
  if (bad_grid(gx) || bad_pitch(pitch, dimup) || ncols < 1 || !src || !dst || !iperm || !sign) return BAD;
  hipLaunchKernelGGL(hxv::rows_ref_to_dev, dim3(gx), dim3(256), 0, nullptr, (const double2*)src, (double2*)dst, iperm, sign, dimup, pitch,
                     (int64_t)pitch * ncols);
  return finish();
}

// src: [ncols][pitch], dst: [ncols][dimup] contiguous; n = dimup * ncols
int mkc_rows_dev_to_ref(int gx, const void* src, void* dst, const int32_t* perm, const uint8_t* sign, int dimup, int pitch, int ncols) {
  if (bad_grid(gx) || bad_pitch(pitch, dimup) || ncols < 1 || !src || !dst || !perm || !sign) return BAD;
  hipLaunchKernelGGL(hxv::rows_dev_to_ref, dim3(gx), dim3(256), 0, nullptr, (const double2*)src, (double2*)dst, perm, sign, dimup, pitch,
                     (int64_t)dimup * ncols);
  return finish();
}

}  // extern "C"
