// The three kernels that apply the non-local block spH0nd (hxv_kernels.hip): text moved out of that file unchanged, so that
// tests/device/nonlocal_kernels_check.hip can launch each alone on tables, slabs and grids of its own making
// (tests/test_gpu_nonlocal_kernels.py).  launch_hxv_nonlocal, which chooses among them, has external linkage (hxv_internal.hpp) and stays
// in hxv_kernels.hip.  rank_in_map, par_below and cfma stay in hxv_device.hpp: the ladder and the product kernels use them too.
#pragma once

#include <hip/hip_runtime.h>

#include "hxv_device.hpp"

namespace hxv {

// ---------------------------------------------------------------------------------------
// Non-local block spH0nd (spin exchange Jx, pair hopping Jp; Norb>1 only), on the fly:
//   hv(i) += sum_j H_nd(i,j) v(j),   j = state reached from i by the two-spin operator
// exactly the (symmetric, "transposed") rows the reference stores at sparse/H_non_local.f90:4-100 and
// multiplies at ED_HAMILTONIAN_SPARSE_HxV.f90:217-225 / :300-313 (there on the all-gathered vector).
// Signs are the product of the four single-spin signs (c/cdg, ED_SETUP.f90:807-833), no cross-spin sign.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) hxv_nonlocal_kernel(DevSector s, const double2* __restrict__ v, double2* __restrict__ hv) {
  const int64_t nloc = (int64_t)s.qdw * s.dimup;
  const uint32_t* __restrict__ map_up = s.diag.map_up;
  const uint32_t* __restrict__ map_dw = s.diag.map_dw;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nloc; t += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(t / s.dimup);
    const int i = (int)(t - (int64_t)cl * s.dimup);
    const uint32_t mu = map_up[i], md = map_dw[cl + s.dw0];
    double2 acc = make_double2(0.0, 0.0);
    bool any = false;
    for (int il = 0; il < s.nd.nlat; ++il)
      for (int io = 0; io < s.nd.norb; ++io)
        for (int jo = 0; jo < s.nd.norb; ++jo) {
          if (io == jo) continue;
          const int is = io + il * s.nd.norb, js = jo + il * s.nd.norb;  // imp_state_index, 0-based bit
          const bool nu_i = (mu >> is) & 1u, nu_j = (mu >> js) & 1u, nd_i = (md >> is) & 1u, nd_j = (md >> js) & 1u;
          // spin exchange, H_non_local.f90:26-60:  [c^+_js c_is]_dw [c^+_is c_js]_up
          if (s.nd.jx != 0.0 && nu_j && nd_i && !nd_j && !nu_i) {
            const uint32_t k1 = md & ~(1u << is), k2 = k1 | (1u << js);
            const uint32_t k3 = mu & ~(1u << js), k4 = k3 | (1u << is);
            const int sg = par_below(md, is) ^ par_below(k1, js) ^ par_below(mu, js) ^ par_below(k3, is);
            const int jdw = rank_in_map(map_dw, s.dimdw, k2), jup = rank_in_map(map_up, s.dimup, k4);
            const double2 x = v[(int64_t)s.vcol[jdw] * s.pitch + jup];
            const double c = sg ? -s.nd.jx : s.nd.jx;
            acc.x += c * x.x;
            acc.y += c * x.y;
            any = true;
          }
          // pair hopping, H_non_local.f90:65-98:  [c^+_is c_js]_dw [c^+_is c_js]_up
          if (s.nd.jp != 0.0 && nu_j && nd_j && !nd_i && !nu_i) {
            const uint32_t k1 = md & ~(1u << js), k2 = k1 | (1u << is);
            const uint32_t k3 = mu & ~(1u << js), k4 = k3 | (1u << is);
            const int sg = par_below(md, js) ^ par_below(k1, is) ^ par_below(mu, js) ^ par_below(k3, is);
            const int jdw = rank_in_map(map_dw, s.dimdw, k2), jup = rank_in_map(map_up, s.dimup, k4);
            const double2 x = v[(int64_t)s.vcol[jdw] * s.pitch + jup];
            const double c = sg ? -s.nd.jp : s.nd.jp;
            acc.x += c * x.x;
            acc.y += c * x.y;
            any = true;
          }
        }
    if (any) {
      const int64_t o = (int64_t)cl * s.pitch + i;
      double2 h = hv[o];
      h.x += acc.x;
      h.y += acc.y;
      hv[o] = h;
    }
  }
}

// Same block from the one-spin move tables (SectorHost::nd_up / nd_dw): spH0nd = sum over sites and orbital pairs of
//   Jx [c^+_j c_i]_dw [c^+_i c_j]_up + Jp [c^+_i c_j]_dw [c^+_i c_j]_up,   Kronecker products of two one-body moves,
// so an element's partner is (up-move of the row) x (dw-move of the column).  One workgroup per (column, 1024 rows): the
// dw moves of the column are wave-uniform (no work at all for the terms the column's dw state rules out), the up moves
// come from a coalesced table row, the partner values from ONE other column with rows in increasing order.  No search.
__global__ void __launch_bounds__(1024) hxv_nonlocal_tab(DevSector s, const double2* __restrict__ v, double2* __restrict__ hv, int rchunks) {
  const int cl = blockIdx.x / rchunks;                      // local column
  const int i = (blockIdx.x - cl * rchunks) * 1024 + threadIdx.x;
  const bool row_ok = i < s.dimup;
  const int ir = min(i, s.dimup - 1);
  const int c = cl + s.dw0;
  const int O = s.nd.norb;
  double2 acc = make_double2(0.0, 0.0);
  bool any = false;
  for (int il = 0; il < s.nd.nlat; ++il)
    for (int io = 0; io < O; ++io)
      for (int jo = 0; jo < O; ++jo) {
        if (io == jo) continue;
        const int q = (il * O + io) * O + jo, r = (il * O + jo) * O + io;
        // dw: spin exchange moves i -> j (entry q), pair hopping moves j -> i (entry r); wave-uniform
        const uint32_t dse = s.nd.jx != 0.0 ? __builtin_amdgcn_readfirstlane(s.nd_dw[(int64_t)q * s.dimdw + c]) : ND_INVALID;
        const uint32_t dph = s.nd.jp != 0.0 ? __builtin_amdgcn_readfirstlane(s.nd_dw[(int64_t)r * s.dimdw + c]) : ND_INVALID;
        if (dse == ND_INVALID && dph == ND_INVALID) continue;
        const uint32_t u = s.nd_up[(int64_t)r * s.dimup + ir];   // up: both terms move j -> i
        if (u == ND_INVALID) continue;
        const int jup = (int)(u & 0x7FFFFFFFu);
        if (dse != ND_INVALID) {
          const double2 x = v[(int64_t)(dse & 0x7FFFFFFFu) * s.pitch + jup];
          const double cf = ((u ^ dse) >> 31) ? -s.nd.jx : s.nd.jx;
          acc.x += cf * x.x;
          acc.y += cf * x.y;
          any = true;
        }
        if (dph != ND_INVALID) {
          const double2 x = v[(int64_t)(dph & 0x7FFFFFFFu) * s.pitch + jup];
          const double cf = ((u ^ dph) >> 31) ? -s.nd.jp : s.nd.jp;
          acc.x += cf * x.x;
          acc.y += cf * x.y;
          any = true;
        }
      }
  if (any && row_ok) {
    const int64_t o = (int64_t)cl * s.pitch + i;
    double2 h = hv[o];
    h.x += acc.x;
    h.y += acc.y;
    hv[o] = h;
  }
}

}  // namespace hxv

// pack_columns_kernel and add_pieces_kernel stood between the two kernels above and the one below; included here, at that place, so that
// the device code of hxv_kernels.hip keeps its order
#include "hxv_move_kernels.hpp"

namespace hxv {

// spH0nd handed over as stored rows (hxv_set_nonlocal_csr): hv(i) += sum_k vals(k) v(cols(k)), the loop of
// ED_HAMILTONIAN_SPARSE_HxV.f90:217-225 with one thread per local row; the global column index is split into (iup, idw) to find the
// element in the gathered layout.  A few entries per row: no tiling.
__global__ void __launch_bounds__(256) hxv_nonlocal_csr(DevSector s, const double2* __restrict__ v, double2* __restrict__ hv) {
  const int64_t nloc = (int64_t)s.qdw * s.dimup;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nloc; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k0 = s.ndcsr_rowptr[t], k1 = s.ndcsr_rowptr[t + 1];
    if (k0 == k1) continue;
    double2 acc = make_double2(0.0, 0.0);
    for (int64_t k = k0; k < k1; ++k) {
      const int64_t j = (int64_t)s.ndcsr_cols[k] - 1;  // Fortran column
      const int jdw = (int)(j / s.dimup), jup = (int)(j - (int64_t)jdw * s.dimup);
      cfma(acc, s.ndcsr_vals[k], v[(int64_t)s.vcol[jdw] * s.pitch + jup]);
    }
    const int cl = (int)(t / s.dimup);
    const int64_t o = (int64_t)cl * s.pitch + (t - (int64_t)cl * s.dimup);
    double2 h = hv[o];
    h.x += acc.x;
    h.y += acc.y;
    hv[o] = h;
  }
}

}  // namespace hxv
