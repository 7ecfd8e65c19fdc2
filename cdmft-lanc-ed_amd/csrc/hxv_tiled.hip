// Tiled two-pass kernels (gfx950) and their launcher (the plan builder is host code: hxv_tile_plan.cpp).
//
//   pass A (hxv_pass_up):  hv  = D.v + H_up v      tile = [up prefix block] x [C columns]
//   pass B (hxv_pass_dw):  hv += v H_dw^T          tile = [R rows] x [dw prefix block]
//
// A "block" is a prefix block of the sorted spin basis (hxv_tiles.hpp): hops among its low
// orbitals stay inside the tile and are gathered from LDS; hops that touch a high orbital read
// another block of the same columns (pass A) / rows (pass B) from global memory, and the
// workgroups that share those columns/rows carry the same blockIdx%8 (one XCD) so these reads
// hit its L2.  Reference semantics: ED_HAMILTONIAN_SPARSE_HxV.f90:167-227 / :230-315.
#include <algorithm>
#include <map>
#include <mutex>
#include <type_traits>

#include "hxv_tile_dev.hpp"

#ifndef HXV_PAIR_LDS
#define HXV_PAIR_LDS 1  // (0: A/B builds only -- the real-vector pass A with one 8-byte LDS element per column)
#endif
// How a workgroup of pass A starts (LABNOTES "How a workgroup starts").  -DHXV_SERIAL_TILE_LOAD=1 builds the earlier order -- one load /
// wait / store loop per tile column, the block's words read behind the barrier -- for A/B runs (scripts/build_variant.py); the results
// are bit-identical.
#ifndef HXV_SERIAL_TILE_LOAD
#define HXV_SERIAL_TILE_LOAD 0
#endif

namespace hxv {

// f(integral_constant<min(l, N)>) for l >= 1, nothing for l <= 0: code specialised on a small wave-uniform count
template <int N, typename F>
__device__ __forceinline__ void with_live_count(int l, F&& f) {
  if (l >= N)
    f(std::integral_constant<int, N>());
  else if constexpr (N > 1)
    with_live_count<N - 1>(l, f);
}

// ---------------------------------------------------------------------------------------
// pass A
// ---------------------------------------------------------------------------------------
// (Round 3 also ran this kernel with several rows per thread -- blocks of 13-14 low orbitals, or 512-thread workgroups on blocks of
//  12 -- and every such plan was slower at C3, C4 and C5 (profiles/r03_ab_mr_*.log): one row per thread it stays.)
// LZ: 0 plain product, 1 Lanczos epilogue, 2 PAIRED Lanczos epilogue (real H, complex vectors): the real and the imaginary part
// are two independent real Lanczos vectors (H(x + iy) = Hx + iHy), each with its own scalars and its own partial sums.
// ND: the spin-exchange / pair-hopping block spH0nd (Jx, Jp; sparse/H_non_local.f90:23-98, ED_HAMILTONIAN_SPARSE_HxV.f90:217-225) is
// added here instead of in a third read-modify-write pass over hv: its terms are Kronecker products of two one-body moves on a site, so
// an element's partner is (up move of the row) x (dw move of the column) -- the up moves of a row serve all C columns of the tile, the dw
// moves of a column are uniform scalars, the partner values come from one other column of the gathered vector (rows of the same block:
// the moves only touch impurity orbitals, the lowest bits).
template <int C, bool REAL, bool NORB1, int LZ, bool P16, typename VT, bool ND = false>
__global__ void __launch_bounds__(1024, 8) hxv_pass_up(DevSector s, DevTiles t, const VT* __restrict__ v,
                                                      const VT* __restrict__ wt, VT* __restrict__ hv, int ngroups,
                                                      int groups_per_xcd, int wc, LzEpilogue lz) {
  using CT = typename Coef<REAL>::type;
  extern __shared__ double2 lds_raw[];
  VT* lds = reinterpret_cast<VT*>(lds_raw);
  const int b = blockIdx.x;
  const int xcd = b & 7, j = b >> 3;
  // column group: all blocks of a group share blockIdx%8 (= one XCD), and each XCD owns a contiguous range of
  // groups because neighbouring groups share the cache lines of the transposed scratch wt
  const int gl = j / t.nblocks;
  int kb = j - gl * t.nblocks;
  // (Round 4 also ran the tiles of Kanamori sectors block-major inside chunks of 8 - 64 column groups, so that the partner columns of the
  //  folded spH0nd block's dw moves were L2-resident: 7.37 - 8.14 ms against 7.12 at C4 with Jx / Jp -- the hopping part's out-of-block
  //  gathers, then G tiles apart, lose more than the block gains; profiles/r04_ab_kanamori_chunks.log.)
  const int g = xcd * groups_per_xcd + gl;
  if (gl >= groups_per_xcd || g >= ngroups) {
    if (LZ && threadIdx.x == 0) {
      lz.partial[blockIdx.x] = 0.0;
      if (LZ == 2) lz.partial2[blockIdx.x] = 0.0;
    }
    return;
  }
  if (t.order) kb = (int)t.order[kb];  // blocks that share their in-block tables are dispatched next to each other
  const int T = blockDim.x;
  const int r0 = (int)t.start[kb];
  const int n = (int)t.start[kb + 1] - r0;
  const int tb0 = (int)t.tstart[kb];  // the block whose in-block tables this one shares
  const int c0 = g * C;  // local column
  const int nc = min(C, s.qdw - c0);
  CT* lcoef = reinterpret_cast<CT*>(lds + C * n);
  const VT* __restrict__ vcol0 = v + (int64_t)(s.slab0 + c0) * s.pitch;
  // REAL vectors (round 5): the columns of a tile are independent batch entries here (the up hops act on rows), so two adjacent columns
  // share one 16-byte LDS element: an in-block hop costs C/2 ds_read_b128 instead of C ds_read_b64 -- the LDS access pattern of the
  // complex kernel, for which the hop lists were dealt over the banks.  Same FMAs in the same order: bit-identical results.
  constexpr bool PL = HXV_PAIR_LDS && sizeof(VT) == 8 && (C % 2 == 0);
  auto lidx = [&](int cc, int r) -> int { return PL ? ((((cc >> 1) * n + r) << 1) + (cc & 1)) : cc * n + r; };
  if constexpr (HXV_SERIAL_TILE_LOAD) {
    // (A/B builds only) the load phase as it was: one loop per column, each waiting for its line before the next column's is asked for
    if constexpr (PL) {
      double2* l2 = reinterpret_cast<double2*>(lds);
#pragma unroll
      for (int pc = 0; pc < C / 2; ++pc) {
        const VT* __restrict__ sa = vcol0 + (int64_t)min(2 * pc, nc - 1) * s.pitch + r0;
        const VT* __restrict__ sb = vcol0 + (int64_t)min(2 * pc + 1, nc - 1) * s.pitch + r0;
        for (int r = threadIdx.x; r < n; r += T) l2[pc * n + r] = make_double2((double)sa[r], (double)sb[r]);
      }
    } else {
#pragma unroll
      for (int cc = 0; cc < C; ++cc) {
        const VT* __restrict__ src = vcol0 + (int64_t)min(cc, nc - 1) * s.pitch + r0;
        for (int r = threadIdx.x; r < n; r += T) lds[cc * n + r] = src[r];
      }
    }
    for (int q = threadIdx.x; q < t.nscoef; q += T) lcoef[q] = Coef<REAL>::from(t.scoef[q]);
  }
  uint32_t* lrq = reinterpret_cast<uint32_t*>(lcoef + t.nscoef);  // (ND only; the launcher adds the bytes)
  const int nvp = ND ? s.nd.nlat * s.nd.norb * (s.nd.norb - 1) : 0;  // ordered pairs of different orbitals of a site
  uint32_t* lnd = lrq + nvp;
  auto nd_tables = [&]() {
    const int O = s.nd.norb;
    for (int idx = threadIdx.x; idx < nvp * 2 * C; idx += T) {
      const int pp = idx / (2 * C), kind = (idx / C) & 1, cc = idx % C;
      const int il = pp / (O * (O - 1)), rem = pp % (O * (O - 1)), io = rem / (O - 1);
      int jo = rem % (O - 1);
      jo += jo >= io ? 1 : 0;
      const int q = (il * O + io) * O + jo, rq = (il * O + jo) * O + io;
      const int c = s.dw0 + min(c0 + cc, s.qdw - 1);
      // dw: spin exchange moves i -> j (entry q), pair hopping j -> i (entry rq); up (both terms): j -> i (entry rq)
      uint32_t w = ND_INVALID;
      if (kind == 0 && s.nd.jx != 0.0) w = s.nd_dw[(int64_t)q * s.dimdw + c];
      if (kind == 1 && s.nd.jp != 0.0) w = s.nd_dw[(int64_t)rq * s.dimdw + c];
      lnd[idx] = w;
      if (kind == 0 && cc == 0) lrq[pp] = (uint32_t)rq;
    }
  };
  if constexpr (ND && HXV_SERIAL_TILE_LOAD) nd_tables();
  const uint32_t p16m = (1u << t.p16_bits) - 1u;  // half-size table words: (coefficient index << p16_bits) | offset
  double asum = 0.0;
  // one row per thread (the plan guarantees n <= blockDim.x)
  const int p = threadIdx.x;
  VT acc[C];
  double au = 0.0;
  uint32_t mu = 0;
  // Issued BEFORE the barrier so their latency hides behind the tile load: the dw-hop part that pass B left in the
  // column-group-blocked scratch wt[group][row][wc] (C*16 contiguous bytes per row, rows consecutive: a plain
  // streaming read) becomes the initial value of the accumulators; the diagonal's per-row inputs come along.
  auto row_inputs = [&]() {
    if (p < n) {
      if (wt && wc == 0) {
        // natural layout [local column][pitch] (the dw part assembled like hv) -- or, with t.wtr, the same in PIECES (all-to-all
        // exchange): one block per rank of origin, read where the second transpose left it (WtRange)
        const VT* wb = wt;
        int64_t wstr = s.pitch;
        int wrow = r0 + p;
        if (t.wtr) {
          int k = 0;
          while (k + 1 < t.nwtr && wrow >= t.wtr[k].row1) ++k;
          wb = reinterpret_cast<const VT*>(t.wtr[k].base);
          wstr = t.wtr[k].stride;
          wrow -= t.wtr[k].row0;
        }
        const VT* __restrict__ wcol = wb + (int64_t)c0 * wstr + wrow;
#pragma unroll
        for (int cc = 0; cc < C; ++cc) acc[cc] = wcol[(int64_t)min(cc, nc - 1) * wstr];
      } else if (wt && (wc >> 8)) {
        // blocked scratch with COLUMN-MAJOR patches (round 5): wt[group][patch of Rp rows][wcl columns][Rp rows], Rp = pass B's rows per tile in
        // this kernel's element units.  Pass B still writes Rp*wcl*16 contiguous bytes per patch; here the Rp lanes of a patch read Rp*16
        // contiguous bytes per column instead of each lane its own 64-byte stretch four (eight) times over: a quarter of the L1 accesses
        // for the same lines.  (REAL vectors whose pass B ran on row pairs arrive in the same layout: a pair of rows IS two rows of it.)
        const int wcl = wc & 0xFF, Rp = wc >> 8, row = r0 + p;
        const int dR = (s.dimup + Rp - 1) & ~(Rp - 1);
        const VT* __restrict__ wrow = wt + ((int64_t)(c0 / wcl) * dR + (row & ~(Rp - 1))) * wcl + (int64_t)(c0 % wcl) * Rp + (row & (Rp - 1));
#pragma unroll
        for (int cc = 0; cc < C; ++cc) acc[cc] = wrow[min(cc, nc - 1) * Rp];
      } else if (wt) {
        const VT* __restrict__ wrow = wt + ((int64_t)(c0 / wc) * s.dimup + r0 + p) * wc + (c0 % wc);
#pragma unroll
        for (int cc = 0; cc < C; ++cc) acc[cc] = wrow[min(cc, nc - 1)];
      } else {
#pragma unroll
        for (int cc = 0; cc < C; ++cc) acc[cc] = vzero<VT>();
      }
      if (s.diag.mode == 0) {
        au = s.diag.a_up[r0 + p];
        mu = s.diag.map_up[r0 + p];
      }
    }
  };
  // What depends only on the block and the wave is asked for in front of the barrier, so that it arrives behind the tile load instead of
  // behind the barrier: the wave's in-block list length (with the tile loads; one register carries it over the barrier) and the ranges of
  // the block hops and the row slots.
  constexpr bool EARLY_KB = !HXV_SERIAL_TILE_LOAD;
  uint32_t gm_early = 0, bh_lo = 0, bh_hi = 0, rs_lo = 0, rs_hi = 0;
  const uint32_t* __restrict__ gm_src = t.gmax + t.gstart[kb];
  if constexpr (EARLY_KB) {
    bh_lo = t.bh_ptr[kb];
    bh_hi = t.bh_ptr[kb + 1];
    rs_lo = t.rs_ptr[kb];
    rs_hi = t.rs_ptr[kb + 1];
  }
  if constexpr (!HXV_SERIAL_TILE_LOAD) {
    // The load phase is straight-line code: a thread with a row asks for its C tile elements, the wave's list length and a coefficient word
    // back to back -- one round trip to memory with all of them in flight -- and stores to LDS as the answers arrive.  (As one loop per
    // column -- the compiler cannot know that n <= blockDim.x makes each run once -- every column's line was waited for before the next was
    // asked for: four dependent round trips and a fifth for the coefficients.)  No branch lies between the loads and the stores -- the
    // compiler moves a load down to the block of its first use -- so the coefficient word has no guard: threads past the table copy its
    // last word once more.  The accumulators' loads follow the stores and stay in flight across the barrier: ahead of the stores, they
    // and the tile do not fit the 64 registers -- the scheduler then moves half of the tile loads below the first store
    // (LABNOTES, "How a workgroup starts").
    if (p < n) {
      const int qc = min(p, t.nscoef - 1);
      VT tx[C];
      const VT* __restrict__ src = vcol0 + r0 + p;
#pragma unroll
      for (int cc = 0; cc < C; ++cc) tx[cc] = src[(int64_t)min(cc, nc - 1) * s.pitch];
      gm_early = gm_src[p >> 6];
      const double2 cw = t.scoef[qc];
      if constexpr (PL) {
        double2* l2 = reinterpret_cast<double2*>(lds);
#pragma unroll
        for (int pc = 0; pc < C / 2; ++pc) l2[pc * n + p] = make_double2((double)tx[2 * pc], (double)tx[2 * pc + 1]);
      } else {
#pragma unroll
        for (int cc = 0; cc < C; ++cc) lds[cc * n + p] = tx[cc];
      }
      lcoef[qc] = Coef<REAL>::from(cw);
    } else if (p < t.nscoef) {  // (a block with fewer rows than there are coefficients)
      lcoef[p] = Coef<REAL>::from(t.scoef[p]);
    }
    for (int q = p + T; q < t.nscoef; q += T) lcoef[q] = Coef<REAL>::from(t.scoef[q]);  // (a table longer than the workgroup: up to 511 words on 256 threads)
    if constexpr (ND) nd_tables();
  }
  row_inputs();
  __syncthreads();
  VT xq[LZ ? C : 1];  // the thread's own input elements, kept for the Lanczos epilogue
  if (p < n) {
    const uint32_t packed = __builtin_amdgcn_readfirstlane(EARLY_KB ? gm_early : gm_src[p >> 6]);
    const int kin = (int)(packed & 0xFFFFu);
    if (LZ) {
#pragma unroll
      for (int cc = 0; cc < C; ++cc) xq[LZ ? cc : 0] = lds[lidx(cc, p)];
    }
    const int i = r0 + p;  // pass A visits the rows in natural order: every global access stays coalesced
    const int r = p;
    if (s.diag.mode == 0) {
#pragma unroll
      for (int cc = 0; cc < C; ++cc) {
        const double d = diag_value<NORB1>(s.diag, au, mu, s.dw0 + min(c0 + cc, s.qdw - 1));
        Coef<true>::fma(acc[cc], d, lds[lidx(cc, r)]);
      }
    } else {
#pragma unroll
      for (int cc = 0; cc < C; ++cc) {
        const double d = s.diag.stored[(int64_t)min(c0 + cc, s.qdw - 1) * s.dimup + i];
        Coef<true>::fma(acc[cc], d, lds[lidx(cc, r)]);
      }
    }
    // hops that leave the block, same columns, other rows: from global memory (L2 of this XCD)
    if (!(t.debug & 1)) {
      // block hops: the partner block is one contiguous run, lanes read consecutive rows
      const uint32_t bh0 = EARLY_KB ? bh_lo : t.bh_ptr[kb], bh1 = EARLY_KB ? bh_hi : t.bh_ptr[kb + 1];
      for (uint32_t h = bh0; h < ((t.debug & 256) ? bh0 : bh1); ++h) {
        const CT cf = lcoef[t.bh[2 * h + 1]];
        const VT* __restrict__ src = vcol0 + t.bh[2 * h] + r;
#pragma unroll
        for (int cc = 0; cc < C; ++cc) Coef<REAL>::fma(acc[cc], cf, src[(int64_t)min(cc, nc - 1) * s.pitch]);
      }
      // row slots: one table word per row and (block, source block) pair -- or, packed, per TWO such pairs (P16)
      const uint32_t rs0 = EARLY_KB ? rs_lo : t.rs_ptr[kb];
      const uint32_t rs1 = (t.debug & 512) ? rs0 : (EARLY_KB ? rs_hi : t.rs_ptr[kb + 1]);
      // (eight-column tiles -- real vectors -- keep one word per slot: with the packed words the fused real-vector pass A went from
      //  1.67 to 1.88 ms at C3, the whole round-3 regression of the real Lanczos iteration, 3.77 -> 3.96 ms; profiles/r04_bisect_real.log)
      if (P16 && C < 8 && t.rs16) {
        const uint32_t empty16 = (uint32_t)(t.nscoef - 1) << t.p16_bits;
        for (uint32_t sl = rs0; sl < rs1; sl += 2) {
          const uint32_t w = t.rs16[t.rs16_off[sl] + r];
#pragma unroll
          for (int hh = 0; hh < 2; ++hh) {
            if (sl + hh < rs1) {  // (uniform)
              const uint32_t e = hh ? w >> 16 : w & 0xFFFFu;
              if (__all(e == empty16)) continue;
              CT cf = lcoef[e >> t.p16_bits];
              if (t.rs_neg[sl + hh]) cf = Coef<REAL>::neg(cf);  // (uniform: the shared table holds the other overall sign)
              const VT* __restrict__ src = vcol0 + t.rs_base[sl + hh] + (e & p16m);
#pragma unroll
              for (int cc = 0; cc < C; ++cc) Coef<REAL>::fma(acc[cc], cf, src[(int64_t)min(cc, nc - 1) * s.pitch]);
            }
          }
        }
      } else {
        const uint32_t emptyz = (uint32_t)(t.nscoef - 1) << TILE_COEF_SHIFT;
        for (uint32_t sl = rs0; sl < rs1; ++sl) {
          const uint32_t e = t.rs_tab[t.rs_off[sl] + r];
          if (__all(e == emptyz)) continue;
          CT cf = lcoef[e >> TILE_COEF_SHIFT];
          if (t.rs_neg[sl]) cf = Coef<REAL>::neg(cf);  // (uniform: the shared table holds the other overall sign)
          const VT* __restrict__ src = vcol0 + t.rs_base[sl] + (e & TILE_OFF_MASK);
#pragma unroll
          for (int cc = 0; cc < C; ++cc) Coef<REAL>::fma(acc[cc], cf, src[(int64_t)min(cc, nc - 1) * s.pitch]);
        }
      }
    }
    if constexpr (ND) {
      // lrq / lnd (LDS, filled with the tile): per ordered orbital pair p of a site, the up-move table row and, per column of the tile, the
      // dw partner columns of the two terms -- uniform values, read back as scalars; a term the column's dw state rules out costs nothing.
      // Lanes whose up state rules the move out fetch their own row with a zero coefficient (no lane-divergent branch around a load).
      for (int p0 = 0; p0 < nvp; p0 += 8) {
        uint32_t u[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (p0 + k < nvp) u[k] = s.nd_up[(int64_t)__builtin_amdgcn_readfirstlane(lrq[p0 + k]) * s.dimup + i];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          if (p0 + k < nvp) {
            const bool upok = u[k] != ND_INVALID;
            const int64_t jup = upok ? (int64_t)(u[k] & 0x7FFFFFFFu) : (int64_t)r0;  // (idle lanes: one shared address)
            uint32_t dw[2 * C];  // the pair's partner columns for the C columns of the tile: one batch of LDS reads
#pragma unroll
            for (int e = 0; e < 2 * C; ++e) dw[e] = lnd[(p0 + k) * 2 * C + e];
#pragma unroll
            for (int e = 0; e < 2 * C; ++e) dw[e] = __builtin_amdgcn_readfirstlane(dw[e]);
#pragma unroll
            for (int cc = 0; cc < C; ++cc) {
              const uint32_t dse = dw[cc], dph = dw[C + cc];
              VT x1 = vzero<VT>(), x2 = vzero<VT>();
              if (dse != ND_INVALID) x1 = v[(int64_t)(dse & 0x7FFFFFFFu) * s.pitch + jup];
              if (dph != ND_INVALID) x2 = v[(int64_t)(dph & 0x7FFFFFFFu) * s.pitch + jup];
              if (dse != ND_INVALID) Coef<true>::fma(acc[cc], upok ? (((u[k] ^ dse) >> 31) ? -s.nd.jx : s.nd.jx) : 0.0, x1);
              if (dph != ND_INVALID) Coef<true>::fma(acc[cc], upok ? (((u[k] ^ dph) >> 31) ? -s.nd.jp : s.nd.jp) : 0.0, x2);
            }
          }
        }
      }
    }
    // hops inside the block: gathers from the LDS tile
    for (int k0 = 0; k0 < ((t.debug & 2) ? 0 : kin); k0 += HOP_CHUNK) {
      uint32_t e[P16 ? HOP_CHUNK / 2 : HOP_CHUNK];
      if constexpr (P16) {  // half-size table: two hops per word
#pragma unroll
        for (int u = 0; u < HOP_CHUNK / 2; ++u) e[u] = t.ell16[(int64_t)(k0 / 2 + u) * s.dimup + tb0 + p];
      } else {
#pragma unroll
        for (int u = 0; u < HOP_CHUNK; ++u) e[u] = t.ell_in[(int64_t)(k0 + u) * s.dimup + tb0 + p];
      }
#pragma unroll
      for (int u = 0; u < HOP_CHUNK; ++u) {
        if (k0 + u < kin) {  // wave-uniform: all 8 words are loaded at once, only the live slots are computed
          uint32_t ci;
          int off;
          if constexpr (P16) {
            const uint32_t hw = (u & 1) ? e[u >> 1] >> 16 : e[u >> 1] & 0xFFFFu;
            ci = hw >> t.p16_bits;
            off = (int)(hw & p16m);
          } else {
            ci = e[u] >> TILE_COEF_SHIFT;
            off = (int)(e[u] & TILE_OFF_MASK);
          }
          const CT cf = lcoef[ci];
          if constexpr (PL) {
            const double2* l2 = reinterpret_cast<const double2*>(lds);
#pragma unroll
            for (int pc = 0; pc < C / 2; ++pc) {
              const double2 x2 = l2[pc * n + off];
              Coef<REAL>::fma(acc[2 * pc], cf, x2.x);
              Coef<REAL>::fma(acc[2 * pc + 1], cf, x2.y);
            }
          } else {
#pragma unroll
            for (int cc = 0; cc < C; ++cc) Coef<REAL>::fma(acc[cc], cf, lds[cc * n + off]);
          }
        }
      }
    }
  }
  // Epilogue, same thread <-> row mapping: store hv with lanes along the rows.
  // With LZ: w = s*(H x) - c*xm and the partial sums of Re(conj(s*x) w).
  double asum2 = 0.0;  // (LZ == 2: the imaginary-part vector's sum)
  if (p < n) {
    const double sc = LZ ? lz.scal[lz.i_s] : 1.0;
    const double cm = (LZ && lz.xm) ? lz.scal[lz.i_c] : 0.0;
    const double sc2 = LZ == 2 ? lz.scal[lz.i_s2] : 1.0;
    const double cm2 = (LZ == 2 && lz.xm) ? lz.scal[lz.i_c2] : 0.0;
#pragma unroll
    for (int cc = 0; cc < C; ++cc) {
      if (cc < nc) {
        const int64_t o = (int64_t)(c0 + cc) * s.pitch + r0 + p;
        VT w = acc[cc];
        if constexpr (LZ == 2) {
          // component-wise: the same operations, in the same order, as two LZ == 1 runs on (x, 0) and (y, 0)
          const VT xo = xq[cc];
          pair_scale(w, sc, sc2);
          if (lz.xm) pair_fma(w, -cm, -cm2, reinterpret_cast<const VT*>(lz.xm)[o]);
          asum = ::fma(sc, pair_dot_re(xo, w), asum);
          asum2 = ::fma(sc2, pair_dot_im(xo, w), asum2);
        } else if (LZ) {
          vscale(w, sc);
          if (lz.xm) Coef<true>::fma(w, -cm, reinterpret_cast<const VT*>(lz.xm)[o]);
          asum = ::fma(sc, vdot(xq[LZ ? cc : 0], w), asum);
        }
        if (t.debug & 8)
          hv[o] = w;
        else  // contiguous runs of a whole block: streaming stores measured ~10 % faster here
          store_stream(&hv[o], w);
      }
    }
  }
  if (LZ) {
    // wavefront partial sums first (shuffles), one LDS word per wave afterwards: two barriers instead of a tree of eleven
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      asum += __shfl_down(asum, off, 64);
      if (LZ == 2) asum2 += __shfl_down(asum2, off, 64);
    }
    __syncthreads();  // every gather from the tile is done
    double* red = reinterpret_cast<double*>(lds);
    if ((threadIdx.x & 63) == 0) {
      red[threadIdx.x >> 6] = asum;
      if (LZ == 2) red[16 + (threadIdx.x >> 6)] = asum2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double tot = 0.0, tot2 = 0.0;
      for (int w = 0; w < (T >> 6); ++w) {
        tot += red[w];
        if (LZ == 2) tot2 += red[16 + w];
      }
      lz.partial[blockIdx.x] = tot;
      if (LZ == 2) lz.partial2[blockIdx.x] = tot2;
    }
  }
}

// ---------------------------------------------------------------------------------------
// pass B.  Tile element (column c of the block, row r) sits at pair index q = c*R + r in LDS, which is also the order the
// lanes touch global memory in (lanes along the R contiguous rows of a column: coalesced 16*R-byte segments), so the
// streaming phases address LDS linearly.  In the in-block phase a thread owns one column and its R rows: one table decode
// serves R gathers at immediate offsets.  The out-of-block hops run lanes along the rows again: before the in-block phase with
// their sums in registers, or after the in-block sums have been parked in the tile (ORD below).
// The address arithmetic is kept off the vector ALU (it was more than half of this kernel's instructions): blockDim.x is a
// multiple of R, so a thread's pairs all have the same row; every global access is a uniform 64-bit base plus a per-thread
// 32-bit byte offset that is computed once (tile load, block hops, scratch store), or one 64-bit multiply-add (row slots).
// ---------------------------------------------------------------------------------------
// ORD, the order of the phases (chosen by the launcher, launch_dw_np):
//   0  tile load | in-block hops | park the sums in the tile | out-of-block hops, each sum added into the tile | store from the tile
//   1  tile load | out-of-block hops with their sums kept in registers, in-block hops (no barrier in between: a wave that has its
//      gathers starts its LDS work while others still gather) | park | own elements of the tile + register sums, stored straight from
//      the registers: one barrier and one read-modify-write pass over the tile fewer, and the out-of-block gathers (global memory only,
//      they depend on nothing in the tile) no longer wait behind the LDS-only phase.  A thread's pairs are then the ones of the blocked
//      store: columns counted from the block's aligned scratch group, `sh` = 0 .. wc-1 columns in front of the block, so the first sh
//      column positions of a workgroup are dead lanes (plan: max_block + wc - 1 columns fit NP sweeps).
//      (With the gathers ahead of the first barrier instead -- every wave then writes its own copy of the coefficient table -- C3 gained
//      a third of what this placement gains: profiles/pass_b_phase_order_ab.log.)
// The floating-point operations and their order are the same in every order.
template <int R, int NP, bool REAL, bool P16, typename VT, int ORD = 0>
__global__ void __launch_bounds__(1024, 8) hxv_pass_dw(DevSector s, DevTiles t, const VT* __restrict__ v, VT* __restrict__ wt,
                                                      int ngroups, int groups_per_xcd, int wc) {
  // NP = (row,column) pairs of the tile per thread (plan: max_block*R <= NP*blockDim.x); all their global
  // loads are issued before the first use so a workgroup keeps NP requests per lane in flight.
  using CT = typename Coef<REAL>::type;
  extern __shared__ double2 lds_raw[];
  constexpr int VB = (int)sizeof(VT);
  constexpr int LR = R == 2 ? 1 : (R == 4 ? 2 : 3);
  static_assert(R == 2 || R == 4 || R == 8, "R");
  const int b = blockIdx.x;
  const int xcd = b & 7, j = b >> 3;
  int gl = j / t.nblocks;
  int kb = j - gl * t.nblocks;
  if (t.pair_rows) {
    // Large sectors: one row group's panel (R rows x DimDw columns, in R*16-byte pieces of 128-byte lines) no longer fits the
    // XCD's L2 next to its neighbour's, so the row group that shares its lines would find them evicted.  The two run back
    // to back instead, block by block (Ns=18: pass B 53.8 -> 47.5 ms; at Ns=16, where both panels fit, this order is 7 % slower).
    const int pr = j / (2 * t.nblocks), rem = j - pr * 2 * t.nblocks;
    kb = rem >> 1;
    gl = 2 * pr + (rem & 1);
  }
  const int rg = xcd * groups_per_xcd + gl;  // contiguous row ranges per XCD: neighbouring row groups share cache lines
  if (gl >= groups_per_xcd || rg >= ngroups) return;
  if (t.order) kb = (int)t.order[kb];  // blocks that share their in-block tables are dispatched next to each other
  const int cb0 = (int)t.start[kb];
  const int n = (int)t.start[kb + 1] - cb0;
  if (cb0 + n <= s.dw0 || cb0 >= s.dw0 + s.qdw) return;  // block holds no local output column
  const int T = blockDim.x;
  const int tid = threadIdx.x;
  const int i0 = rg * R;
  // LDS (by byte offset): the signed coefficients at 0 -- an in-block table word's coefficient field shifted down IS the
  // coefficient's address, because a column offset within a block (< 1024) leaves the bits between the fields clear --
  // and the tile behind them
  constexpr int LCB = sizeof(CT) == 8 ? 3 : 4;
  constexpr int LTB = LR + (VB == 8 ? 3 : 4);  // log2 of the bytes of one column of the tile
  const uint32_t ltile = (uint32_t)((t.nscoef << LCB) + 255) & ~255u;
  // XOR swizzle of the R row positions inside a column's chunk by the column's index among the columns that share its
  // 256-byte bank sweep: without it the R gathers of an in-block hop (all lanes at the same row position of random
  // columns) would use only 1/R of the banks.  The linear phases see a permutation inside each chunk: still conflict-free.
  constexpr int LSW = 8 - LTB;                      // log2(columns per 256 B); LTB <= 7
  constexpr int LVB = VB == 8 ? 3 : 4;
  auto swz_of = [](uint32_t col) -> uint32_t { return ((col >> LSW) & (R - 1)) << LVB; };  // byte XOR of a column
  constexpr bool REGS = ORD != 0;
  static_assert(!REGS || NP <= 4, "the register sums of eight pairs do not fit");
  // REGS: columns in front of the block in the thread-to-pair mapping (blocked scratch: the block start's misalignment to the group width)
  const int sh = (REGS && wc) ? ((cb0 - s.dw0) & ((wc & 0xFF) - 1)) : 0;
  const int c0 = (tid >> LR) - sh;  // column of this thread's pair 0 within the block (REGS: negative in a dead lane)
  // this thread's pair 0 in the tile (pair it: + it*T*VB; a sweep advances the column by T/R, which leaves its swizzle bits alone)
  const uint32_t tq = REGS ? ltile + (uint32_t)((c0 << LTB) + ((int)((uint32_t)(tid & (R - 1)) << LVB) ^ (int)swz_of((uint32_t)c0)))
                           : ltile + (((uint32_t)tid << LVB) ^ swz_of((uint32_t)tid >> LR));
  const uint32_t emptyz = (uint32_t)(t.nscoef - 1) << TILE_COEF_SHIFT;
  const uint32_t p16m = (1u << t.p16_bits) - 1u;  // half-size table words: (coefficient index << p16_bits) | column
  for (int q = tid; q < t.nscoef; q += T) lds_st<CT>(q << LCB, Coef<REAL>::from(t.scoef[q]));
  // per-thread constants
  const int r = tid & (R - 1);
  const int cstep = T >> LR;                      // columns between a thread's consecutive pairs
  const uint32_t pitchb = (uint32_t)s.pitch * VB;  // bytes per column
  const uint32_t rowb = (uint32_t)(min(i0 + r, s.dimup - 1) - i0) * VB;
  const char* __restrict__ vrows = reinterpret_cast<const char*>(v) + (int64_t)i0 * VB;  // uniform
  // column of pair `it` within the block (clamped) and its byte offset relative to (first column of a block, row i0);
  // the offsets are kept in registers when a thread has few pairs and recomputed (two instructions) when it has eight
  auto ccol = [&](int it) -> uint32_t { return (uint32_t)min(REGS && it == 0 ? max(c0, 0) : c0 + it * cstep, n - 1); };
  auto owns = [&](int it) -> bool { return REGS ? (uint32_t)(c0 + it * cstep) < (uint32_t)n : c0 + it * cstep < n; };  // pair `it` lies in the block
  constexpr bool KEEP = NP <= 4 && R < 8;  // (eight-row tiles need the registers for their accumulators)
  uint32_t voff_keep[KEEP ? NP : 1];
  if constexpr (KEEP) {
#pragma unroll
    for (int it = 0; it < NP; ++it) voff_keep[it] = ccol(it) * pitchb + rowb;
  }
  auto voff = [&](int it) -> uint32_t {
    if constexpr (KEEP)
      return voff_keep[it];
    else
      return ccol(it) * pitchb + rowb;
  };
  // NP is sized for the largest block: in a smaller one the last pair iterations of a wave can lie past the block altogether (C3: a
  // fifth of all wave iterations).  That is a wave-uniform fact -- the iterations [nlive, NP) of this wave have no live lane -- and
  // nothing is issued for them: no tile load, no block hop's load, no row slot's word or gather, no add into the tile.  Waves that
  // are partly live keep the clamped column.
  const int wcol0 = (__builtin_amdgcn_readfirstlane(tid) >> LR) - sh;  // the wave's first column of pair 0 (every lane is active here)
  int nlive = 0;
#pragma unroll
  for (int it = 0; it < NP; ++it) nlive += (wcol0 + it * cstep < n || (t.debug & 4096)) ? 1 : 0;
  const uint32_t rs0 = t.rs_ptr[kb], rs_end = (t.debug & 512) ? rs0 : t.rs_ptr[kb + 1];
  // phase 0: tile load
  {
    VT x[NP];
    if (s.vcol_identity) {
      const char* __restrict__ src = vrows + (int64_t)cb0 * pitchb;
#pragma unroll
      for (int it = 0; it < NP; ++it)
        if (it < nlive) x[it] = *reinterpret_cast<const VT*>(src + voff(it));
    } else {
      uint32_t slot[NP];
#pragma unroll
      for (int it = 0; it < NP; ++it)
        if (it < nlive) slot[it] = s.vcol[cb0 + ccol(it)];
#pragma unroll
      for (int it = 0; it < NP; ++it)
        if (it < nlive) x[it] = *reinterpret_cast<const VT*>(vrows + ((uint64_t)slot[it] * pitchb + rowb));
    }
#pragma unroll
    for (int it = 0; it < NP; ++it) {
      if (it < nlive && owns(it)) lds_st<VT>(tq + it * T * VB, x[it]);
    }
  }
  // out-of-block hops: lanes along the contiguous rows again (coalesced R*16-byte segments of other columns, L2 of
  // this XCD); ORD 0: the sums are added into the tile, each element by the one thread that owns the (row,column) pair;
  // REGS: they stay in okeep until the store.
  // Pairs are handled HB at a time to bound the registers (two 1024-thread workgroups per CU need <= 64 VGPRs).
  VT okeep[REGS ? NP : 1];
  if constexpr (REGS) {
#pragma unroll
    for (int it = 0; it < NP; ++it) okeep[it] = vzero<VT>();
  }
  auto out_of_block = [&]() {
    if (t.debug & 1) return;
    constexpr int HB = NP > 4 ? 4 : NP;
    const char* __restrict__ vrow64 = vrows + rowb;  // per-thread 64-bit base of the row-slot gathers
    // One group of HB pairs, compiled once per number L of its pairs that have a live lane in this wave (the live ones come first):
    // straight-line code for every L, so the register arrays stay arrays of registers; L = HB is the kernel as it was.
    auto group = [&](auto lc, const int base) {
      constexpr int L = decltype(lc)::value;
      // (REGS: one group, base = 0, and the sums are accumulated where they stay -- copying them out of the L-specialised code
      //  afterwards let the compiler merge the copies of different L into one indexed store, which put half of okeep into scratch memory)
      VT osum_own[REGS ? 1 : L];
      VT* const osum = REGS ? okeep : osum_own;
      if constexpr (!REGS) {
#pragma unroll
        for (int it = 0; it < L; ++it) osum[it] = vzero<VT>();
      }
      // block hops: source column slot = start + column offset, one signed coefficient for the whole block
      for (uint32_t h = t.bh_ptr[kb]; h < ((t.debug & 256) ? t.bh_ptr[kb] : t.bh_ptr[kb + 1]); ++h) {
        const CT cf = lds_ld<CT>(t.bh[2 * h + 1] << LCB);
        const char* __restrict__ src = vrows + (int64_t)t.bh[2 * h] * pitchb;
        VT x[L];
#pragma unroll
        for (int it = 0; it < L; ++it) x[it] = *reinterpret_cast<const VT*>(src + voff(base + it));
#pragma unroll
        for (int it = 0; it < L; ++it) Coef<REAL>::fma(osum[it], cf, x[it]);
      }
      // row slots: one table word per column of the block and (block, source block) pair; the words of SB slots
      // are fetched together so that the gathers that depend on them follow one table round trip, not SB
      // (the half-size, two-slots-per-word copy of these tables serves pass A only: here its decode costs the registers that
      //  keep eight-pair tiles from spilling, for no measurable gain)
      constexpr int SB = 2;
      for (uint32_t sl0 = rs0; sl0 < rs_end; sl0 += SB) {
        uint32_t e[SB][L];
#pragma unroll
        for (int jj = 0; jj < SB; ++jj) {
          if (sl0 + jj < rs_end) {  // uniform
            const uint32_t* __restrict__ tab = t.rs_tab + t.rs_off[sl0 + jj];
#pragma unroll
            for (int it = 0; it < L; ++it) e[jj][it] = tab[ccol(base + it)];
          }
        }
#pragma unroll
        for (int jj = 0; jj < SB; ++jj) {
          if (sl0 + jj < rs_end) {
            bool none = true;
#pragma unroll
            for (int it = 0; it < L; ++it) none = none && (e[jj][it] == emptyz);
            if (__all(none)) continue;
            VT x[L];
            const char* __restrict__ vslot = vrow64 + (uint64_t)t.rs_base[sl0 + jj] * pitchb;  // (the slot's source block)
            const bool neg = t.rs_neg[sl0 + jj] != 0;  // (uniform: the shared table holds the other overall sign)
#pragma unroll
            for (int it = 0; it < L; ++it)
              x[it] = *reinterpret_cast<const VT*>(vslot + (uint64_t)(e[jj][it] & TILE_OFF_MASK) * pitchb);
#pragma unroll
            for (int it = 0; it < L; ++it) {
              CT cf = lds_ld<CT>((e[jj][it] >> TILE_COEF_SHIFT) << LCB);
              if (neg) cf = Coef<REAL>::neg(cf);
              Coef<REAL>::fma(osum[it], cf, x[it]);
            }
          }
        }
      }
      if constexpr (!REGS) {
#pragma unroll
        for (int it = 0; it < L; ++it) {
          if ((tid >> LR) + (base + it) * cstep < n) {
            const uint32_t q = tq + (base + it) * T * VB;
            VT a = lds_ld<VT>(q);
            vadd(a, osum[it]);
            lds_st<VT>(q, a);
          }
        }
      }
    };
#pragma unroll
    for (int base = 0; base < NP; base += HB) with_live_count<HB>(nlive - base, [&](auto lc) { group(lc, base); });  // (uniform)
  };
  __syncthreads();
  if constexpr (REGS) out_of_block();
  // in-block hops, one column per thread (plan guarantees n <= blockDim.x)
  {
    VT acc[R];
    int col1 = 0;
    if (tid < n) {
      const uint32_t packed = __builtin_amdgcn_readfirstlane(t.gmax[t.gstart[kb] + (tid >> 6)]);
      const int kin = (t.debug & 2) ? 0 : (int)(packed & 0xFFFFu);
      const int tb0 = (int)t.tstart[kb];  // the block whose in-block tables this one shares
      col1 = (int)t.perm[tb0 + tid] - tb0;
      const uint32_t* __restrict__ ellp = (P16 ? t.ell16 : t.ell_in) + tb0 + tid;
#pragma unroll
      for (int rr = 0; rr < R; ++rr) acc[rr] = vzero<VT>();
      for (int k0 = 0; k0 < kin; k0 += HOP_CHUNK) {
        uint32_t e[P16 ? HOP_CHUNK / 2 : HOP_CHUNK];
        if constexpr (P16) {
#pragma unroll
          for (int u = 0; u < HOP_CHUNK / 2; ++u) e[u] = ellp[(int64_t)(k0 / 2 + u) * s.dimdw];
        } else {
#pragma unroll
          for (int u = 0; u < HOP_CHUNK; ++u) e[u] = ellp[(int64_t)(k0 + u) * s.dimdw];
        }
#pragma unroll
        for (int u = 0; u < HOP_CHUNK; ++u) {
          if (k0 + u < kin) {  // wave-uniform
            uint32_t cfa, col;  // coefficient's LDS address, source column within the block
            if constexpr (P16) {
              const uint32_t hw = (u & 1) ? e[u >> 1] >> 16 : e[u >> 1] & 0xFFFFu;
              cfa = (hw >> t.p16_bits) << LCB;
              col = hw & p16m;
            } else {
              cfa = e[u] >> (TILE_COEF_SHIFT - LCB);
              col = e[u] & TILE_OFF_MASK;
            }
            const CT cf = lds_ld<CT>(cfa);
            const uint32_t src = shl_add<LTB>(col, ltile), sw = swz_of(col);
#pragma unroll
            for (int rr = 0; rr < R; ++rr) Coef<REAL>::fma(acc[rr], cf, lds_ld<VT>(src + ((uint32_t)(rr * VB) ^ sw)));
          }
        }
      }
    }
    __syncthreads();  // every in-block gather is done: the tile can be overwritten by the sums
    if (tid < n) {
      const uint32_t dst = ltile + ((uint32_t)col1 << LTB), sw = swz_of((uint32_t)col1);
#pragma unroll
      for (int rr = 0; rr < R; ++rr) lds_st<VT>(dst + ((uint32_t)(rr * VB) ^ sw), acc[rr]);
    }
  }
  __syncthreads();
  if constexpr (!REGS) {
    out_of_block();
    __syncthreads();
  }
  const int cl0 = max(cb0, s.dw0) - s.dw0, cl1 = min(cb0 + n, s.dw0 + s.qdw) - s.dw0;  // local output columns [cl0,cl1)
  if constexpr (REGS) {
    // every thread finishes its own pairs: in-block sum from the tile + out-of-block sum from its registers (the addition the tile's
    // read-modify-write did), stored from the registers.  A local column in [cl0,cl1) is a column of the block, so the guard of the
    // store is the guard of the tile read as well.
    const bool rowok = i0 + r < s.dimup;
    const int lc0 = cb0 - s.dw0 + c0;  // local column of pair 0
    if (wc == 0) {  // natural layout [local column][pitch] (the launcher passes no row-major patches here)
#pragma unroll
      for (int it = 0; it < NP; ++it) {
        const int lc = lc0 + it * cstep;
        if (it < nlive && lc >= cl0 && lc < cl1 && rowok) {
          VT a = lds_ld<VT>(tq + it * T * VB);
          vadd(a, okeep[it]);
          wt[(int64_t)lc * s.pitch + i0 + r] = a;
        }
      }
      return;
    }
    // blocked scratch, column-major patches: pair (column lc, row r) is element (lc mod wc)*R + r of the patch of group lc / wc, and
    // lc0 - c0's group is aligned to the mapping -- the addresses are the ones of the sweeps below with g0 = that group (it lies before
    // the slab when the slab's edge cuts the block: nothing is stored there)
    wc &= 0xFF;
    const int lw = 31 - __clz(wc);
    const int gb = (lc0 - (tid >> LR)) >> lw;  // (arithmetic shift of a multiple of wc)
    const int per = R << lw;
    const int gstep = T >> (LR + lw);
    const int rem = tid & (per - 1), gi = tid >> (LR + lw);
    const uint32_t drows = (uint32_t)((s.dimup + R - 1) & ~(R - 1));
    const uint32_t so = (uint32_t)gi * (drows * per / R * VB) + (uint32_t)rem * VB;
    char* __restrict__ dstb = reinterpret_cast<char*>(wt) + ((int64_t)gb * (int64_t)drows + i0) * ((int64_t)VB << lw);
    const int64_t dstep = (int64_t)gstep * drows * ((int64_t)VB << lw);
#pragma unroll
    for (int it = 0; it < NP; ++it) {
      const int lc = lc0 + it * cstep;
      if (it < nlive && lc >= cl0 && lc < cl1 && rowok) {
        VT a = lds_ld<VT>(tq + it * T * VB);
        vadd(a, okeep[it]);
        store_stream(reinterpret_cast<VT*>(dstb + it * dstep + so), a);  // (streaming: see below)
      }
    }
    return;
  }
  if (wc == 0) {
    // natural layout [local column][pitch], lanes along the R rows (row-panel product of the all-to-all exchange:
    // 1/P of the data, so the short strided write runs do not matter)
    for (int q = tid, k = 0; q < n * R; q += T, ++k) {
      const int lc = cb0 + (q >> LR) - s.dw0;
      if (lc >= cl0 && lc < cl1 && i0 + r < s.dimup) wt[(int64_t)lc * s.pitch + i0 + r] = lds_ld<VT>(tq + k * T * VB);
    }
    return;
  }
  // store into the column-group-blocked scratch wt[group][row][wc] (wc = pass A's scratch group width, a power of two): the
  // R rows x wc columns of one group are R*wc*16 contiguous, aligned bytes -- strided WRITES need long aligned runs on this
  // memory system -- and pass A later reads its whole tile of wt as one contiguous run.  A sweep of the workgroup covers
  // T/(R*wc) groups = T/R columns; uniform base and LDS address advance by constants from sweep to sweep.
  {
    const bool cm = (wc & 0x100) != 0;       // column-major patches (pass A's tile kernel reads them with a quarter of the L1 accesses)
    wc &= 0xFF;
    const int lw = 31 - __clz(wc);
    const int g0 = cl0 >> lw, g1 = (cl1 + wc - 1) >> lw;
    const int per = R << lw;                 // elements of one group's patch
    const int gstep = T >> (LR + lw);        // groups per sweep (T >= R*wc)
    const int rem = tid & (per - 1);         // this thread's element of the patch = its place in the patch's contiguous bytes
    const int r2 = cm ? (rem & (R - 1)) : (rem >> lw), cc = cm ? (rem >> LR) : (rem & (wc - 1));
    const int gi = tid >> (LR + lw);
    const bool rowok = i0 + r2 < s.dimup;
    int lc = ((g0 + gi) << lw) + cc;         // local column of this thread in the current sweep
    const uint32_t drows = cm ? (uint32_t)((s.dimup + R - 1) & ~(R - 1)) : (uint32_t)s.dimup;  // rows of a group's stretch (whole patches when column-major)
    const uint32_t so = (uint32_t)gi * (drows * per / R * VB) + (uint32_t)rem * VB;
    // LDS byte offset of (column, row); a sweep advances the column by T/R, which leaves its swizzle bits alone
    uint32_t lo = ltile + (uint32_t)(((lc + s.dw0 - cb0) << LTB) + ((r2 << LVB) ^ (int)swz_of((uint32_t)(lc + s.dw0 - cb0))));
    char* __restrict__ dstb = reinterpret_cast<char*>(wt) + ((int64_t)g0 * drows + i0) * ((int64_t)VB << lw);
    const int64_t dstep = (int64_t)gstep * drows * ((int64_t)VB << lw);
    for (int g = g0; g < g1; g += gstep) {
      // streaming store: wt is read back once, by pass A, long after it has left L2; not letting it linger leaves the L2
      // to the tile lines that the out-of-block gathers of the neighbouring workgroups hit (-3 % on pass B, measured)
      if (lc >= cl0 && lc < cl1 && rowok) store_stream(reinterpret_cast<VT*>(dstb + so), lds_ld<VT>(lo));
      lc += gstep << lw;
      lo += T * VB;
      dstb += dstep;
    }
  }
}

// ---------------------------------------------------------------------------------------
// launcher (host; the plan it runs is built in hxv_tile_plan.cpp)
// ---------------------------------------------------------------------------------------
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per kernel and size, not per launch (small sectors are launch-bound)
hipError_t allow_dynamic_lds(const void* kern, int bytes) {
  static std::mutex mu;
  static std::map<const void*, int> granted;
  std::lock_guard<std::mutex> lk(mu);
  int& g = granted[kern];
  if (bytes <= g) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) g = bytes;
  return e;
}

namespace {

template <int C, int LZ, typename VT>
hipError_t launch_up_lz(const DevSector& s, const DevTiles& t, int lds_bytes, int threads, bool norb1, int wc, const VT* v,
                        const VT* wt, VT* hv, const LzEpilogue& lz, hipStream_t st) {
  const int ngroups = (s.qdw + C - 1) / C;
  const int gpx = (ngroups + 7) / 8;
  const int64_t nwg = (int64_t)gpx * 8 * t.nblocks;
  using Kern = void (*)(DevSector, DevTiles, const VT*, const VT*, VT*, int, int, int, LzEpilogue);
  constexpr bool cplx = std::is_same<VT, double2>::value;
  constexpr bool pair_built = cplx && C <= 4;         // paired epilogue: real H on complex vectors only
  constexpr bool nd_built = pair_built && LZ != 2;    // (the spH0nd block rides along on complex vectors, never with the paired epilogue)
  if (LZ == 2 && !(pair_built && s.real_h)) return hipErrorInvalidValue;
  const bool p16 = t.ell16 != nullptr;          // (the half-size in-block table exists)
  const bool nd = nd_folds(s) && !norb1;        // (Norb > 1: never the one-orbital diagonal)
  // (plain = without the spH0nd block; the arguments in the order that emits the kernels as the written-out choice did: same code object)
  const Kern kern = with_bools(
      [](auto plain, auto real, auto p, auto n1) -> Kern {
        constexpr bool ND = !decltype(plain)::value, REAL = decltype(real)::value, P16 = decltype(p)::value, NORB1 = decltype(n1)::value;
        if constexpr ((LZ == 2 && !pair_built) || (!REAL && (!cplx || LZ == 2)) || (ND && (NORB1 || !nd_built)))
          return nullptr;  // (not built, and never asked for: real vectors exist for real H only)
        else
          return hxv_pass_up<C, REAL, NORB1, LZ, P16, VT, ND>;
      },
      !(nd_built && nd), !cplx || s.real_h, p16, norb1);
  lds_bytes = std::max(lds_bytes, 32 * 8);  // the epilogue reduces through LDS: 16 (+16 paired) doubles
  hipError_t e = allow_dynamic_lds((const void*)kern, lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(threads), (size_t)lds_bytes, st, s, t, v, wt, hv, ngroups, gpx, wc, lz);
  return hipGetLastError();
}

template <int C, typename VT>
hipError_t launch_up(const DevSector& s, const DevTiles& t, int lds_bytes, int threads, bool norb1, int wc, const VT* v,
                     const VT* wt, VT* hv, const LzEpilogue* lz, hipStream_t st) {
  if (lz && lz->pair) return launch_up_lz<C, 2, VT>(s, t, lds_bytes, threads, norb1, wc, v, wt, hv, *lz, st);
  if (lz) return launch_up_lz<C, 1, VT>(s, t, lds_bytes, threads, norb1, wc, v, wt, hv, *lz, st);
  return launch_up_lz<C, 0, VT>(s, t, lds_bytes, threads, norb1, wc, v, wt, hv, LzEpilogue(), st);
}

// Which instantiations of pass B are built with the out-of-block sums in registers (hxv_pass_dw, ORD 1): up to four pairs per thread
// (eight would be 32 registers of sums), and only where the kernel stays within the 64 vector registers of two 1024-thread workgroups
// per CU without a spill (-Rpass-analysis=kernel-resource-usage; the table is in LABNOTES.md)
template <int R, int NP, bool REAL, typename VT>
constexpr bool dw_regs_built() {
  constexpr bool cplx = std::is_same<VT, double2>::value;
  if (NP > 4) return false;
  if (cplx && R == 8 && (NP == 4 || (NP == 2 && !REAL))) return false;  // 8 - 12 spilled vector registers (NP 4), 2 - 3 (NP 2, complex H)
  if (cplx && R == 2 && NP == 4 && !REAL) return false;                 // 2 spilled with the half-size in-block table
  return true;
}

template <int R, int NP, bool REAL, typename VT, int ORD>
auto dw_kernel(bool p16) -> void (*)(DevSector, DevTiles, const VT*, VT*, int, int, int) {
  if constexpr (ORD == 0 || dw_regs_built<R, NP, REAL, VT>())
    return p16 ? hxv_pass_dw<R, NP, REAL, true, VT, ORD> : hxv_pass_dw<R, NP, REAL, false, VT, ORD>;
  else
    return nullptr;
}

template <int R, int NP, int ORD, typename VT>
hipError_t launch_dw_ord(const DevSector& s, const DevTiles& t, int lds_bytes, int threads, int wc, const VT* v, VT* hv,
                         hipStream_t st) {
  const int ngroups = (s.dimup + R - 1) / R;
  const int gpx = (ngroups + 7) / 8;
  const int64_t nwg = (int64_t)((gpx + 1) & ~1) * 8 * t.nblocks;  // (an even number of row groups per XCD: DevTiles::pair_rows)
  void (*kern)(DevSector, DevTiles, const VT*, VT*, int, int, int);
  const bool p16 = t.ell16 != nullptr;  // (the half-size in-block table exists: blocks <= 1024 columns, <= 64 signed coefficients)
  if constexpr (std::is_same<VT, double>::value)
    kern = dw_kernel<R, NP, true, double, ORD>(p16);
  else if (s.real_h)
    kern = dw_kernel<R, NP, true, double2, ORD>(p16);
  else
    kern = dw_kernel<R, NP, false, double2, ORD>(p16);
  if (!kern) return hipErrorInvalidValue;  // (an order that is not built for this instantiation: launch_dw_np does not ask for it)
  hipError_t e = allow_dynamic_lds((const void*)kern, lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(threads), (size_t)lds_bytes, st, s, t, v, hv, ngroups, gpx, wc);
  return hipGetLastError();
}

// The order of pass B's phases for one launch (hxv_pass_dw, ORD).  The register order needs the store's thread-to-pair mapping: natural
// layout or column-major patches, and room for the up to wc-1 dead column positions in front of a block in the NP sweeps of a workgroup.
template <int R, int NP, typename VT>
hipError_t launch_dw_np(const DevSector& s, const DevTiles& t, int max_block, int lds_bytes, int threads, int wc, const VT* v, VT* hv,
                        hipStream_t st, int* order_ran) {
  const bool regs_built = std::is_same<VT, double>::value ? dw_regs_built<R, NP, true, VT>()
                                                          : (s.real_h ? dw_regs_built<R, NP, true, VT>() : dw_regs_built<R, NP, false, VT>());
  const int wcw = wc & 0xFF;
  const bool mapped = wc == 0 || (wc & 0x100) != 0;
  const bool fits = (int64_t)(max_block + (wcw ? wcw - 1 : 0)) * R <= (int64_t)NP * threads;
  const int ord = (regs_built && mapped && fits && !(t.debug & 8192)) ? 1 : 0;
  if (order_ran) *order_ran = ord;
  if constexpr (NP <= 4) {
    if (ord == 1) return launch_dw_ord<R, NP, 1, VT>(s, t, lds_bytes, threads, wc, v, hv, st);
  }
  return launch_dw_ord<R, NP, 0, VT>(s, t, lds_bytes, threads, wc, v, hv, st);
}

template <int R, typename VT>
hipError_t launch_dw(const DevSector& s, const DevTiles& t, int max_block, int lds_bytes, int threads, int wc, const VT* v,
                     VT* hv, hipStream_t st, int* order_ran) {
  const int np = (max_block * R + threads - 1) / threads;  // <= R because max_block <= threads
  if (np <= 1) return launch_dw_np<R, 1, VT>(s, t, max_block, lds_bytes, threads, wc, v, hv, st, order_ran);
  if (np <= 2) return launch_dw_np<R, 2, VT>(s, t, max_block, lds_bytes, threads, wc, v, hv, st, order_ran);
  if (np <= 4) return launch_dw_np<R, 4, VT>(s, t, max_block, lds_bytes, threads, wc, v, hv, st, order_ran);
  return launch_dw_np<R, 8, VT>(s, t, max_block, lds_bytes, threads, wc, v, hv, st, order_ran);
}

}  // namespace


// The kernels' view of one spin's tables.  The block order (TileOptions::block_order): automatic = by the particle number of the high
// orbitals where table classes are few (it IS a class order there, and it keeps coupled blocks close: Ns=18 fabric traffic 330 -> 261 GB
// per product, 73.1 -> 70.1 ms; Ns=16 -0.8 %; profiles/r04_ab_block_order.log), natural otherwise (11 table sets for 16 blocks, C4: 2.6 %
// faster).  wtr / nwtr: pass A's dw part in row ranges (up spin only).
static DevTiles dev_tiles(const SpinTiles& t, const double2* scoef, int ncoef, const TileOptions& opt, const WtRange* wtr = nullptr, int nwtr = 0) {
  int bo = opt.block_order;
  if (opt.debug & 32) bo = 2;
  if (bo < 0) bo = 2 * t.table_classes <= t.nblocks ? 1 : 2;
  DevTiles d{};
  d.start = t.d_start;
  d.tstart = t.d_tstart;
  d.perm = t.d_perm;
  d.gstart = t.d_gstart;
  d.gmax = t.d_gmax;
  d.ell_in = t.d_ell_in;
  d.ell16 = t.d_ell16;
  d.scoef = scoef;
  d.bh_ptr = t.d_bh_ptr;
  d.bh = t.d_bh;
  d.rs_ptr = t.d_rs_ptr;
  d.rs_off = t.d_rs_off;
  d.rs_tab = t.d_rs_tab;
  d.rs_base = t.d_rs_base;
  d.rs_neg = t.d_rs_neg;
  d.nblocks = t.nblocks;
  d.nscoef = 2 * ncoef + 1;
  d.debug = opt.debug;
  d.pair_rows = 0;  // (pass B: set by the launcher, once the tile's row count is known)
  d.order = bo == 0 ? t.d_order : (bo == 1 ? t.d_order_pc : nullptr);
  d.p16_bits = t.p16_bits;
  d.rs16 = (t.rs16_on && !(opt.debug & 64)) ? t.d_rs16 : nullptr;
  d.rs16_off = t.d_rs16_off;
  d.wtr = wtr;
  d.nwtr = nwtr;
  return d;
}

template <typename VT>
static hipError_t launch_tiled_vt(const DevSector& s, const TilePlan& plan, const VT* v, VT* wt, VT* hv, hipStream_t st, const LzEpilogue* lz,
                                  int only_pass, bool wt_natural, const WtRange* wtr = nullptr, int nwtr = 0) {
  constexpr bool RV = std::is_same<VT, double>::value;
  const DevTiles tu = dev_tiles(plan.up, plan.d_scoef_up, plan.ncoef_up, plan.opt, wtr, nwtr);
  DevTiles td = dev_tiles(plan.dw, plan.d_scoef_dw, plan.ncoef_dw, plan.opt);
  const int C = RV ? real_cols(plan) : cplx_cols(plan), R = RV ? real_rows(plan) : plan.opt.rows_per_tile;
  // columns per group of the wt scratch; 0 = natural layout
  const int passes = only_pass ? only_pass : plan.opt.passes;
  {
    // (only tiles whose column segments are half lines have a neighbour to pair with)
    const int64_t panel_pair = (int64_t)2 * R * (int)sizeof(VT) * s.dimdw;  // bytes of the lines two neighbouring row groups share
    td.pair_rows = plan.opt.pair_rows < 0 ? ((R * (int)sizeof(VT) < 128 && panel_pair > ((int64_t)4 << 20)) ? 1 : 0) : plan.opt.pair_rows;
  }
  // (with the job kernels pass A's tile width no longer constrains the scratch layout)
  int wc = wt_natural ? 0 : (RV ? real_wc(plan) : std::max(C, plan.opt.wt_cols));
  bool job_a = false;
  if constexpr (!RV) job_a = (passes & 1) && !wtr && use_job_up(s, plan, false, lz != nullptr, wt_natural, &wc);  // (a dw part in pieces: tile kernel)
  // (folded spH0nd block: one table row index and 2*C partner-column words per ordered orbital pair of a site, behind the coefficients)
  const int lds_nd = nd_folds(s) ? s.nd.nlat * s.nd.norb * (s.nd.norb - 1) * (2 * C + 1) * 4 : 0;
  const int lds_a = std::max(plan.up.max_block * C * (int)sizeof(VT) + tu.nscoef * 16 + lds_nd, plan.opt.lds_min_kb_up * 1024);
  const int lds_b = std::max(plan.dw.max_block * R * (int)sizeof(VT) + ((td.nscoef * 16 + 255) & ~255), plan.opt.lds_min_kb_dw * 1024);
  const int ta = plan.opt.threads_up, tb = plan.opt.threads_dw;
  const bool norb1 = s.diag.mode == 0 && s.diag.cross.norb == 1;
  hipError_t e = hipSuccess;
  // REAL vectors: pass B treats rows as independent batch entries (the dw hops act on columns), so a real vector IS a complex vector of
  // DimUp/2 rows with real coefficients: the complex kernel does one table decode and one 16-byte LDS gather where the double kernel
  // does two of each (round 5: 1.23 -> ~1.0 ms at C3; option "real_dw_pairs").  With column-major patches the scratch it writes is the
  // real kernel's own layout (a pair of rows = two rows of a patch); natural-layout outputs (row panels of exchange mode 2) likewise.
  bool dw_pairs = false;
  if constexpr (RV) dw_pairs = plan.opt.real_dw_pairs && (passes & 2) && (s.pitch % 2 == 0);
  // blocked scratch: column-major patches for the tile kernels (pass A reads them with a quarter of the L1 accesses); the job kernel's
  // group buffers keep the row-major patches.  Row pairs need them (their scratch would otherwise interleave the two rows of a pair).
  const bool cm = wc > 0 && !job_a && (plan.opt.wt_colmajor || dw_pairs);
  const int wc_b = wc_pass_b(wc, cm);
  if (passes & 2) {
    if constexpr (RV) {
      if (dw_pairs) {
        DevSector sp = s;
        sp.dimup = (s.dimup + 1) / 2;
        sp.pitch = s.pitch / 2;
        const double2* v2 = reinterpret_cast<const double2*>(v);
        double2* w2 = reinterpret_cast<double2*>(wt);
        if (R == 4)
          e = launch_dw<2, double2>(sp, td, plan.dw.max_block, lds_b, tb, wc_b, v2, w2, st, &plan.dw_order_last);
        else
          e = launch_dw<4, double2>(sp, td, plan.dw.max_block, lds_b, tb, wc_b, v2, w2, st, &plan.dw_order_last);
      }
    }
    if (!dw_pairs) switch (R) {
        case 2: e = launch_dw<2, VT>(s, td, plan.dw.max_block, lds_b, tb, wc_b, v, wt, st, &plan.dw_order_last); break;
        case 4: e = launch_dw<4, VT>(s, td, plan.dw.max_block, lds_b, tb, wc_b, v, wt, st, &plan.dw_order_last); break;
        default: e = launch_dw<8, VT>(s, td, plan.dw.max_block, lds_b, tb, wc_b, v, wt, st, &plan.dw_order_last); break;
      }
  }
  if (e != hipSuccess) return e;
  const int wc_a = wc_pass_a(wc, cm ? R : 0);  // (patch rows in pass A's element units -- R real rows also when pass B ran on R/2 row pairs)
  const VT* wta = ((passes & 2) || only_pass == 1) ? wt : nullptr;
  if constexpr (!RV) {
    if (job_a) return launch_up_job(s, plan, tu, wc_a, v, wta, hv, lz, st);
  }
  if (passes & 1) switch (C) {
      case 2: e = launch_up<2, VT>(s, tu, lds_a, ta, norb1, wc_a, v, wta, hv, lz, st); break;
      case 4: e = launch_up<4, VT>(s, tu, lds_a, ta, norb1, wc_a, v, wta, hv, lz, st); break;
      default:
        if constexpr (RV)
          e = launch_up<8, VT>(s, tu, lds_a, ta, norb1, wc_a, v, wta, hv, lz, st);
        else
          e = hipErrorInvalidValue;  // (cplx_cols)
        break;
    }
  return e;
}

hipError_t launch_hxv_tiled(const DevSector& s, const TilePlan& plan, const double2* v, double2* wt, double2* hv, hipStream_t st,
                            const LzEpilogue* lz, int only_pass, bool wt_natural, const WtRange* wtr, int nwtr) {
  // wt: scratch of tiled_wt_elems() elements (dw-hop part, column-group-blocked), owned by the handle
  if (s.qdw == 0) return hipSuccess;
  return launch_tiled_vt<double2>(s, plan, v, wt, hv, st, lz, only_pass, wt_natural, wtr, nwtr);
}

hipError_t launch_hxv_tiled_real(const DevSector& s, const TilePlan& plan, const double* v, double* wt, double* hv, hipStream_t st,
                                 const LzEpilogue* lz, int only_pass, bool wt_natural, const WtRange* wtr, int nwtr) {
  // REAL vectors (H real; s.pitch must be the real pitch, a multiple of 16): wt needs no more bytes than in complex mode
  if (s.qdw == 0) return hipSuccess;
  if (!s.real_h) return hipErrorInvalidValue;
  return launch_tiled_vt<double>(s, plan, v, wt, hv, st, lz, only_pass, wt_natural, wtr, nwtr);
}

}  // namespace hxv
