// Pipelined "job" kernels (gfx950): the same two passes as hxv_tiled.hip, restructured so that the HBM streams, the
// LDS gathers and the out-of-block gathers of a workgroup overlap instead of adding up.
//
//   job of pass A = (up prefix block kb) x (a run of `gc` column groups of C columns).  One 1024-thread workgroup per CU:
//     * wave 15 is the LOADER: it streams the [block] x [C columns] tiles of v and of the dw-hop scratch wt into an LDS
//       ring with LDS-DMA (global_load_lds_dwordx4: no staging registers), NST-1 tiles ahead of the compute waves, paced
//       by counted s_waitcnt vmcnt(N);
//     * waves 0..14 COMPUTE one row of the block per thread.  The per-row hop tables (in-block LDS offsets, out-of-block
//       row slots and block hops) are read ONCE per job into registers, so inside the tile loop a hop costs a decode,
//       one LDS coefficient read, C ds_read_b128 and the FMAs -- no dependent table round trips;
//     * one s_barrier per tile: "tile k+1 has landed" and "tile k's buffer is free" are the same barrier.
//   The out-of-block gathers of a tile are issued first (L2 of this XCD), the in-block LDS phase runs under their
//   latency, then they are consumed.  Workgroups of one chunk of column groups are adjacent in blockIdx (one XCD each),
//   so the blocks a gather reads are being streamed by a neighbour at about the same time.
//
// Reference semantics: ED_HAMILTONIAN_SPARSE_HxV.f90:167-227 (Hv = spH0d.v + spH0ups(1).v + spH0dws(1).v).
#include <algorithm>
#include <type_traits>

#include "hxv_job_kernels.hpp"  // hxv_up_job and its device helpers

namespace hxv {

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
namespace {

template <int C, int LZ, int KIN, int KO>
hipError_t launch_up_job_k(const DevSector& s, const DevTiles& t, const JobUp& jb, int lds_bytes, int64_t nwg, const LzEpilogue& lz,
                           hipStream_t st) {
  const bool norb1 = s.diag.cross.norb == 1;
  using Kern = void (*)(DevSector, DevTiles, JobUp, LzEpilogue);
  if (LZ == 2 && !s.real_h) return hipErrorInvalidValue;  // the paired epilogue exists for real H only
  const Kern kern = with_bools(
      [](auto real, auto n1) -> Kern {
        if constexpr (LZ == 2 && !decltype(real)::value)
          return nullptr;
        else
          return hxv_up_job<C, decltype(real)::value, decltype(n1)::value, LZ, KIN, KO, double2>;
      },
      s.real_h != 0, norb1);
  hipError_t e = allow_dynamic_lds((const void*)kern, lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(64 * JOB_WAVES), (size_t)lds_bytes, st, s, t, jb, lz);
  return hipGetLastError();
}

template <int C, int LZ>
hipError_t launch_up_job_c(const DevSector& s, const DevTiles& t, const JobUp& jb, int lds_bytes, int64_t nwg, const LzEpilogue& lz,
                           hipStream_t st) {
  // fewer table registers when the longest in-block list / the out-of-block slot count allow it
  if (jb.max_outer > JOB_KO) return hipErrorInvalidValue;  // (job_up_usable)
  if (jb.kin_rows <= 20) return launch_up_job_k<C, LZ, 20, JOB_KO>(s, t, jb, lds_bytes, nwg, lz, st);
  return launch_up_job_k<C, LZ, JOB_KIN, JOB_KO>(s, t, jb, lds_bytes, nwg, lz, st);
}

}  // namespace

hipError_t launch_up_job(const DevSector& s, const TilePlan& plan, const DevTiles& tu, int wc, const double2* v, const double2* wt, double2* hv,
                         const LzEpilogue* lz, hipStream_t st) {
  JobUp jb{};
  int lds_bytes = 0;
  int64_t nwg = 0;
  job_up_geometry(s, plan, lz != nullptr, wc, jb, lds_bytes, nwg);
  if (!job_up_fits(s, plan, lz != nullptr, wc)) return hipErrorInvalidValue;
  jb.v = v;
  jb.wt = wt;
  jb.hv = hv;
  jb.wc = wc;
  // (two columns per tile were measured slower, and every such kernel spills vector and scalar registers: not built any more)
  if (plan.opt.job_cols != 1) return hipErrorInvalidValue;
  if (lz && lz->pair) return launch_up_job_c<1, 2>(s, tu, jb, lds_bytes, nwg, *lz, st);
  return lz ? launch_up_job_c<1, 1>(s, tu, jb, lds_bytes, nwg, *lz, st) : launch_up_job_c<1, 0>(s, tu, jb, lds_bytes, nwg, LzEpilogue(), st);
}

}  // namespace hxv
