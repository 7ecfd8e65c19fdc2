// TEST-ONLY: a launcher for the pass-A job kernel hxv_up_job alone (csrc/hxv_job_kernels.hpp), so that tests/test_gpu_job_kernel.py can run it
// on the synthetic tables, slabs, ring depths and scratch layouts of tests/job_kernel_ref.py, which no sector reaches.  The kernel is the
// header's text, compiled with the engine's flags and linked with the engine's csrc/hxv_tile_plan.cpp for the geometry
// (build_job_kernel_check() of __graft_entry__.py); this library is never linked into libhxv.so.
//
// jkc_geometry makes no device call: it reports what the engine's job_up_geometry / job_up_fits give for the plan numbers.
// jkc_up_job fills DevSector, DevTiles, JobUp (with job_up_geometry) and LzEpilogue from raw device pointers, picks the instantiation the way
// launch_up_job_c / launch_up_job_k of csrc/hxv_jobs.hip do, launches on the null stream, waits and returns the HIP status.  job_debug is
// always 0.  Before any launch it refuses (hipErrorInvalidValue) what the product's gates refuse and what could leave a buffer whatever the
// tables hold; table CONTENTS are not checked here: tests/test_job_kernel_ref_cpu.py walks every index of every case the GPU file runs.
#include "hxv_job_kernels.hpp"

namespace {
using namespace hxv;
constexpr int BAD = (int)hipErrorInvalidValue;

hipError_t grant_lds(const void* kern, int bytes) { return hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); }

// (launch_up_job_k)
template <int LZ, int KIN>
hipError_t launch_k(const DevSector& s, const DevTiles& t, const JobUp& jb, int lds_bytes, int64_t nwg, const LzEpilogue& lz) {
  const bool norb1 = s.diag.cross.norb == 1;
  using Kern = void (*)(DevSector, DevTiles, JobUp, LzEpilogue);
  if (LZ == 2 && !s.real_h) return hipErrorInvalidValue;
  const Kern kern = with_bools(
      [](auto real, auto n1) -> Kern {
        if constexpr (LZ == 2 && !decltype(real)::value)
          return nullptr;
        else
          return hxv_up_job<1, decltype(real)::value, decltype(n1)::value, LZ, KIN, JOB_KO, double2>;
      },
      s.real_h != 0, norb1);
  hipError_t e = grant_lds((const void*)kern, lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(64 * JOB_WAVES), (size_t)lds_bytes, nullptr, s, t, jb, lz);
  return hipGetLastError();
}
// (launch_up_job_c)
template <int LZ>
hipError_t launch_c(const DevSector& s, const DevTiles& t, const JobUp& jb, int lds_bytes, int64_t nwg, const LzEpilogue& lz) {
  if (jb.max_outer > JOB_KO) return hipErrorInvalidValue;
  if (jb.kin_rows <= 20) return launch_k<LZ, 20>(s, t, jb, lds_bytes, nwg, lz);
  return launch_k<LZ, JOB_KIN>(s, t, jb, lds_bytes, nwg, lz);
}

TilePlan plan_of(int nblocks, int max_block, int ncoef, int k_in, int k_in_real, int max_outer, int job_groups, int job_stages) {
  TilePlan plan;
  plan.opt.job_cols = 1;
  plan.opt.job_groups = job_groups;
  plan.opt.job_stages = job_stages;
  plan.opt.job_debug = 0;
  plan.up.nblocks = nblocks;
  plan.up.max_block = max_block;
  plan.up.k_in = k_in;
  plan.up.k_in_real = k_in_real;
  plan.up.max_outer = max_outer;
  plan.ncoef_up = ncoef;
  return plan;
}
bool bad_plan(int qdw, int nblocks, int max_block, int ncoef, int k_in, int k_in_real, int max_outer, int job_groups, int job_stages, int wc, int lz) {
  return qdw < 1 || nblocks < 1 || max_block < 1 || ncoef < 1 || ncoef > TILE_MAX_COEF || k_in < 0 || k_in % 4 != 0 || k_in_real < 0 ||
         k_in_real > k_in || max_outer < 0 || job_groups < 1 || job_groups > 65536 || job_stages < 2 || job_stages > 8 || lz < 0 || lz > 2 ||
         !(wc == 0 || wc == 1 || wc == 2 || wc == 4 || wc == 8 || wc == 16);
}
}  // namespace

extern "C" {

// out[11] = ngroups, gpx, chunks, ns, stage_bytes, wt_bytes, nst, lds_bytes, kin_rows, nwg, job_up_fits
int jkc_geometry(int qdw, int nblocks, int max_block, int ncoef, int k_in, int k_in_real, int max_outer, int job_groups, int job_stages, int wc, int lz,
                 int64_t* out) {
  if (!out || bad_plan(qdw, nblocks, max_block, ncoef, k_in, k_in_real, max_outer, job_groups, job_stages, wc, lz)) return BAD;
  const TilePlan plan = plan_of(nblocks, max_block, ncoef, k_in, k_in_real, max_outer, job_groups, job_stages);
  DevSector s{};
  s.qdw = qdw;
  JobUp jb{};
  int lds = 0;
  int64_t nwg = 0;
  job_up_geometry(s, plan, lz != 0, wc, jb, lds, nwg);
  const int64_t r[11] = {jb.ngroups, jb.gpx, jb.chunks, jb.ns, jb.stage_bytes, jb.wt_bytes, jb.nst, lds, jb.kin_rows, nwg, job_up_fits(s, plan, lz != 0, wc) ? 1 : 0};
  for (int i = 0; i < 11; ++i) out[i] = r[i];
  return 0;
}

struct JkcArgs {
  // DevTiles (device pointers)
  const uint32_t *start, *tstart, *gstart, *gmax, *ell_in, *bh_ptr, *bh, *rs_ptr, *rs_off, *rs_tab, *rs_base, *rs_neg, *order;
  const void* scoef;  // [2*ncoef+1] complex
  // DevSector: separable diagonal
  const double *a_up, *a_dw;
  const uint32_t *map_up, *map_dw;
  // vectors: v [vslots][pitch], wt (may be null), hv [qdw][pitch], xm [qdw][pitch] (may be null)
  const void *v, *wt, *xm;
  void* hv;
  const double* scal;  // [nscal]
  double *partial, *partial2;  // [npartial]
  int32_t dimup, dimdw, pitch, qdw, dw0, slab0, vslots, real_h;
  int32_t nblocks, max_block, ncoef, k_in, k_in_real, max_outer, job_groups, job_stages;
  int32_t wc, lz, i_s, i_c, i_s2, i_c2, nscal, npartial;
  // cross term of the diagonal (CrossParams)
  int32_t norb, nlat;
  double uloc[5];
  double ust;
  uint32_t orbmask[5];
  uint32_t sitemask[16];
};

int jkc_up_job(const JkcArgs* a) {
  if (!a) return BAD;
  if (bad_plan(a->qdw, a->nblocks, a->max_block, a->ncoef, a->k_in, a->k_in_real, a->max_outer, a->job_groups, a->job_stages, a->wc, a->lz)) return BAD;
  // the product's gates (job_up_usable)
  if (a->dimup < 1 || a->dimup >= 65536 || a->max_block > 64 * JOB_LOADER || a->max_block > a->dimup || a->k_in > JOB_KIN || a->max_outer > JOB_KO) return BAD;
  if (a->lz == 2 && !a->real_h) return BAD;
  // shapes
  if (a->pitch < a->dimup || a->dimdw < 1 || a->vslots < 1 || a->dw0 < 0 || (int64_t)a->dw0 + a->qdw > a->dimdw || a->slab0 < 0 ||
      (int64_t)a->slab0 + a->qdw > a->vslots)
    return BAD;
  if (a->norb < 1 || a->norb > 5 || a->nlat < 0 || a->nlat > 16) return BAD;
  // pointers the kernel dereferences
  if (!a->start || !a->tstart || !a->gstart || !a->gmax || !a->ell_in || !a->bh_ptr || !a->bh || !a->rs_ptr || !a->rs_off || !a->rs_tab || !a->rs_base ||
      !a->rs_neg || !a->order || !a->scoef || !a->a_up || !a->a_dw || !a->map_up || !a->map_dw || !a->v || !a->hv)
    return BAD;
  if (a->lz) {
    if (!a->scal || !a->partial || a->nscal < 1 || a->i_s < 0 || a->i_s >= a->nscal || a->i_c < 0 || a->i_c >= a->nscal) return BAD;
    if (a->lz == 2 && (!a->partial2 || a->i_s2 < 0 || a->i_s2 >= a->nscal || a->i_c2 < 0 || a->i_c2 >= a->nscal)) return BAD;
  }
  const TilePlan plan = plan_of(a->nblocks, a->max_block, a->ncoef, a->k_in, a->k_in_real, a->max_outer, a->job_groups, a->job_stages);
  DevSector s{};
  s.dimup = a->dimup;
  s.dimdw = a->dimdw;
  s.pitch = a->pitch;
  s.qdw = a->qdw;
  s.dw0 = a->dw0;
  s.slab0 = a->slab0;
  s.real_h = a->real_h;
  s.diag.mode = 0;
  s.diag.a_up = a->a_up;
  s.diag.a_dw = a->a_dw;
  s.diag.map_up = a->map_up;
  s.diag.map_dw = a->map_dw;
  s.diag.cross.norb = a->norb;
  s.diag.cross.nlat = a->nlat;
  s.diag.cross.ust = a->ust;
  for (int i = 0; i < 5; ++i) {
    s.diag.cross.uloc[i] = a->uloc[i];
    s.diag.cross.orbmask[i] = a->orbmask[i];
  }
  for (int i = 0; i < 16; ++i) s.diag.cross.sitemask[i] = a->sitemask[i];
  const bool lzon = a->lz != 0;
  if (!job_up_fits(s, plan, lzon, a->wc)) return BAD;
  JobUp jb{};
  int lds_bytes = 0;
  int64_t nwg = 0;
  job_up_geometry(s, plan, lzon, a->wc, jb, lds_bytes, nwg);
  if (nwg < 1 || nwg > 65535 * 8 || lds_bytes > 160 * 1024) return BAD;
  if (lzon && a->npartial < nwg) return BAD;
  jb.v = a->v;
  jb.wt = a->wt;
  jb.hv = a->hv;
  jb.wc = a->wc;
  jb.order = a->order;
  jb.debug = 0;
  DevTiles t{};
  t.start = a->start;
  t.tstart = a->tstart;
  t.gstart = a->gstart;
  t.gmax = a->gmax;
  t.ell_in = a->ell_in;
  t.scoef = (const double2*)a->scoef;
  t.bh_ptr = a->bh_ptr;
  t.bh = a->bh;
  t.rs_ptr = a->rs_ptr;
  t.rs_off = a->rs_off;
  t.rs_tab = a->rs_tab;
  t.rs_base = a->rs_base;
  t.rs_neg = a->rs_neg;
  t.nblocks = a->nblocks;
  t.nscoef = 2 * a->ncoef + 1;
  LzEpilogue lz;
  if (lzon) {
    lz.xm = a->xm;
    lz.scal = a->scal;
    lz.i_s = a->i_s;
    lz.i_c = a->i_c;
    lz.partial = a->partial;
    if (a->lz == 2) {
      lz.pair = 1;
      lz.i_s2 = a->i_s2;
      lz.i_c2 = a->i_c2;
      lz.partial2 = a->partial2;
    }
  }
  hipError_t e = a->lz == 2 ? launch_c<2>(s, t, jb, lds_bytes, nwg, lz) : a->lz == 1 ? launch_c<1>(s, t, jb, lds_bytes, nwg, lz) : launch_c<0>(s, t, jb, lds_bytes, nwg, LzEpilogue());
  hipError_t w = hipStreamSynchronize(nullptr);
  return (int)(e != hipSuccess ? e : w);
}

}  // extern "C"
