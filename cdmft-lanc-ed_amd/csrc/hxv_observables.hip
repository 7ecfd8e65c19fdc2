// Impurity observables of a device-resident state (include/hxv.h: hxv_observables_accumulate).
//
// Every quantity of the reference's lanc_observables / lanc_local_energy and the single-particle density matrix of
// density_matrix_impurity (ED_OBSERVABLES.f90:94-236, 246-452, 609-686) is a function of one small RAW RECORD per state:
//   W[a_up + 2^Nimp a_dw] = sum |psi(iup,idw)|^2 over the basis states whose impurity bits (the low Nimp bits of each spin's
//                           configuration, ED_OBSERVABLES.f90:540-556) are a_up and a_dw;
//   R_s(is,js)            = sum sgn * psi_i * conj(psi_j),  |j> = c^+_is c_js |i>  (same spin s; is < js on the device, the host fills
//                           R_s(js,is) = conj R_s(is,js));  R_s(is,is) from W.
// Four kernels compute it without floating-point atomics, in a fixed order (the same vector gives the same bits on every call):
//   obs_rows_kernel<false>, obs_rows_kernel<true>, obs_rdw_kernel
//                      one workgroup per local column c -> colout[c][g], g over Gtot = 2^Nimp + 2*Nimp^2 groups:
//                        g <  2^Nimp           sum |psi(r,c)|^2 over the device rows r whose up impurity bits are g
//                        g in R_up block       sum sgn * psi(a,c) * conj(psi(b,c)) over the row pairs of impurity pair p
//                                              (partner row in the same column: the access pattern of the product's up hops)
//                        g in R_dw block       sgn * <psi(:,c'), psi(:,c)>  for the column c' = c^+_is c_js c (whole columns, as the
//                                              dw-hop pass; c' may live on another rank: then it is read from a gathered copy)
//   obs_reduce_kernel  one workgroup per record element: W(a_up,a_dw) sums colout[c][a_up] over the columns with dw bits a_dw,
//                      R(p) sums colout[c][p] over every local column; per-thread strided sums + a fixed-order tree.
// The pair and bin tables are built on the host in device-row numbering (the basis signs of the device row order folded into the
// pair's sign) and cached with the sector image.  On a split sector every rank reduces its columns and the record is all-reduced.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "hxv_call_scope.hpp"

using namespace hxv;

namespace {
struct ObsTables : DeviceTables {
  int nimp = 0, nw = 0, np = 0, gtot = 0;
  int64_t nent = 0, ndwp = 0;
  // up side (rows of one column): groups [seg_ptr[g], seg_ptr[g+1]) of (row_a, row_b, sign), g < nw: W bins (row_a == row_b), then np pair groups
  int32_t *seg_ptr = nullptr, *ent_a = nullptr, *ent_b = nullptr;
  int8_t* ent_s = nullptr;
  // dw side (local columns): pairs [dwp_ptr[c], dwp_ptr[c+1]) of (partner column slot, pair index, sign); columns by dw impurity bits
  int32_t *dwp_ptr = nullptr, *dwp_slot = nullptr, *dwp_p = nullptr, *dwbin_ptr = nullptr, *dwbin_cols = nullptr;
  int8_t* dwp_s = nullptr;
};
constexpr int OBS_THREADS = 256;
constexpr int OBS_WAVES = OBS_THREADS / 64;
constexpr int OBS_MAX_NIMP = 10;  // record of 4^10 + 400 doubles (8 MB); the reference's own cluster_density_matrix is 4^Nimp squared

inline int parity_below(uint32_t m, int bit) { return __builtin_popcount(m & ((1u << bit) - 1u)) & 1; }

// |k> = c^+_is c_js |m> (ED_SETUP.f90 c / cdg: the sign counts the occupied orbitals below the one acted on); false if not applicable
inline bool hop(uint32_t m, int is, int js, uint32_t& k, int& sg) {
  if (!((m >> js) & 1u) || ((m >> is) & 1u)) return false;
  const uint32_t r = m ^ (1u << js);
  sg = (parity_below(m, js) ^ parity_below(r, is)) ? -1 : 1;
  k = r | (1u << is);
  return true;
}

std::string build_tables(const SectorHost& s, int nimp, int device, ObsTables& t) {
  const int nw = 1 << nimp, np = nimp * nimp;
  const uint32_t mask = (uint32_t)nw - 1u;
  t.nimp = nimp;
  t.nw = nw;
  t.np = np;
  t.gtot = nw + 2 * np;
  t.device = device;
  const std::vector<uint32_t>& mdev = s.dev_map_up();  // reference bit strings by device row
  const bool ro = s.row_order();
  std::vector<int32_t> seg_ptr(nw + np + 1, 0), ea, eb;
  std::vector<int8_t> es;
  ea.reserve((size_t)s.dimup * 4);
  eb.reserve((size_t)s.dimup * 4);
  es.reserve((size_t)s.dimup * 4);
  {
    std::vector<std::vector<int32_t>> bins(nw);
    for (int r = 0; r < s.dimup; ++r) bins[mdev[r] & mask].push_back(r);
    for (int g = 0; g < nw; ++g) {
      seg_ptr[g] = (int32_t)ea.size();
      for (int r : bins[g]) {
        ea.push_back(r);
        eb.push_back(r);
        es.push_back(1);
      }
    }
  }
  for (int p = 0; p < np; ++p) {
    const int is = p % nimp, js = p / nimp;
    seg_ptr[nw + p] = (int32_t)ea.size();
    if (is >= js) continue;  // R(js,is) = conj R(is,js): the host fills the lower triangle
    for (int r = 0; r < s.dimup; ++r) {
      uint32_t k;
      int sg;
      if (!hop(mdev[r], is, js, k, sg)) continue;
      const int jref = rank_in(s.map_up, k);
      if (jref < 0) return "observables: a hop target is missing from the up basis";
      const int rb = ro ? s.up_perm[jref] : jref;
      if (ro && (s.up_sign[r] ^ s.up_sign[rb])) sg = -sg;
      ea.push_back(r);
      eb.push_back(rb);
      es.push_back((int8_t)sg);
    }
  }
  seg_ptr[nw + np] = (int32_t)ea.size();
  t.nent = (int64_t)ea.size();
  if (t.nent >= INT32_MAX) return "observables: too many row pairs";
  // dw side: this rank's columns; a partner column owned by rank o sits at slot o*cmax + (its index in o's slab) of the gathered copy,
  // or is read from the slab itself when the sector is not split
  std::vector<int32_t> first(s.nranks + 1, 0);
  for (int p = 0; p < s.nranks; ++p) {
    int q, c0;
    dw_split(s.dimdw, p, s.nranks, q, c0);
    first[p] = c0;
  }
  first[s.nranks] = s.dimdw;
  std::vector<int32_t> dwp_ptr(std::max(s.qdw, 0) + 1, 0), dslot, dp;
  std::vector<int8_t> ds;
  std::vector<std::vector<int32_t>> cbins(nw);
  for (int c = 0; c < s.qdw; ++c) {
    const uint32_t m = s.map_dw[s.dw0 + c];
    cbins[m & mask].push_back(c);
    dwp_ptr[c] = (int32_t)dslot.size();
    for (int p = 0; p < np; ++p) {
      const int is = p % nimp, js = p / nimp;
      if (is >= js) continue;  // (as the up side)
      uint32_t k;
      int sg;
      if (!hop(m, is, js, k, sg)) continue;
      const int cj = rank_in(s.map_dw, k);
      if (cj < 0) return "observables: a hop target is missing from the dw basis";
      int32_t slot = cj;
      if (s.nranks > 1) {
        const int o = (int)(std::upper_bound(first.begin(), first.end(), cj) - first.begin()) - 1;
        slot = o * s.cmax + (cj - first[o]);
      }
      dslot.push_back(slot);
      dp.push_back(p);
      ds.push_back((int8_t)sg);
    }
  }
  dwp_ptr[std::max(s.qdw, 0)] = (int32_t)dslot.size();
  t.ndwp = (int64_t)dslot.size();
  std::vector<int32_t> dwbin_ptr(nw + 1, 0), dwbin_cols;
  for (int g = 0; g < nw; ++g) {
    dwbin_ptr[g] = (int32_t)dwbin_cols.size();
    dwbin_cols.insert(dwbin_cols.end(), cbins[g].begin(), cbins[g].end());
  }
  dwbin_ptr[nw] = (int32_t)dwbin_cols.size();
  TableArena ar;
  (void)ar.add(seg_ptr, &t.seg_ptr);
  (void)ar.add(ea, &t.ent_a);
  (void)ar.add(eb, &t.ent_b);
  (void)ar.add(es, &t.ent_s);
  (void)ar.add(dwp_ptr, &t.dwp_ptr);
  (void)ar.add(dslot, &t.dwp_slot);
  (void)ar.add(dp, &t.dwp_p);
  (void)ar.add(ds, &t.dwp_s);
  (void)ar.add(dwbin_ptr, &t.dwbin_ptr);
  (void)ar.add(dwbin_cols, &t.dwbin_cols);
  hipError_t e = ar.commit(&t.base, &t.bytes);
  if (e != hipSuccess) return std::string("observables tables: ") + hipGetErrorString(e);
  return std::string();
}

__device__ __forceinline__ double2 wave_sum(double2 v) {
  for (int off = 32; off > 0; off >>= 1) {
    v.x += __shfl_xor(v.x, off, 64);
    v.y += __shfl_xor(v.y, off, 64);
  }
  return v;
}

// the same value on every thread of the workgroup: per-wave butterflies, then the waves in order
__device__ __forceinline__ double2 block_sum(double2 v, double2* sh) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  double2 r = sh[0];
  for (int i = 1; i < OBS_WAVES; ++i) {
    r.x += sh[i].x;
    r.y += sh[i].y;
  }
  __syncthreads();
  return r;
}

// One workgroup per local column c of this rank's slab psi [qdw][pitch]; colout[c][g], g over Gtot = nw + 2*np.
// W bins (PAIRS = false, g < nw) and R_up pairs (PAIRS = true, g = nw + p): one wave per group, lanes over the group's rows.
template <bool PAIRS>
__global__ void __launch_bounds__(OBS_THREADS) obs_rows_kernel(const double2* __restrict__ psi, int pitch, int qdw, int nw, int np,
                                                               const int32_t* __restrict__ seg_ptr, const int32_t* __restrict__ ent_a,
                                                               const int32_t* __restrict__ ent_b, const int8_t* __restrict__ ent_s,
                                                               double2* __restrict__ colout) {
  const int c = blockIdx.x;
  if (c >= qdw) return;
  const double2* __restrict__ col = psi + (int64_t)c * pitch;
  double2* __restrict__ out = colout + (int64_t)c * (nw + 2 * np);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g0 = PAIRS ? nw : 0, g1 = PAIRS ? nw + np : nw;
  for (int g = g0 + w; g < g1; g += OBS_WAVES) {
    const int e0 = seg_ptr[g], e1 = seg_ptr[g + 1];
    double2 acc = make_double2(0.0, 0.0);
    if (!PAIRS) {
      for (int e = e0 + lane; e < e1; e += 64) {
        const double2 x = col[ent_a[e]];
        acc.x += x.x * x.x + x.y * x.y;
      }
    } else {
      for (int e = e0 + lane; e < e1; e += 64) {
        const double2 x = col[ent_a[e]], y = col[ent_b[e]];
        const double sg = (double)ent_s[e];
        acc.x += sg * (x.x * y.x + x.y * y.y);  // x * conj(y)
        acc.y += sg * (x.y * y.x - x.x * y.y);
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) out[g] = acc;
  }
}

// R_dw pairs: whole-column products <partner column | this column>; full: the column slots the dw pairs name ([nranks*cmax][pitch] gathered
// copy, or psi itself)
__global__ void __launch_bounds__(OBS_THREADS) obs_rdw_kernel(const double2* __restrict__ psi, const double2* __restrict__ full, int pitch, int dimup,
                                                              int qdw, int nw, int np, const int32_t* __restrict__ dwp_ptr,
                                                              const int32_t* __restrict__ dwp_slot, const int32_t* __restrict__ dwp_p,
                                                              const int8_t* __restrict__ dwp_s, double2* __restrict__ colout) {
  __shared__ double2 sh[OBS_WAVES];
  __shared__ double2 sdw[OBS_MAX_NIMP * OBS_MAX_NIMP];
  const int c = blockIdx.x;
  if (c >= qdw) return;
  const double2* __restrict__ col = psi + (int64_t)c * pitch;
  double2* __restrict__ out = colout + (int64_t)c * (nw + 2 * np);
  for (int i = threadIdx.x; i < np; i += OBS_THREADS) sdw[i] = make_double2(0.0, 0.0);
  __syncthreads();
  for (int k = dwp_ptr[c]; k < dwp_ptr[c + 1]; ++k) {
    const double2* __restrict__ pc = full + (int64_t)dwp_slot[k] * pitch;
    double2 acc = make_double2(0.0, 0.0);
    for (int r = threadIdx.x; r < dimup; r += OBS_THREADS) {
      const double2 x = col[r], y = pc[r];
      acc.x += x.x * y.x + x.y * y.y;
      acc.y += x.y * y.x - x.x * y.y;
    }
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) {
      const double sg = (double)dwp_s[k];
      sdw[dwp_p[k]] = make_double2(sg * acc.x, sg * acc.y);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < np; i += OBS_THREADS) out[nw + np + i] = sdw[i];
}

// rec: [nw*nw] W, then [2*np] R_up, [2*np] R_dw (re, im); R's diagonal is left 0 here (the host fills it from W)
__global__ void __launch_bounds__(OBS_THREADS) obs_reduce_kernel(const double2* __restrict__ colout, int qdw, int nimp, int nw, int np,
                                                                 const int32_t* __restrict__ dwbin_ptr, const int32_t* __restrict__ dwbin_cols,
                                                                 double* __restrict__ rec) {
  __shared__ double2 sh[OBS_WAVES];
  const int64_t o = blockIdx.x;
  const int64_t nww = (int64_t)nw * nw;
  const int gtot = nw + 2 * np;
  double2 acc = make_double2(0.0, 0.0);
  if (o < nww) {
    const int a_up = (int)(o & (nw - 1)), a_dw = (int)(o >> nimp);
    for (int k = dwbin_ptr[a_dw] + threadIdx.x; k < dwbin_ptr[a_dw + 1]; k += OBS_THREADS) acc.x += colout[(int64_t)dwbin_cols[k] * gtot + a_up].x;
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) rec[o] = acc.x;
  } else {
    const int q = (int)(o - nww);  // 0..2np-1: R_up(p), then R_dw(p)
    for (int c = threadIdx.x; c < qdw; c += OBS_THREADS) {
      const double2 v = colout[(int64_t)c * gtot + nw + q];
      acc.x += v.x;
      acc.y += v.y;
    }
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) {
      rec[nww + 2 * q] = acc.x;
      rec[nww + 2 * q + 1] = acc.y;
    }
  }
}
}  // namespace

extern "C" {

int64_t hxv_obs_record_elems(const hxv_handle* h) {
  if (!h || h->host.map_up.empty() || h->host.map_dw.empty() || h->host.panel_rows > 0) return 0;
  const int n = nimp_of(h->host);
  if (n < 1 || n > OBS_MAX_NIMP) return 0;
  return ((int64_t)1 << (2 * n)) + 4 * (int64_t)n * n;
}

int hxv_observables_accumulate(hxv_handle* h, const void* d_psi, double weight, int32_t accumulate, double* record) {
  if (!h || !d_psi || !record) return fail(HXV_ERR_ARG, "hxv_observables_accumulate: NULL argument");
  const SectorHost& s = h->host;
  if (s.map_up.empty() || s.map_dw.empty() || s.panel_rows > 0)
    return fail(HXV_ERR_STATE, "hxv_observables_accumulate needs a handle built from a model (basis maps)");
  const int nimp = nimp_of(s);
  if (nimp < 1 || nimp > s.ns) return fail(HXV_ERR_STATE, "hxv_observables_accumulate: the handle carries no impurity size");
  if (nimp > OBS_MAX_NIMP) return fail(HXV_ERR_UNSUPPORTED, "hxv_observables_accumulate: Nimp > 10 (a record of more than 8 MB)");
  const bool split = s.nranks > 1;
  if (split && !comm_ready(h)) return fail(HXV_ERR_STATE, "hxv_observables_accumulate on a split sector needs the communicator (hxv_comm_init after opening it)");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  // rank-local preparation: tables (once per sector image), scratch; every rank learns whether all could go on
  int rc_local = HXV_OK;
  std::shared_ptr<ObsTables> t;
  rc_local = h->img->tables.get("observables", "", 1, t, [&](std::shared_ptr<ObsTables>& nt) {
    nt = std::make_shared<ObsTables>();
    const std::string err = build_tables(s, nimp, h->device, *nt);
    return err.empty() ? HXV_OK : fail(err.rfind("observables tables", 0) == 0 ? HXV_ERR_HIP : HXV_ERR_STATE, err);
  });
  const int np = nimp * nimp, gtot = (1 << nimp) + 2 * np;
  const int64_t nww = (int64_t)1 << (2 * nimp), nrec = nww + 4 * (int64_t)np;
  double2 *d_col = nullptr, *d_full = nullptr;
  double* d_rec = nullptr;
  CallScope scratch(h);
  if (rc_local == HXV_OK) {
    hipError_t e1 = scratch.take(std::max<size_t>((size_t)s.qdw * gtot, 1) * sizeof(double2), &d_col);
    hipError_t e2 = scratch.take((size_t)nrec * sizeof(double), &d_rec);
    hipError_t e3 = split ? scratch.take(std::max<size_t>((size_t)s.nranks * s.cmax * s.pitch, 1) * sizeof(double2), &d_full) : hipSuccess;
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) rc_local = fail(HXV_ERR_HIP, "hxv_observables_accumulate: scratch buffers");
  }
  int rc = split ? comm_agree(h, rc_local) : rc_local;
  if (rc) return rc;
  const double2* psi = (const double2*)d_psi;
  if (split) {
    rc = comm_allgather_slab(h, psi, d_full, st);
    if (rc) return rc;
  }
  if (s.qdw > 0) {
    const dim3 grid((unsigned)s.qdw), block(OBS_THREADS);
    hipLaunchKernelGGL(obs_rows_kernel<false>, grid, block, 0, st, psi, s.pitch, s.qdw, t->nw, t->np, t->seg_ptr, t->ent_a, t->ent_b, t->ent_s, d_col);
    hipLaunchKernelGGL(obs_rows_kernel<true>, grid, block, 0, st, psi, s.pitch, s.qdw, t->nw, t->np, t->seg_ptr, t->ent_a, t->ent_b, t->ent_s, d_col);
    hipLaunchKernelGGL(obs_rdw_kernel, grid, block, 0, st, psi, split ? (const double2*)d_full : psi, s.pitch, s.dimup, s.qdw, t->nw, t->np,
                       t->dwp_ptr, t->dwp_slot, t->dwp_p, t->dwp_s, d_col);
  }
  hipLaunchKernelGGL(obs_reduce_kernel, dim3((unsigned)(nww + 2 * np)), dim3(OBS_THREADS), 0, st, (const double2*)d_col, s.qdw, nimp, t->nw,
                     t->np, t->dwbin_ptr, t->dwbin_cols, d_rec);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("observables kernels: ") + hipGetErrorString(e));
  if (split) {
    rc = comm_allreduce_sum(h, d_rec, (size_t)nrec, st);
    if (rc) return rc;
  }
  std::vector<double> raw((size_t)nrec);
  e = hipMemcpyAsync(raw.data(), d_rec, (size_t)nrec * sizeof(double), hipMemcpyDeviceToHost, st);
  scratch.release();  // (synchronises the stream: raw is read below)
  if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("hxv_observables_accumulate: ") + hipGetErrorString(e));
  // R_s(js,is) = conj R_s(is,js): c^+_js c_is is the adjoint of c^+_is c_js, and the device computes is < js only
  for (int spin = 0; spin < 2; ++spin) {
    double* R = raw.data() + nww + 2 * np * spin;
    for (int js = 0; js < nimp; ++js)
      for (int is = js + 1; is < nimp; ++is) {
        R[2 * (is + js * nimp)] = R[2 * (js + is * nimp)];
        R[2 * (is + js * nimp) + 1] = -R[2 * (js + is * nimp) + 1];
      }
  }
  // R_s(is,is) = sum of W over the impurity configurations with orbital is occupied in spin s (ED_OBSERVABLES.f90:633-640)
  for (int is = 0; is < nimp; ++is) {
    double up = 0.0, dw = 0.0;
    for (int64_t a = 0; a < nww; ++a) {
      if ((a >> is) & 1) up += raw[a];
      if ((a >> (nimp + is)) & 1) dw += raw[a];
    }
    raw[nww + 2 * (is + is * nimp)] = up;
    raw[nww + 2 * np + 2 * (is + is * nimp)] = dw;
  }
  for (int64_t i = 0; i < nrec; ++i) record[i] = accumulate ? record[i] + weight * raw[i] : weight * raw[i];
  return HXV_OK;
}

}  // extern "C"
