// Twin-sector map of a device-resident state (include/hxv.h: hxv_twin_vector).
//
// With ed_twin the reference solves one sector of every pair A = (nup,ndw), B = (ndw,nup) (ED_SETUP.f90:353-362), stores each eigenstate once
// with a twin link (ED_DIAG.f90:84,231) and rebuilds B's vector on demand, vector(i) = cvec(Order(i)) (es_return_cvector,
// ED_EIGENSPACE.f90:485-494).  Order (twin_sector_order, ED_SETUP.f90:854-898) is the argsort of the spin-flipped Fock states; with A's index
// iup + idw*DimUp_A and B's iup' + idw'*DimUp_B, iup' = idw, idw' = iup, that is the plain transpose of the DimUp x DimDw amplitude matrix,
//     v_B[idw_A + iup_A*DimDw_A] = v_A[iup_A + idw_A*DimUp_A],
// without a sign.  On device vectors (columns padded to the pitch, rows in each sector's device row order, basis signs by device row):
//     d_B[kB*pitch_B + rB] = sB[rB] * sA[rA] * d_A[kA*pitch_A + rA],     kB = iperm_A[rA],  kA = iperm_B[rB].
//   twin_transpose_kernel  one workgroup per tile of TW device rows of A by TW device rows of B, through LDS.  A tile row of the load is a
//                      run of TW elements inside ONE column of A (column iperm_B[rB]), a tile row of the store a run of TW elements inside
//                      ONE column of B (column iperm_A[rA]): both sides move whole 128-byte lines (TW and both pitches are multiples of 8),
//                      whatever the two row orders are.  Pad rows of d_A are never read; every element of d_B is written, its pad rows with
//                      zeros (the last tile along rB reaches pitch_B).  Only moves and +-1: the same input gives the same bits.
//
// SPLIT SECTORS (both handles rank r of P > 1).  A's slab holds the columns idw in [fa[r], fa[r+1]) of A, B's slab the columns kB in
// [fb[r], fb[r+1]) of B, i.e. the REFERENCE up-rows of A in that range (DimDw_B = DimUp_A, both split by dw_split): the twin of a DimDw split
// is a DimUp split, one all-to-all.  The reference gathers the whole vector on the master and permutes there (es_return_cvector_mpi,
// ED_EIGENSPACE.f90:498-569).  Here: one collective step between two kernels, every number of it from twin_split_plan (hxv_sector.cpp).
//   block r -> q       [iup in fb[q]..fb[q+1))[idw in fa[r]..fa[r+1)), reference order both ways, idw fastest, rows S(r) = roundup8(qdw_A(r))
//                      elements apart (every block row starts on a 128-byte line; the stride pads are never written and never read).  The
//                      blocks towards q = 0..P-1 follow each other in the send buffer, so the row of reference row iup starts at iup * S(r):
//                      the packer needs no owner table, only its own range [fb[r], fb[r+1)) -- that block goes straight to its place in the
//                      receive buffer and never through the exchange.
//   twin_pack_kernel   the tile of twin_transpose_kernel (TW x TW through LDS, the same 33-slot rows and conflict-free accesses).  Loads: runs
//                      of TW device rows of A inside one local column; stores: runs of TW local columns inside the block row of iup =
//                      iperm_A[rA].  sA is applied here.  Pad rows of d_psi are never read.
//   exchange           one comm_sendrecv_cols on `to`'s communicator, offsets in elements (cb = 16 bytes).
//   twin_unpack_kernel for local column kB and device row rB of B: idw = iperm_B[rB], o = owner of idw in A's split (a table of P+1 firsts,
//                      counted through with a uniform trip count), d_out = sB * recv_o[kB * S(o) + idw - fa[o]]; stores coalesced along rB,
//                      rows DimUp_B <= rB < pitch_B written as zero.  No LDS: the gathers of one (kB, block of rB) stay inside P block rows.
// All element offsets are int64 (a C5 slab is more than 2^31 bytes); both grids loop over their y extent instead of exceeding 65535.
#include <hip/hip_runtime.h>

#include "hxv_call_scope.hpp"
#include "hxv_twin_kernels.hpp"

using namespace hxv;

namespace {
// both handles rank r of the same P > 1, `to` bound to a communicator, the pair checked: pack, one exchange, unpack (see the head of the file)
int twin_vector_split(hxv_handle* from, hxv_handle* to, const void* d_psi, void* d_out) {
  const SectorHost &a = from->host, &b = to->host;
  const int P = b.nranks, r = b.rank;
  std::vector<int64_t> sc(P), rc(P);
  if (!twin_split_plan(a.dimup, a.dimdw, r, P, sc.data(), rc.data()))
    return fail(HXV_ERR_STATE, "hxv_twin_vector: no split plan for this pair (nranks > min(DimUp, DimDw))");
  if (a.qdw < 1 || b.qdw < 1) return fail(HXV_ERR_STATE, "hxv_twin_vector: a rank without columns");
  // offsets in elements; the own entries keep their place in both buffers (comm_sendrecv_cols skips the own rank)
  std::vector<int64_t> send_ptr(P + 1, 0), recv_ptr(P + 1, 0), tab(3 * (size_t)P + 2, 0);
  for (int p = 0; p < P; ++p) {
    int q, c0;
    dw_split(a.dimdw, p, P, q, c0);
    send_ptr[p + 1] = send_ptr[p] + sc[p];
    recv_ptr[p + 1] = recv_ptr[p] + rc[p];
    tab[p] = c0;
    tab[P + 1 + p] = recv_ptr[p];
    tab[2 * P + 2 + p] = rc[p] / b.qdw;
  }
  tab[P] = a.dimdw;
  tab[2 * P + 1] = recv_ptr[P];
  const int64_t stride = sc[r] / b.qdw;
  // what the packer's addressing rests on: the plan's blocks follow each other by reference row, and this handle's slabs are the plan's
  if (stride < a.qdw || send_ptr[P] != (int64_t)a.dimup * stride || send_ptr[r] != (int64_t)b.dw0 * stride ||
      rc[r] != sc[r] || tab[r] != a.dw0)
    return fail(HXV_ERR_STATE, "hxv_twin_vector: the split plan does not match the handles' slabs");
  HIPCHK(hipSetDevice(to->device));
  hipStream_t st = to->stream;
  double2 *d_send = nullptr, *d_recv = nullptr;
  int64_t* d_tab = nullptr;
  int rc_local = HXV_OK;
  CallScope scratch(to);
  hipError_t e1 = scratch.take((size_t)send_ptr[P] * sizeof(double2), &d_send);
  hipError_t e2 = scratch.take((size_t)recv_ptr[P] * sizeof(double2), &d_recv);
  hipError_t e3 = scratch.take_device(tab.size() * sizeof(int64_t), &d_tab);
  if (e3 == hipSuccess) e3 = hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(int64_t), hipMemcpyHostToDevice, st);
  for (auto& ev : to->tw_ev)
    if (!ev && e3 == hipSuccess) e3 = hipEventCreate(&ev);
  if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
    (void)hipGetLastError();
    rc_local = fail(HXV_ERR_HIP, "hxv_twin_vector: staging buffers and table of the split map");
  }
  int rcx = comm_agree(to, rc_local);
  if (rcx) return rcx;
  auto step_failed = [&](const char* what, hipError_t e) {
    return fail(HXV_ERR_HIP, std::string("hxv_twin_vector: ") + what + ": " + hipGetErrorString(e));
  };
  hipError_t e = hipEventRecord(to->tw_ev[0], st);
  if (e != hipSuccess) return step_failed("event", e);
  {
    const unsigned gx = (unsigned)((a.dimup + TW - 1) / TW), gy = (unsigned)std::min((a.qdw + TW - 1) / TW, 65535);
    hipLaunchKernelGGL(twin_pack_kernel, dim3(gx, gy), dim3(TW_THREADS), 0, st, (const double2*)d_psi, a.dimup, a.pitch, a.qdw, from->dev.up_iperm,
                       from->dev.up_sign, d_send, d_recv + recv_ptr[r], (int)stride, b.dw0, b.dw0 + b.qdw);
    e = hipGetLastError();
    if (e != hipSuccess) return step_failed("pack kernel", e);
  }
  (void)hipEventRecord(to->tw_ev[1], st);
  rcx = comm_sendrecv_cols(to, d_send, send_ptr.data(), d_recv, recv_ptr.data(), sizeof(double2), st);
  if (rcx) return rcx;
  (void)hipEventRecord(to->tw_ev[2], st);
  {
    const unsigned gx = (unsigned)((b.pitch + TW_THREADS - 1) / TW_THREADS), gy = (unsigned)std::min(b.qdw, 65535);
    hipLaunchKernelGGL(twin_unpack_kernel, dim3(gx, gy), dim3(TW_THREADS), 0, st, (const double2*)d_recv, (const int64_t*)d_tab, P, (double2*)d_out,
                       b.dimup, b.pitch, b.qdw, to->dev.up_iperm, to->dev.up_sign);
    e = hipGetLastError();
    if (e != hipSuccess) return step_failed("unpack kernel", e);
  }
  (void)hipEventRecord(to->tw_ev[3], st);
  e = hipStreamSynchronize(st);
  if (e != hipSuccess) return step_failed("synchronise", e);
  for (int i = 0; i < 3; ++i) {
    float ms = 0.f;
    to->twin_last_us[i] = hipEventElapsedTime(&ms, to->tw_ev[i], to->tw_ev[i + 1]) == hipSuccess ? (int64_t)(ms * 1e3f + 0.5f) : -1;
  }
  return HXV_OK;
}
}  // namespace

extern "C" {

int hxv_twin_split_plan(int32_t dimup_a, int32_t dimdw_a, int32_t rank, int32_t nranks, int64_t* send_counts, int64_t* recv_counts) {
  if (!twin_split_plan(dimup_a, dimdw_a, rank, nranks, send_counts, recv_counts))
    return fail(HXV_ERR_ARG, "hxv_twin_split_plan: bad argument (dimensions >= 1, 0 <= rank < nranks <= min(dimup_a, dimdw_a), counts not NULL)");
  return HXV_OK;
}

int hxv_twin_vector(hxv_handle* from, hxv_handle* to, const void* d_psi, void* d_out) {
  if (!from || !to || !d_psi || !d_out) return fail(HXV_ERR_ARG, "hxv_twin_vector: NULL argument");
  const SectorHost &a = from->host, &b = to->host;
  if (a.map_up.empty() || a.map_dw.empty() || b.map_up.empty() || b.map_dw.empty() || a.panel_rows > 0 || b.panel_rows > 0)
    return fail(HXV_ERR_STATE, "hxv_twin_vector needs handles built from a model (basis maps)");
  if (from->device != to->device) return fail(HXV_ERR_ARG, "hxv_twin_vector: handles on different devices");
  if (d_out == d_psi) return fail(HXV_ERR_ARG, "hxv_twin_vector: d_out must not be d_psi (the map is not done in place)");
  const bool split = a.nranks > 1 && a.nranks == b.nranks && a.rank == b.rank;
  if (!split && (a.nranks > 1 || b.nranks > 1 || comm_ready(from) || comm_ready(to)))
    return fail(HXV_ERR_UNSUPPORTED, "hxv_twin_vector: split sectors are not supported unless both handles are the same rank of the same split "
                                     "(and an unsplit pair bound to a communicator is not): the twin of a DimDw split is a DimUp split of the same ranks");
  if (a.ns != b.ns || b.nup != a.ndw || b.ndw != a.nup || b.dimup != a.dimdw || b.dimdw != a.dimup)
    return fail(HXV_ERR_ARG, "hxv_twin_vector: `to` is not the twin sector (ndw,nup) of `from`");
  if (split) {
    if (!comm_ready(to)) return fail(HXV_ERR_STATE, "hxv_twin_vector on a split sector needs `to` bound to a communicator (hxv_comm_init / hxv_comm_init_local)");
    return twin_vector_split(from, to, d_psi, d_out);
  }
  HIPCHK(hipSetDevice(to->device));
  hipStream_t st = to->stream;
  const unsigned gx = (unsigned)((a.dimup + TW - 1) / TW), gy = (unsigned)((b.pitch + TW - 1) / TW);
  if (gy > 65535u) return fail(HXV_ERR_UNSUPPORTED, "hxv_twin_vector: more than 65535 tiles along the target's rows");
  hipLaunchKernelGGL(twin_transpose_kernel, dim3(gx, gy), dim3(TW_THREADS), 0, st, (const double2*)d_psi, a.dimup, a.pitch, from->dev.up_iperm,
                     from->dev.up_sign, (double2*)d_out, b.dimup, b.pitch, to->dev.up_iperm, to->dev.up_sign);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("twin kernel: ") + hipGetErrorString(e));
  HIPCHK(hipStreamSynchronize(st));
  return HXV_OK;
}

}  // extern "C"
