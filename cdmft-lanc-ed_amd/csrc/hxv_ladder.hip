// c / c^dagger on one orbital of one spin, between two sectors, behind the C-ABI (include/hxv.h: hxv_apply_ladder, hxv_apply_ladder_axpy): the
// Green's-function start vectors (ED_GF_NORMAL.f90:180-199) built on the device.  One operator, two kernels: ladder_kernel looks every target
// element's source up (spin up, and spin dw on an unsplit sector); on a split sector a dw operator is a signed column permutation across the
// ranks -- one column exchange, then ladder_cols_kernel assembles the local target columns.
#include <algorithm>
#include <string>
#include <vector>

#include "hxv_device.hpp"
#include "hxv_call_scope.hpp"
#include "hxv_ladder_kernels.hpp"

using namespace hxv;

extern "C" {

int hxv_apply_ladder(hxv_handle* from, hxv_handle* to, int32_t orbital, int32_t spin, int32_t create, const void* d_psi, void* d_out,
                     double* norm2) {
  return hxv_apply_ladder_axpy(from, to, orbital, spin, create, 1.0, 0.0, 0, d_psi, d_out, norm2);
}

int hxv_apply_ladder_axpy(hxv_handle* from, hxv_handle* to, int32_t orbital, int32_t spin, int32_t create, double coef_re, double coef_im,
                          int32_t accumulate, const void* d_psi, void* d_out, double* norm2) {
  if (!from || !to || !d_psi || !d_out) return fail(HXV_ERR_ARG, "hxv_apply_ladder: NULL argument");
  const SectorHost &a = from->host, &b = to->host;
  if (a.map_up.empty() || b.map_up.empty()) return fail(HXV_ERR_STATE, "hxv_apply_ladder needs handles built from a model (basis maps)");
  if (from->device != to->device) return fail(HXV_ERR_ARG, "hxv_apply_ladder: handles on different devices");
  if (a.ns != b.ns || orbital < 0 || orbital >= a.ns || spin < 0 || spin > 1) return fail(HXV_ERR_ARG, "hxv_apply_ladder: bad orbital/spin");
  const int d = create ? 1 : -1;
  if (spin == 0 ? (b.nup != a.nup + d || b.ndw != a.ndw) : (b.ndw != a.ndw + d || b.nup != a.nup))
    return fail(HXV_ERR_ARG, "hxv_apply_ladder: `to` is not the sector reached by this operator");
  if (a.nranks != b.nranks || a.rank != b.rank) return fail(HXV_ERR_ARG, "hxv_apply_ladder: the two sectors must be split over the same ranks");
  const bool split = b.nranks != 1 || comm_ready(to);
  if (split && !comm_ready(to)) return fail(HXV_ERR_STATE, "hxv_apply_ladder on split sectors needs the communicator of `to` (hxv_comm_init after opening it)");
  HIPCHK(hipSetDevice(to->device));
  hipStream_t st = to->stream;
  const double2 coef = make_double2(coef_re, coef_im);
  // The reference applies c / c^dagger on the master and scatters the result (ED_GF_NORMAL.f90:174-214).  Here every rank builds its
  // own slab of the new vector:
  //  * spin up: the operator acts inside a column and both sectors have the same DimDw, hence the same split -- purely local;
  //  * spin dw: target column j of sector B is (a sign times) ONE column of sector A, which may belong to another rank of A's split:
  //    a column permutation.  Every rank derives from the two dw maps what it needs from whom and what everybody needs from it
  //    (deterministic, no negotiation), packs, exchanges once, and assembles.
  // a dw operator keeps the row: the two sectors -- same nup, same model -- must store their rows in the same order, split or not
  if (spin == 1 && (a.row_order() != b.row_order() || (a.row_order() && a.up_pos != b.up_pos)))
    return fail(HXV_ERR_STATE, "hxv_apply_ladder: the two sectors store their rows in different orders (HXV_ROW_ORDER changed between the opens?)");
  if (!accumulate) HIPCHK(hipMemsetAsync(d_out, 0, (size_t)b.pitch * std::max(b.qdw, 1) * sizeof(double2), st));  // pad rows = 0
  if (spin == 0 || !split) {
    // spin up with a device row order (SectorHost::up_perm): the source row is looked up in the source sector's SORTED reference map and sent
    // through its permutation; `to`'s map is by device row already; both basis signs ride along.  A dw operator keeps the row (same row
    // order on both sides, checked above): nothing to do.
    const uint32_t* mf = spin == 0 ? (a.row_order() ? from->dev.map_up_ref : from->dev.diag.map_up) : from->dev.diag.map_dw;
    const uint32_t* mt = spin == 0 ? to->dev.diag.map_up : to->dev.diag.map_dw + b.dw0;  // (dw: the local target columns)
    if (spin == 0 && a.qdw != b.qdw) return fail(HXV_ERR_STATE, "hxv_apply_ladder: the DimDw splits of the two sectors differ");
    hipError_t e = launch_ladder(mf, spin == 0 ? a.dimup : a.dimdw, mt, spin == 0 ? b.dimup : b.dimdw, a.pitch, b.dimup, b.pitch, b.qdw,
                                 orbital, spin, create ? 1 : 0, (const double2*)d_psi, (double2*)d_out, st, coef, accumulate ? 1 : 0,
                                 spin == 0 ? from->dev.up_perm : nullptr, spin == 0 ? from->dev.up_sign : nullptr, spin == 0 ? to->dev.up_sign : nullptr);
    if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("ladder kernel: ") + hipGetErrorString(e));
  } else {
    const int P = b.nranks, r = b.rank;
    const uint32_t bit = 1u << orbital;
    // source column (global, in A) and sign of a target column (global, in B); -1: not reached
    auto source_of = [&](int jb, int& sg) -> int {
      const uint32_t mb = b.map_dw[jb];
      if (((mb & bit) != 0u) != (create != 0)) return -1;
      const uint32_t ma = mb ^ bit;
      sg = (__builtin_popcount(ma & (bit - 1u)) & 1) ? -1 : 1;  // (-1)^(occupied orbitals of this spin below `orbital`): c/cdg, ED_SETUP.f90:807-833
      return rank_in(a.map_dw, ma);
    };
    std::vector<int> first_a(P + 1), first_b(P + 1);
    for (int p = 0; p < P; ++p) {
      int q, c0;
      dw_split(a.dimdw, p, P, q, c0);
      first_a[p] = c0;
      dw_split(b.dimdw, p, P, q, c0);
      first_b[p] = c0;
    }
    first_a[P] = a.dimdw;
    first_b[P] = b.dimdw;
    auto owner_a = [&](int ja) { return (int)(std::upper_bound(first_a.begin(), first_a.end(), ja) - first_a.begin()) - 1; };
    // what I receive: my target columns in order, grouped by the source's owner; what I send: every peer's target columns in ITS order
    std::vector<int32_t> slot(std::max(b.qdw, 1), 0), sgn(std::max(b.qdw, 1), 0), send_cols;
    std::vector<int64_t> recv_ptr(P + 1, 0), send_ptr(P + 1, 0);
    std::vector<std::vector<int>> want(P);  // per owner: my local target columns whose source it holds, ascending
    for (int c = 0; c < b.qdw; ++c) {
      int sg = 0;
      const int ja = source_of(b.dw0 + c, sg);
      if (ja < 0) continue;
      sgn[c] = sg;
      const int o = owner_a(ja);
      if (o == r)
        slot[c] = ja - a.dw0;
      else
        want[o].push_back(c);
    }
    int nrecv = 0;
    for (int p = 0; p < P; ++p) {
      recv_ptr[p] = nrecv;
      for (int c : want[p]) slot[c] = -1 - nrecv++;
    }
    recv_ptr[P] = nrecv;
    for (int p = 0; p < P; ++p) {
      send_ptr[p] = (int64_t)send_cols.size();
      if (p == r) continue;
      for (int jb = first_b[p]; jb < first_b[p + 1]; ++jb) {
        int sg = 0;
        const int ja = source_of(jb, sg);
        if (ja >= 0 && owner_a(ja) == r) send_cols.push_back(ja - a.dw0);
      }
    }
    send_ptr[P] = (int64_t)send_cols.size();
    const size_t cb = (size_t)a.pitch * sizeof(double2);
    double2 *d_sendbuf = nullptr, *d_recvbuf = nullptr;
    int32_t* d_lists = nullptr;
    const size_t nl = send_cols.size() + 2 * (size_t)std::max(b.qdw, 1);
    int rc_local = HXV_OK;
    CallScope scratch(to);  // (its release synchronises the stream: the host lists above are read by asynchronous copies and outlive it)
    hipError_t e1 = scratch.take(std::max<size_t>(send_cols.size(), 1) * cb, &d_sendbuf);
    hipError_t e2 = scratch.take(std::max<size_t>((size_t)nrecv, 1) * cb, &d_recvbuf);
    hipError_t e3 = scratch.take_device(std::max<size_t>(nl, 1) * sizeof(int32_t), &d_lists);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) rc_local = fail(HXV_ERR_HIP, "hxv_apply_ladder: staging buffers for the column exchange");
    int rc = comm_agree(to, rc_local);
    if (rc) return rc;
    int32_t* d_send_cols = d_lists;
    int32_t* d_slot = d_lists + send_cols.size();
    int32_t* d_sgn = d_slot + std::max(b.qdw, 1);
    hipError_t e = hipSuccess;
    if (!send_cols.empty()) e = hipMemcpyAsync(d_send_cols, send_cols.data(), send_cols.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_slot, slot.data(), slot.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_sgn, sgn.data(), sgn.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launch_pack_columns((const double2*)d_psi, d_sendbuf, d_send_cols, (int)send_cols.size(), a.pitch, st);
    if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("hxv_apply_ladder: ") + hipGetErrorString(e));
    rc = comm_sendrecv_cols(to, d_sendbuf, send_ptr.data(), d_recvbuf, recv_ptr.data(), cb, st);
    if (rc) return rc;
    if (b.qdw > 0)
      hipLaunchKernelGGL(ladder_cols_kernel, dim3((unsigned)b.qdw), dim3(256), 0, st, b.dimup, b.qdw, a.pitch, b.pitch, d_slot, d_sgn, (const double2*)d_psi,
                         d_recvbuf, (double2*)d_out, coef, accumulate ? 1 : 0);
  }
  if (norm2) {
    // <out|out> over ALL ranks of a split sector (pads of d_out must be zero: hxv.h)
    int rcn = enqueue_norm(to, (const double2*)d_out, (int64_t)b.pitch * b.qdw, LZ_TMP, 0);
    if (rcn) return rcn;
    HIPCHK(hipMemcpyAsync(norm2, to->d_scalars + LZ_TMP, sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return HXV_OK;
}

}  // extern "C"
