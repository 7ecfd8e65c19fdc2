// The partial-trace engine: rho = Tr_env |psi><psi| of a device-resident state from the tables of hxv_partial_trace_host.hpp, under
// hxv_cluster_dm_accumulate (hxv_cluster_dm.cpp) and hxv_reduced_dm_accumulate (hxv_reduced_dm.cpp).  The only file of the three with device code.
//   pt_pair_kernel     classes with n = dU*dD <= 4 (every class of a one- or two-orbital subset): one thread per pair, its at most four
//                      amplitudes loaded straight from the vector (16 bytes each) and the upper triangle of x x^+ kept in registers;
//                      consecutive threads take consecutive up groups of one dw group.  The workgroup sums its threads in a fixed order (xor
//                      butterfly inside a wave, then wave 0..3) and writes one partial block.
//   pt_tile_kernel<T,NT>  the other classes: one workgroup per item of the work list.  It stages the amplitudes of a batch of pairs through
//                      LDS (16-byte loads; a batch takes consecutive up groups of the class) and keeps the upper triangle of the class block
//                      in registers, NT tiles of T x T elements per thread; it writes one partial block (four, one per wave, where the
//                      block's tiles fit one wave and the waves share out a batch's pairs).  <2,1> and <4,2>.
//   pt_reduce_kernel   one thread per class-block element: the partials of its class, summed in list order.
// No floating-point atomics: the same vector on the same handle gives the same bits on every call.  On a split sector a dw group belongs to
// the rank that owns its first column and reads the gathered copy; the class blocks are all-reduced.  The host scatters the class blocks into
// the dense matrix and fills the lower triangle by conjugation.  The kernels and that scatter are in hxv_partial_trace_kernels.hpp, which a test-only
// library includes as well (tests/device/partial_trace_kernels_check.hip); the tables' owner and the two entry points are here.
#include <hip/hip_runtime.h>

#include "hxv_call_scope.hpp"
#include "hxv_partial_trace_host.hpp"
#include "hxv_partial_trace_kernels.hpp"

namespace hxv {
struct PtTables : PtHostTables, DeviceTables {
  std::string name;  // "cluster density matrix": the head of the error text
  PtClass* d_cls = nullptr;
  PtItem* d_items = nullptr;
  uint32_t *d_rows = nullptr, *d_cols = nullptr, *d_tiles = nullptr;
  int32_t *d_el_cnt = nullptr, *d_el_stride = nullptr;
  int64_t* d_el_src = nullptr;
};

int pt_make_tables(const hxv_handle* h, int nsub, const PtGroups& up, const PtGroups& dw, int small_n, const char* name, std::shared_ptr<PtTables>& out) {
  const SectorHost& s = h->host;
  auto t = std::make_shared<PtTables>();
  const std::string err = pt_build(PtSector{nsub, s.nup, s.ndw, s.dimup, s.dimdw, s.nranks, s.cmax, s.qdw, s.dw0}, up, dw, small_n, compute_units(h->device), name, *t);
  if (!err.empty()) return fail(HXV_ERR_STATE, err);
  t->name = name;
  t->device = h->device;
  TableArena ar;
  (void)ar.add(t->cls, &t->d_cls);
  (void)ar.add(t->items, &t->d_items);
  (void)ar.add(t->rows, &t->d_rows);
  (void)ar.add(t->cols, &t->d_cols);
  (void)ar.add(t->tiles, &t->d_tiles);
  (void)ar.add(t->el_src, &t->d_el_src);
  (void)ar.add(t->el_cnt, &t->d_el_cnt);
  (void)ar.add(t->el_stride, &t->d_el_stride);
  const hipError_t e = ar.commit(&t->base, &t->bytes);
  if (e != hipSuccess) return fail(HXV_ERR_HIP, t->name + " tables: " + hipGetErrorString(e));
  out = t;
  return HXV_OK;
}

int pt_stored_tables(hxv_handle* h, const char* family, const std::string& key, size_t cap, std::shared_ptr<PtTables>& out,
                     const std::function<int(std::shared_ptr<PtTables>&)>& build) {
  return h->img->tables.get(family, key, cap, out, build);
}

int pt_accumulate(hxv_handle* h, const std::shared_ptr<PtTables>& t, int rc_local, const void* d_psi, double weight, bool accumulate, double* out,
                  const char* what) {
  const SectorHost& s = h->host;
  const bool split = s.nranks > 1;
  hipStream_t st = h->stream;
  // rank-local preparation: scratch; every rank learns whether all could go on
  double2 *d_part = nullptr, *d_out = nullptr, *d_full = nullptr;
  CallScope scratch(h);
  if (rc_local == HXV_OK) {
    hipError_t e1 = scratch.take(std::max<size_t>((size_t)t->partial_elems, 1) * sizeof(double2), &d_part);
    hipError_t e2 = scratch.take(std::max<size_t>((size_t)t->out_elems, 1) * sizeof(double2), &d_out);
    hipError_t e3 = split ? scratch.take(std::max<size_t>((size_t)s.nranks * s.cmax * s.pitch, 1) * sizeof(double2), &d_full) : hipSuccess;
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) rc_local = fail(HXV_ERR_HIP, std::string(what) + ": scratch buffers");
  }
  int rc = split ? comm_agree(h, rc_local) : rc_local;
  if (rc) return rc;
  const double2* psi = (const double2*)d_psi;
  if (split) {
    rc = comm_allgather_slab(h, psi, d_full, st);
    if (rc) return rc;
  }
  const double2* src = split ? (const double2*)d_full : psi;
  const int* ni = t->nitems;
  if (ni[0] > 0)
    hipLaunchKernelGGL(pt_pair_kernel, dim3((unsigned)ni[0]), dim3(PT_THREADS), 0, st, src, s.pitch, t->d_cls, t->d_items, t->d_rows, t->d_cols,
                       t->d_tiles, d_part);
  if (ni[1] > 0)
    hipLaunchKernelGGL((pt_tile_kernel<2, 1>), dim3((unsigned)ni[1]), dim3(PT_THREADS), 0, st, src, s.pitch, t->d_cls, t->d_items + ni[0], t->d_rows,
                       t->d_cols, t->d_tiles, d_part);
  if (ni[2] > 0)
    hipLaunchKernelGGL((pt_tile_kernel<4, 2>), dim3((unsigned)ni[2]), dim3(PT_THREADS), 0, st, src, s.pitch, t->d_cls, t->d_items + ni[0] + ni[1],
                       t->d_rows, t->d_cols, t->d_tiles, d_part);
  hipLaunchKernelGGL(pt_reduce_kernel, dim3((unsigned)((t->out_elems + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0, st,
                     (const double2*)d_part, t->d_el_src, t->d_el_cnt, t->d_el_stride, t->out_elems, d_out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(HXV_ERR_HIP, t->name + " kernels: " + hipGetErrorString(e));
  if (split) {
    rc = comm_allreduce_sum(h, (double*)d_out, (size_t)(2 * t->out_elems), st);
    if (rc) return rc;
  }
  std::vector<double2> raw((size_t)t->out_elems);
  e = hipMemcpyAsync(raw.data(), d_out, (size_t)t->out_elems * sizeof(double2), hipMemcpyDeviceToHost, st);
  scratch.release();  // (synchronises the stream: raw is read below)
  if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  scatter(*t, raw, weight, accumulate, out);
  return HXV_OK;
}
}  // namespace hxv
