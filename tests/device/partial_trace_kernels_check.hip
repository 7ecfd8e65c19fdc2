// TEST-ONLY: one launcher per kernel of the partial-trace engine, so that tests/test_gpu_partial_trace_kernels.py can run each kernel alone
// on the tables of a synthetic sector and compare it with an exact sum or an exact restatement (tests/partial_trace_kernels_ref.py).  The
// kernels and the host scatter are the text of csrc/hxv_partial_trace_kernels.hpp, compiled with the engine's flags
// (build_partial_trace_kernels_check() of __graft_entry__.py); this library is never linked into libhxv.so.
//
// Tables: the ptb_* entries of tests/host/partial_trace_build.hpp (pt_build on flat arrays; every host table handed back), and ptc_upload,
// which copies them to the device.  The three accumulating kernels take a slice [first, first + count) of THEIR part of the work list, as
// pt_accumulate passes it (d_items + the items of the kernels before), on the caller's src, pitch and partial; pt_reduce_kernel runs on the
// uploaded tables or on tables the caller made by hand.  Every launch is on the null stream; the entry waits and returns the HIP status.
// An empty or overlong slice, a null pointer, a pitch below 1 or a handle that is not an uploaded table set is refused
// (hipErrorInvalidValue) before anything is launched.
#include "hxv_partial_trace_kernels.hpp"

#include "../host/partial_trace_build.hpp"

namespace {

constexpr int BAD = (int)hipErrorInvalidValue;

struct Uploaded {
  PtClass* cls = nullptr;
  PtItem* items = nullptr;
  uint32_t *rows = nullptr, *cols = nullptr, *tiles = nullptr;
  int64_t* el_src = nullptr;
  int32_t *el_cnt = nullptr, *el_stride = nullptr;
  ~Uploaded() {
    (void)hipFree(cls);
    (void)hipFree(items);
    (void)hipFree(rows);
    (void)hipFree(cols);
    (void)hipFree(tiles);
    (void)hipFree(el_src);
    (void)hipFree(el_cnt);
    (void)hipFree(el_stride);
  }
};

template <class T>
hipError_t up(const std::vector<T>& v, T** d) {
  hipError_t e = hipMalloc((void**)d, std::max<size_t>(v.size(), 1) * sizeof(T));
  if (e == hipSuccess && !v.empty()) e = hipMemcpy(*d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  return e;
}

int finish() {
  hipError_t e = hipGetLastError();
  hipError_t s = hipStreamSynchronize(nullptr);
  return (int)(e != hipSuccess ? e : s);
}

// the uploaded tables of a handle, or null: not a handle, or tables that were never uploaded
const Uploaded* uploaded(void* h, const PtHostTables** t) {
  ptb::Tables* p = ptb::tables_of(h);
  if (!p || !p->device) return nullptr;
  *t = &p->t;
  return (const Uploaded*)p->device;
}

// which: 0 pair kernel, 1 tile kernel <2,1>, 2 tile kernel <4,2>
int launch(int which, void* h, int first, int count, const void* src, int pitch, void* partial) {
  const PtHostTables* t = nullptr;
  const Uploaded* u = uploaded(h, &t);
  if (!u || !src || !partial || pitch < 1 || first < 0 || count < 1 || (int64_t)first + count > t->nitems[which]) return BAD;
  int before = 0;
  for (int k = 0; k < which; ++k) before += t->nitems[k];
  const PtItem* items = u->items + before + first;
  const dim3 grid((unsigned)count), block(PT_THREADS);
  if (which == 0)
    hipLaunchKernelGGL(pt_pair_kernel, grid, block, 0, nullptr, (const double2*)src, pitch, u->cls, items, u->rows, u->cols, u->tiles, (double2*)partial);
  else if (which == 1)
    hipLaunchKernelGGL((pt_tile_kernel<2, 1>), grid, block, 0, nullptr, (const double2*)src, pitch, u->cls, items, u->rows, u->cols, u->tiles, (double2*)partial);
  else
    hipLaunchKernelGGL((pt_tile_kernel<4, 2>), grid, block, 0, nullptr, (const double2*)src, pitch, u->cls, items, u->rows, u->cols, u->tiles, (double2*)partial);
  return finish();
}

}  // namespace

extern "C" {

// out[0..5] = PT_THREADS, PT_XS, PT_PAIR_N, PT_LOADS, PT_PAIR_COST, PT_WG_PER_CU
void ptc_constants(int* out) {
  out[0] = PT_THREADS;
  out[1] = PT_XS;
  out[2] = PT_PAIR_N;
  out[3] = PT_LOADS;
  out[4] = PT_PAIR_COST;
  out[5] = PT_WG_PER_CU;
}

// copies the tables of a ptb_build handle to the current device (once); ptb_free releases them
int ptc_upload(void* h) {
  ptb::Tables* p = ptb::tables_of(h);
  if (!p || p->device) return BAD;
  auto* u = new Uploaded();
  const PtHostTables& t = p->t;
  hipError_t e = up(t.cls, &u->cls);
  if (e == hipSuccess) e = up(t.items, &u->items);
  if (e == hipSuccess) e = up(t.rows, &u->rows);
  if (e == hipSuccess) e = up(t.cols, &u->cols);
  if (e == hipSuccess) e = up(t.tiles, &u->tiles);
  if (e == hipSuccess) e = up(t.el_src, &u->el_src);
  if (e == hipSuccess) e = up(t.el_cnt, &u->el_cnt);
  if (e == hipSuccess) e = up(t.el_stride, &u->el_stride);
  if (e != hipSuccess) {
    delete u;
    return (int)e;
  }
  p->device = u;
  p->release = [](void* d) { delete (Uploaded*)d; };
  return 0;
}

int ptc_pair(void* h, int first, int count, const void* src, int pitch, void* partial) { return launch(0, h, first, count, src, pitch, partial); }
int ptc_tile_2_1(void* h, int first, int count, const void* src, int pitch, void* partial) { return launch(1, h, first, count, src, pitch, partial); }
int ptc_tile_4_2(void* h, int first, int count, const void* src, int pitch, void* partial) { return launch(2, h, first, count, src, pitch, partial); }

// pt_reduce_kernel on the uploaded tables, with pt_accumulate's grid
int ptc_reduce(void* h, const void* partial, void* out) {
  const PtHostTables* t = nullptr;
  const Uploaded* u = uploaded(h, &t);
  if (!u || !partial || !out || t->out_elems < 1) return BAD;
  hipLaunchKernelGGL(pt_reduce_kernel, dim3((unsigned)((t->out_elems + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0, nullptr,
                     (const double2*)partial, u->el_src, u->el_cnt, u->el_stride, t->out_elems, (double2*)out);
  return finish();
}

// pt_reduce_kernel on the caller's tables (device pointers, nel entries each), with pt_accumulate's grid
int ptc_reduce_tables(const void* partial, const int64_t* el_src, const int32_t* el_cnt, const int32_t* el_stride, int64_t nel, void* out) {
  if (!partial || !el_src || !el_cnt || !el_stride || !out || nel < 1 || nel > (int64_t)1 << 30) return BAD;
  hipLaunchKernelGGL(pt_reduce_kernel, dim3((unsigned)((nel + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0, nullptr,
                     (const double2*)partial, el_src, el_cnt, el_stride, nel, (double2*)out);
  return finish();
}

// HOST: scatter of out_elems class-block elements (re, im pairs) into rho, 2 * 16^nsub doubles
int ptc_scatter(void* h, const double* raw, double weight, int accumulate, double* rho) {
  ptb::Tables* p = ptb::tables_of(h);
  if (!p || !raw || !rho) return BAD;
  std::vector<double2> v((size_t)p->t.out_elems);
  for (size_t i = 0; i < v.size(); ++i) v[i] = make_double2(raw[2 * i], raw[2 * i + 1]);
  scatter(p->t, v, weight, accumulate != 0, rho);
  return 0;
}

}  // extern "C"
