// The slab exchange behind the C-ABI: what the product does with the collectives of hxv_transport.cpp, which knows no layout.  The reference splits the vector along DimDw (ED_HAMILTONIAN.f90:93-105) and re-assembles what a rank needs with
// MPI collectives inside spMatVec_MPI_main (ED_HAMILTONIAN_SPARSE_HxV.f90:272-296, ED_HAMILTONIAN_COMMON.f90:30-94).
// Here the re-assembly is ONE equal-count all-gather of the padded slabs (or the halo exchange: only the columns H_dw
// couples across ranks; or the reference's two transposes), on the stream the product runs on, so a Fortran rank needs nothing but this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>

#include "hxv_handle.hpp"
#include "hxv_tile_dev.hpp"

using namespace hxv;

namespace {

// bytes of one column of a Lanczos / product vector: complex(8) columns of `pitch` elements or real ones of pitch_real
size_t col_bytes(const hxv_handle* h, bool real) { return real ? (size_t)pitch_real_of(h) * sizeof(double) : (size_t)h->host.pitch * sizeof(double2); }

int ensure_gather(hxv_handle* h, hipStream_t st) {
  const SectorHost& s = h->host;
  if (h->d_gather) return HXV_OK;
  // sized for complex vectors; real ones (half the bytes per column) use the front of the same buffer
  const size_t cb = col_bytes(h, false);
  if (s.exchange == 1) {
    const size_t nfull = (size_t)s.qdw + s.halo_cols.size();
    HIPCHK(pool_alloc(h->device, std::max<size_t>(nfull, 1) * cb, (void**)&h->d_gather));
    HIPCHK(pool_alloc(h->device, std::max<size_t>(s.send_cols.size(), 1) * cb, (void**)&h->d_send));
    HIPCHK(hipMalloc((void**)&h->d_send_cols, std::max<size_t>(s.send_cols.size(), 1) * sizeof(int32_t)));
    HIPCHK(hipMemcpy(h->d_send_cols, s.send_cols.data(), s.send_cols.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    h->device_bytes += (int64_t)((nfull + s.send_cols.size()) * cb);
  } else {
    const size_t bytes = (size_t)s.cmax * s.nranks * cb;
    HIPCHK(pool_alloc(h->device, std::max<size_t>(bytes, 1), (void**)&h->d_gather));
    HIPCHK(hipMemsetAsync(h->d_gather, 0, bytes, st));
    h->device_bytes += (int64_t)bytes;
  }
  return HXV_OK;
}

// Exchange: this rank's slab d_v_local -> the gathered vector h->d_gather in the layout the kernels expect
// (all-gather layout or halo layout, hxv.h); asynchronous on st.
int exchange(hxv_handle* h, const void* d_v_local, bool real, hipStream_t st) {
  const SectorHost& s = h->host;
  HIPCHK(hipSetDevice(h->device));
  int rc = ensure_gather(h, st);
  if (rc) return rc;
  const size_t cb = col_bytes(h, real);
  // A vector that already sits at the slab's place of one of the handle's gather buffers (hxv_slab_home; the Lanczos vectors of a split
  // sector) is exchanged where it is; anything else is copied into the first buffer.
  const size_t home_off = s.exchange == 1 ? 0 : (size_t)s.rank * s.cmax * cb;
  char* gather = reinterpret_cast<char*>(h->d_gather);
  bool at_home = false;
  for (double2* cand : {h->d_gather, h->d_gather_x[0], h->d_gather_x[1]})
    if (cand && reinterpret_cast<const char*>(cand) + home_off == reinterpret_cast<const char*>(d_v_local)) {
      gather = reinterpret_cast<char*>(cand);
      at_home = true;
    }
  h->gather_cur = reinterpret_cast<double2*>(gather);
  if (!at_home) h->n_slab_copy++;
  if (s.exchange == 1) {
    // HALO exchange: only the columns H_dw couples to another rank's rows travel -- packed per destination; they land
    // behind the local slab, where the column -> slot table of this layout expects them
    // (a caller that keeps its slab where the exchange wants it -- hxv_slab_home -- saves this copy)
    if (!at_home) HIPCHK(hipMemcpyAsync(gather, d_v_local, (size_t)s.qdw * cb, hipMemcpyDeviceToDevice, st));
    hipError_t pe = launch_pack_columns((const double2*)d_v_local, h->d_send, h->d_send_cols, (int)s.send_cols.size(), (int)(cb / sizeof(double2)), st);
    if (pe != hipSuccess) return fail(HXV_ERR_HIP, std::string("pack kernel: ") + hipGetErrorString(pe));
    const std::vector<int64_t> sp(s.send_ptr.begin(), s.send_ptr.end()), hp(s.halo_ptr.begin(), s.halo_ptr.end());
    rc = comm_sendrecv_cols(h, h->d_send, sp.data(), gather + (size_t)s.qdw * cb, hp.data(), cb, st);
    if (rc) return rc;
    h->n_exchange++;
    return HXV_OK;
  }
  // ALL-GATHER: copy the slab into its slot of the gather buffer, all-gather in place (equal counts: ranks that own one
  // column less leave their last column unused)
  const size_t slot = (size_t)s.cmax * cb;
  char* mine = gather + (size_t)s.rank * slot;
  if (!at_home) HIPCHK(hipMemcpyAsync(mine, d_v_local, (size_t)s.qdw * cb, hipMemcpyDeviceToDevice, st));
  rc = comm_allgather_inplace(h, gather, slot, st);
  if (rc) return rc;
  h->n_exchange++;
  return HXV_OK;
}
}  // namespace

namespace hxv {

// Does p point into one of the handle's gather buffers (hxv_slab_home hands out a slot of the first)?  The device Lanczos drivers zero
// the slab's place in all three before they read their start vector: a start vector that lives there is staged first.
bool comm_in_gather(const hxv_handle* h, const void* p) {
  const SectorHost& s = h->host;
  const size_t cbc = col_bytes(h, false);
  const size_t bytes = s.exchange == 1 ? std::max<size_t>((size_t)s.qdw + s.halo_cols.size(), 1) * cbc : std::max<size_t>((size_t)s.cmax * s.nranks * cbc, 1);
  for (const double2* b : {h->d_gather, h->d_gather_x[0], h->d_gather_x[1]})
    if (b && reinterpret_cast<const char*>(p) >= reinterpret_cast<const char*>(b) && reinterpret_cast<const char*>(p) < reinterpret_cast<const char*>(b) + bytes) return true;
  return false;
}

// Three places for the slab of a split sector's Lanczos vectors: its slot in the handle's gather buffer and in two more of the same
// size, so that every vector of the three-term recurrence is exchanged where it lies (no slab copy per product).  The slab regions
// are zeroed (pad rows must be zero; `real`: layout of the coming run).  HXV_OK with out[] set, or an error (the caller falls back to
// slab buffers of its own on HXV_ERR_HIP from the allocation).
int comm_lz_homes(hxv_handle* h, bool real, double2* out[3]) {
  const SectorHost& s = h->host;
  HIPCHK(hipSetDevice(h->device));
  int rc = ensure_gather(h, h->stream);
  if (rc) return rc;
  const size_t cbc = col_bytes(h, false);
  const size_t bytes = s.exchange == 1 ? std::max<size_t>((size_t)s.qdw + s.halo_cols.size(), 1) * cbc : std::max<size_t>((size_t)s.cmax * s.nranks * cbc, 1);
  {
    // Three whole gather buffers are the right trade only where they fit comfortably (in all-gather layout each is a whole-Dim vector,
    // and the sectors that get split are the large ones): with less than the missing buffers + 1/16 of the device free (the engine's
    // cache counted as free) the caller's fall-back runs -- three SLAB buffers, one slab copy per product.
    size_t need = 0;
    for (const double2* p : h->d_gather_x)
      if (!p) need += bytes;
    if (need) {
      size_t fr = 0, tot = 0;
      int64_t cached = 0;
      HIPCHK(hipMemGetInfo(&fr, &tot));
      (void)hxv_pool_stats(h->device, &cached, nullptr, nullptr);
      if (fr + (size_t)cached < need + tot / 16) return fail(HXV_ERR_HIP, "gather buffers of the device Lanczos: not enough free device memory for the in-place layout");
    }
  }
  for (auto& p : h->d_gather_x)
    if (!p) {
      hipError_t e = pool_alloc(h->device, bytes, (void**)&p);
      if (e != hipSuccess) {
        // not enough memory for three whole gather buffers (the sectors that get split are the large ones): give back what this call
        // obtained, so that the caller's fall-back -- three SLAB buffers and one slab copy per product -- starts from a clean slate
        p = nullptr;
        (void)hipGetLastError();
        for (auto& q : h->d_gather_x)
          if (q) {
            pool_free(h->device, q);
            q = nullptr;
            h->device_bytes -= (int64_t)bytes;
          }
        return fail(HXV_ERR_HIP, std::string("gather buffers of the device Lanczos: ") + hipGetErrorString(e));
      }
      h->device_bytes += (int64_t)bytes;
    }
  const size_t cb = col_bytes(h, real);
  const size_t home_off = s.exchange == 1 ? 0 : (size_t)s.rank * s.cmax * cb;
  double2* base[3] = {h->d_gather, h->d_gather_x[0], h->d_gather_x[1]};
  for (int i = 0; i < 3; ++i) {
    out[i] = reinterpret_cast<double2*>(reinterpret_cast<char*>(base[i]) + home_off);
    HIPCHK(hipMemsetAsync(out[i], 0, (size_t)std::max(s.qdw, 1) * col_bytes(h, false), h->stream));  // (the complex slab's extent covers the real one's)
  }
  return HXV_OK;
}

// The whole vector on every rank, in the padded all-gather layout, into a buffer of the caller's (nranks * cmax columns of pitch elements):
// what the impurity observables read when a pair of dw configurations spans two ranks.  Independent of the exchange the products use
// (the halo layout holds only the columns H_dw couples).  Unused slots of ranks that own one column less hold whatever was there.
int comm_allgather_slab(hxv_handle* h, const double2* d_v_local, double2* d_full, hipStream_t st) {
  const SectorHost& s = h->host;
  HIPCHK(hipSetDevice(h->device));
  const size_t cb = col_bytes(h, false), slot = (size_t)s.cmax * cb;
  char* full = reinterpret_cast<char*>(d_full);
  char* mine = full + (size_t)s.rank * slot;
  if (s.qdw > 0) HIPCHK(hipMemcpyAsync(mine, d_v_local, (size_t)s.qdw * cb, hipMemcpyDeviceToDevice, st));
  return comm_allgather_inplace(h, d_full, slot, st);
}

// d_hv_local = (H v)|slab with v given as this rank's slab: exchange, then the product on the gathered vector.
// `ep`: optional Lanczos epilogue of pass A (fused recurrence on a split sector: the partial sums are this rank's share).
// ---------------------------------------------------------------------------------------------------------------------------------
// Exchange 2: the reference's own scheme (spMatVec_mpi_main, ED_HAMILTONIAN_SPARSE_HxV.f90:272-296; vector_transpose_MPI,
// ED_HAMILTONIAN_COMMON.f90:30-94) -- transpose the slab to row panels, dw hops on the panel, transpose back, then diagonal + up hops +
// the assembled dw part on the slab.  Each transpose moves (P-1)/P of ONE slab per rank instead of (P-1) slabs: the lowest-traffic
// exchange (C3 at 8 ranks: 0.58 GB into a GPU per product against 2.32 GB for the all-gather).  Rows are split like the columns
// (mpiQup rule, :274-275).  Blocks are packed / unpacked with strided device copies; the block a rank keeps never leaves its GPU.
// hxv_time_apply_slab: events around the kernels of a slab product
static inline void kt_mark(hxv_handle* h, int i, hipStream_t st) {
  if (h->kt_on && h->kt_ev[i]) (void)hipEventRecord(h->kt_ev[i], st);
}

struct A2A {
  hxv_handle* panel = nullptr;
  std::vector<int> rn, ru0, cq, cc0;         // per rank: its rows (count, first) and columns (count, first)
  std::vector<int64_t> sp1, rp1, sp2, rp2;   // [P+1] element offsets of the per-peer blocks in the send / receive buffers, both transposes
  std::vector<int64_t> pan;                  // [P+1] element offsets of the ranks' column ranges in an UNPADDED panel (direct receive / send)
  double2 *d_send = nullptr, *d_recv = nullptr, *d_x = nullptr, *d_y = nullptr;
  WtRange* d_wtr[2] = {nullptr, nullptr};    // [P] where pass A finds the dw part after the second transpose, per rank of origin (complex / real layout)
  int pp = 0;                                // panel pitch (complex layout)
  int mode = 0;                              // layout the panel / dw-part buffers were last used in (0 complex, 1 real): the pad rows differ
};

static void a2a_release(hxv_handle* h) {
  A2A* a = static_cast<A2A*>(h->a2a);
  if (!a) return;
  for (double2* p : {a->d_send, a->d_recv, a->d_x, a->d_y})
    if (p) pool_free(h->device, p);
  for (WtRange* p : a->d_wtr)
    if (p) (void)hipFree(p);
  if (a->panel) (void)hxv_destroy(a->panel);
  delete a;
  h->a2a = nullptr;
}

static int ensure_a2a(hxv_handle* h, hipStream_t st) {
  if (h->a2a) return HXV_OK;
  const SectorHost& s = h->host;
  const int P = s.nranks;
  std::unique_ptr<A2A> a(new A2A());
  a->rn.resize(P);
  a->ru0.resize(P);
  a->cq.resize(P);
  a->cc0.resize(P);
  // Rows are dealt in units of 16 where every rank still gets some: a rank whose row count is a multiple of the panel's pitch granularity
  // (8 complex / 16 real elements) has an UNPADDED panel, receives its blocks of the first transpose straight into it and sends the
  // blocks of the second straight out of it -- two of the four strided copies per product go away.
  const int units = (s.dimup + 15) / 16;
  for (int p = 0; p < P; ++p) {
    if (units >= P) {
      int nu, u0;
      dw_split(units, p, P, nu, u0);
      a->ru0[p] = std::min(16 * u0, s.dimup);
      a->rn[p] = std::min(16 * (u0 + nu), s.dimup) - a->ru0[p];
    } else {
      dw_split(s.dimup, p, P, a->rn[p], a->ru0[p]);
    }
    dw_split(s.dimdw, p, P, a->cq[p], a->cc0[p]);
  }
  const int nme = a->rn[s.rank], qme = s.qdw;
  if (nme < 1) return fail(HXV_ERR_UNSUPPORTED, "all-to-all exchange: a rank without rows (nranks > DimUp)");
  a->sp1.assign(P + 1, 0);
  a->rp1.assign(P + 1, 0);
  a->sp2.assign(P + 1, 0);
  a->rp2.assign(P + 1, 0);
  for (int p = 0; p < P; ++p) {
    const bool self = p == s.rank;
    a->sp1[p + 1] = a->sp1[p] + (self ? 0 : (int64_t)qme * a->rn[p]);   // my columns, p's rows
    a->rp1[p + 1] = a->rp1[p] + (self ? 0 : (int64_t)a->cq[p] * nme);   // p's columns, my rows
    a->sp2[p + 1] = a->sp2[p] + (self ? 0 : (int64_t)a->cq[p] * nme);   // (the way back: the same blocks, roles swapped)
    a->rp2[p + 1] = a->rp2[p] + (self ? 0 : (int64_t)qme * a->rn[p]);
  }
  a->pan.assign(P + 1, 0);
  for (int p = 0; p < P; ++p) a->pan[p + 1] = a->pan[p] + (int64_t)a->cq[p] * nme;
  HIPCHK(hipSetDevice(h->device));
  hxv_handle* ph = new hxv_handle();
  std::string e = make_panel_host(s, nme, ph->host);
  if (!e.empty()) {
    delete ph;
    return fail(HXV_ERR_STATE, "all-to-all exchange: " + e);
  }
  hxv_handle* out = nullptr;
  int rc = finish_create(ph, h->device, &out);  // (deletes ph on failure)
  if (rc) return rc;
  a->panel = out;
  a->pp = out->host.pitch;
  const size_t nsend = (size_t)std::max<int64_t>(std::max(a->sp1[P], a->sp2[P]), 1), nrecv = (size_t)std::max<int64_t>(std::max(a->rp1[P], a->rp2[P]), 1);
  const size_t npanel = (size_t)s.dimdw * a->pp;
  struct { double2** p; size_t n; } bufs[4] = {{&a->d_send, nsend}, {&a->d_recv, nrecv}, {&a->d_x, npanel}, {&a->d_y, npanel}};
  for (auto& b : bufs) {
    hipError_t ea = pool_alloc(h->device, b.n * sizeof(double2), (void**)b.p);
    if (ea != hipSuccess) {
      h->a2a = a.release();
      a2a_release(h);
      return fail(HXV_ERR_HIP, std::string("all-to-all exchange buffers: ") + hipGetErrorString(ea));
    }
    h->device_bytes += (int64_t)(b.n * sizeof(double2));
  }
  // pad rows of the panel are never written by the unpack copies: zero them once
  HIPCHK(hipMemsetAsync(a->d_x, 0, npanel * sizeof(double2), st));
  // Where the dw part of this rank's slab lies after the second transpose, per rank of origin: the blocks the peers sent stay in the
  // receive buffer ([q columns][rn[p] rows] each), the block this rank kept stays in its panel output (column range cc0[me].., pitch =
  // panel pitch).  Pass A reads them there (WtRange): no unpack copies, no assembled copy of the dw part.
  for (int real = 0; real < 2; ++real) {
    const size_t esz = real ? sizeof(double) : sizeof(double2);
    const int64_t ppr = real ? (int64_t)pitch_real_of(out) : (int64_t)a->pp;
    std::vector<WtRange> tab(P);
    for (int p = 0; p < P; ++p) {
      tab[p].row0 = a->ru0[p];
      tab[p].row1 = a->ru0[p] + a->rn[p];
      if (p == s.rank) {
        tab[p].stride = ppr;
        tab[p].base = reinterpret_cast<const char*>(a->d_y) + (size_t)a->cc0[p] * ppr * esz;
      } else {
        tab[p].stride = a->rn[p];
        tab[p].base = reinterpret_cast<const char*>(a->d_recv) + (size_t)a->rp2[p] * esz;
      }
    }
    hipError_t ea = hipMalloc((void**)&a->d_wtr[real], P * sizeof(WtRange));
    if (ea == hipSuccess) ea = hipMemcpy(a->d_wtr[real], tab.data(), P * sizeof(WtRange), hipMemcpyHostToDevice);
    if (ea != hipSuccess) {
      h->a2a = a.release();
      a2a_release(h);
      return fail(HXV_ERR_HIP, std::string("all-to-all exchange tables: ") + hipGetErrorString(ea));
    }
  }
  h->a2a = a.release();
  return HXV_OK;
}

// (rows [u0,u0+n) of `ncols` columns of pitch `pitch`) <-> contiguous [ncols][n]; esz = bytes per element (16 complex, 8 real)
static hipError_t copy_block(void* dst, size_t dpitch, const void* src, size_t spitch, int n, int ncols, size_t esz, hipStream_t st) {
  if (n <= 0 || ncols <= 0) return hipSuccess;
  return hipMemcpy2DAsync(dst, dpitch * esz, src, spitch * esz, (size_t)n * esz, (size_t)ncols, hipMemcpyDeviceToDevice, st);
}

// `real`: the slabs are double[qdw][pitch_real] (REAL-vector mode of the drivers: half the bytes in every step below)
static int apply_slab_a2a(hxv_handle* h, const void* v_, void* hv_, bool real, hipStream_t st, const LzEpilogue* ep) {
  const SectorHost& s = h->host;
  if (!comm_ready(h)) return fail(HXV_ERR_STATE, "split sector without a communicator: call hxv_comm_init after opening the sector");
  HIPCHK(hipSetDevice(h->device));
  int rc = ensure_a2a(h, st);
  if (rc) return rc;
  A2A& a = *static_cast<A2A*>(h->a2a);
  const int P = s.nranks, me = s.rank, nme = a.rn[me], q = s.qdw;
  const size_t esz = real ? sizeof(double) : sizeof(double2);
  const size_t pit = real ? (size_t)pitch_real_of(h) : (size_t)s.pitch;          // slab pitch
  const size_t pp = real ? (size_t)pitch_real_of(a.panel) : (size_t)a.pp;         // panel pitch
  if (a.mode != (real ? 1 : 0)) {
    // the pad rows of the two layouts sit at different places and the unpack copies never write pads
    HIPCHK(hipMemsetAsync(a.d_x, 0, (size_t)s.dimdw * a.pp * sizeof(double2), st));
    a.mode = real ? 1 : 0;
  }
  const char* v = static_cast<const char*>(v_);
  char *send = reinterpret_cast<char*>(a.d_send), *recv = reinterpret_cast<char*>(a.d_recv), *x = reinterpret_cast<char*>(a.d_x),
       *y = reinterpret_cast<char*>(a.d_y);
  // OVERLAPPED form (option "exchange_overlap", plain products): the reference computes the diagonal and the up hops before its first
  // transpose (ED_HAMILTONIAN_SPARSE_HxV.f90:250-270, then :272-296); here they run on a second stream WHILE pack, transpose, panel
  // product and transpose back are under way, and the dw part is added at the end (hv += pieces: 32 B per local state more than the
  // fused form, which reads the pieces as pass A's accumulator init).  Pays where a transpose takes longer than pass A on the slab.
  const bool overlap = h->a2a_overlap && !ep && h->plan.usable;
  //  every error return below the launch on the second stream waits for it first: the caller may free or reuse v / hv at once
  struct JoinSecondStream {
    hipStream_t s2 = nullptr;
    ~JoinSecondStream() {
      if (s2) (void)hipStreamSynchronize(s2);
    }
  } join2;
  if (overlap) {
    if (!h->stream2) HIPCHK(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
    for (auto& e : h->ov_ev)
      if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIPCHK(hipEventRecord(h->ov_ev[0], st));                 // v is ready (and the previous user of hv is done) on st
    HIPCHK(hipStreamWaitEvent(h->stream2, h->ov_ev[0], 0));
    kt_mark(h, 4, h->stream2);
    hipError_t eo;
    if (real) {
      DevSector d = h->dev;
      d.pitch = (int)pit;
      eo = launch_hxv_tiled_real(d, h->plan, reinterpret_cast<const double*>(v) - (int64_t)d.slab0 * d.pitch, nullptr, static_cast<double*>(hv_), h->stream2, nullptr, 1, true);
    } else {
      eo = launch_hxv_tiled(h->dev, h->plan, reinterpret_cast<const double2*>(v) - (int64_t)h->dev.slab0 * h->dev.pitch, nullptr, static_cast<double2*>(hv_), h->stream2,
                            nullptr, 1, true);
    }
    if (eo != hipSuccess) return fail(HXV_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(eo));
    kt_mark(h, 5, h->stream2);
    join2.s2 = h->stream2;  // from here on pass A is writing hv on the second stream: no return may leave it unjoined
    HIPCHK(hipEventRecord(h->ov_ev[1], h->stream2));
  }
  // 1. my slab cut by the receivers' row ranges; my own block goes straight into the panel
  for (int p = 0; p < P; ++p) {
    if (p == me)
      HIPCHK(copy_block(x + (size_t)a.cc0[me] * pp * esz, pp, v + (size_t)a.ru0[me] * esz, pit, nme, q, esz, st));
    else
      HIPCHK(copy_block(send + (size_t)a.sp1[p] * esz, a.rn[p], v + (size_t)a.ru0[p] * esz, pit, a.rn[p], q, esz, st));
  }
  const bool direct = pp == (size_t)nme;  // unpadded panel: a peer's block IS its column range of the panel
  rc = direct ? comm_sendrecv_cols(h, send, a.sp1.data(), x, a.pan.data(), esz, st) : comm_sendrecv_cols(h, send, a.sp1.data(), recv, a.rp1.data(), esz, st);
  if (rc) return rc;
  if (!direct)
    for (int p = 0; p < P; ++p)
      if (p != me) HIPCHK(copy_block(x + (size_t)a.cc0[p] * pp * esz, pp, recv + (size_t)a.rp1[p] * esz, nme, nme, a.cq[p], esz, st));
  // 2. dw hops on the row panel [my rows] x [all columns]
  kt_mark(h, 0, st);
  if (real) {
    if (!a.panel->plan.usable) return fail(HXV_ERR_UNSUPPORTED, "all-to-all exchange: tiled kernels unavailable on the panel");
    DevSector d = a.panel->dev;
    d.pitch = (int)pp;
    hipError_t e = launch_hxv_tiled_real(d, a.panel->plan, reinterpret_cast<const double*>(x), reinterpret_cast<double*>(y), nullptr, st, nullptr, 2, true);
    if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  } else {
    rc = hxv_apply_dw_panel(a.panel, a.d_x, a.d_y, st);
    if (rc) return rc;
  }
  kt_mark(h, 1, st);
  // 3. back to the column owners: peers' blocks go out of the panel output (direct) or through the send buffer; what arrives STAYS in the
  //    receive buffer and the block this rank keeps stays in the panel output -- pass A reads the pieces where they are (a.d_wtr)
  if (!direct)
    for (int p = 0; p < P; ++p)
      if (p != me) HIPCHK(copy_block(send + (size_t)a.sp2[p] * esz, nme, y + (size_t)a.cc0[p] * pp * esz, pp, nme, a.cq[p], esz, st));
  rc = direct ? comm_sendrecv_cols(h, y, a.pan.data(), recv, a.rp2.data(), esz, st) : comm_sendrecv_cols(h, send, a.sp2.data(), recv, a.rp2.data(), esz, st);
  if (rc) return rc;
  if (overlap) {
    // 4'. the dw part joins what the second stream has computed meanwhile
    HIPCHK(hipStreamWaitEvent(st, h->ov_ev[1], 0));
    join2.s2 = nullptr;  // joined in stream order: st now waits for pass A
    kt_mark(h, 2, st);
    hipError_t ea = launch_add_pieces(hv_, a.d_wtr[real ? 1 : 0], P, s.dimup, (int)pit, q, real, st);
    if (ea != hipSuccess) return fail(HXV_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(ea));
    kt_mark(h, 3, st);
    h->n_apply++;
    h->n_exchange += 2;
    return HXV_OK;
  }
  // 4. diagonal + up hops + the assembled dw part on the slab (pass A alone, with the Lanczos epilogue when asked for)
  if (!h->plan.usable) return fail(HXV_ERR_UNSUPPORTED, "all-to-all exchange: tiled kernels unavailable (too many distinct amplitudes)");
  hipError_t e;
  kt_mark(h, 2, st);
  if (real) {
    DevSector d = h->dev;
    d.pitch = (int)pit;
    const double* vbase = reinterpret_cast<const double*>(v) - (int64_t)d.slab0 * d.pitch;  // (pass A addresses its slab as column slots slab0..)
    e = launch_hxv_tiled_real(d, h->plan, vbase, reinterpret_cast<double*>(recv), static_cast<double*>(hv_), st, ep, 1, true, a.d_wtr[1], P);
  } else {
    const double2* vbase = reinterpret_cast<const double2*>(v) - (int64_t)h->dev.slab0 * h->dev.pitch;
    e = launch_hxv_tiled(h->dev, h->plan, vbase, a.d_recv, static_cast<double2*>(hv_), st, ep, 1, true, a.d_wtr[0], P);
  }
  if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  kt_mark(h, 3, st);
  h->n_apply++;
  h->n_exchange += 2;
  return HXV_OK;
}

int apply_slab(hxv_handle* h, const double2* d_v_local, double2* d_hv_local, hipStream_t st, const LzEpilogue* ep) {
  const SectorHost& s = h->host;
  if (s.exchange == 2 && s.nranks > 1) return apply_slab_a2a(h, d_v_local, d_hv_local, false, st, ep);
  const double2* vfull = d_v_local;
  if (s.nranks != 1 || comm_ready(h)) {
    if (!comm_ready(h)) return fail(HXV_ERR_STATE, "split sector without a communicator: call hxv_comm_init after opening the sector");
    int rc = exchange(h, d_v_local, false, st);
    if (rc) return rc;
    vfull = h->gather_cur;
  }
  kt_mark(h, 0, st);
  if (!ep) {
    const int rcp = hxv_apply_device(h, vfull, d_hv_local, st);
    kt_mark(h, 1, st);
    return rcp;
  }
  int rcw = ensure_wt(h);
  if (rcw) return rcw;
  hipError_t e = launch_hxv_tiled(h->dev, h->plan, vfull, h->d_wt, d_hv_local, st, ep);
  if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  kt_mark(h, 1, st);
  h->n_apply++;
  return HXV_OK;
}

// the same on REAL vectors (double[qdw][pitch_real] slabs; half the bytes on the links)
int apply_slab_real(hxv_handle* h, const double* d_v_local, double* d_hv_local, hipStream_t st, const LzEpilogue* ep) {
  const SectorHost& s = h->host;
  if (s.exchange == 2 && s.nranks > 1) return apply_slab_a2a(h, d_v_local, d_hv_local, true, st, ep);
  const double* vfull = d_v_local;
  if (s.nranks != 1 || comm_ready(h)) {
    if (!comm_ready(h)) return fail(HXV_ERR_STATE, "split sector without a communicator: call hxv_comm_init after opening the sector");
    int rc = exchange(h, d_v_local, true, st);
    if (rc) return rc;
    vfull = reinterpret_cast<const double*>(h->gather_cur);
  }
  int rcw = ensure_wt(h);
  if (rcw) return rcw;
  DevSector d = h->dev;
  d.pitch = pitch_real_of(h);
  hipError_t e = launch_hxv_tiled_real(d, h->plan, vfull, (double*)h->d_wt, d_hv_local, st, ep);
  if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  h->n_apply++;
  return HXV_OK;
}

void comm_release(hxv_handle* h) {
  comm_release_transport(h);
  if (h->d_gather) {
    pool_free(h->device, h->d_gather);
    h->d_gather = nullptr;
  }
  for (auto& p : h->d_gather_x)
    if (p) {
      pool_free(h->device, p);
      p = nullptr;
    }
  h->gather_cur = nullptr;
  for (auto& p : h->lz_vec) p = nullptr;
  a2a_release(h);
  if (h->d_send) {
    pool_free(h->device, h->d_send);
    h->d_send = nullptr;
  }
  if (h->d_send_cols) {
    (void)hipFree(h->d_send_cols);
    h->d_send_cols = nullptr;
  }
}

}  // namespace hxv

extern "C" {

int hxv_apply_device_slab(hxv_handle* h, const void* d_v_local, void* d_hv_local, void* stream) {
  if (!h || !d_v_local || !d_hv_local) return fail(HXV_ERR_ARG, "hxv_apply_device_slab: NULL argument");
  if (h->host.panel_rows > 0) return fail(HXV_ERR_STATE, "hxv_apply_device_slab: panel handles only do hxv_apply_dw_panel");
  return apply_slab(h, (const double2*)d_v_local, (double2*)d_hv_local, (hipStream_t)stream);
}

// Measurement: nrep slab products (exchange + kernels, COLLECTIVE on a split sector: every rank calls it with the same nrep) timed with HIP
// events on the handle's stream; *ms_step = mean time of a whole product on this rank, *ms_kernels = mean time of its product kernels alone
// (the panel product and pass A in exchange mode 2) -- what bench.py's roofline leg quotes for N > 1.
int hxv_time_apply_slab(hxv_handle* h, const void* d_v_local, void* d_hv_local, int32_t nrep, float* ms_step, float* ms_kernels) {
  if (!h || !d_v_local || !d_hv_local || nrep < 1 || !ms_step || !ms_kernels) return fail(HXV_ERR_ARG, "hxv_time_apply_slab: bad argument");
  if (h->host.panel_rows > 0) return fail(HXV_ERR_STATE, "hxv_time_apply_slab: not on a panel handle");
  HIPCHK(hipSetDevice(h->device));
  for (auto& e : h->kt_ev)
    if (!e) HIPCHK(hipEventCreate(&e));
  const bool two = h->host.exchange == 2 && h->host.nranks > 1;
  const bool ov = two && h->a2a_overlap && h->plan.usable;  // overlapped mode 2: pass A runs on the second stream, between kt_ev[4] and [5]
  double tot = 0.0, ker = 0.0, ovl = 0.0;
  int rc = HXV_OK;
  h->kt_on = 1;
  for (int i = 0; i < nrep && rc == HXV_OK; ++i) {
    hipError_t e = hipEventRecord(h->ev0, h->stream);
    rc = apply_slab(h, (const double2*)d_v_local, (double2*)d_hv_local, h->stream);
    if (rc) break;
    if (e == hipSuccess) e = hipEventRecord(h->ev1, h->stream);
    if (e == hipSuccess) e = hipEventSynchronize(h->ev1);
    float a = 0, b = 0, c = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&a, h->ev0, h->ev1);
    if (e == hipSuccess) e = hipEventElapsedTime(&b, h->kt_ev[0], h->kt_ev[1]);
    if (e == hipSuccess && two) e = hipEventElapsedTime(&c, h->kt_ev[2], h->kt_ev[3]);
    float d = 0;
    if (e == hipSuccess && ov) e = hipEventElapsedTime(&d, h->kt_ev[4], h->kt_ev[5]);
    if (e != hipSuccess) rc = fail(HXV_ERR_HIP, std::string("hxv_time_apply_slab: ") + hipGetErrorString(e));
    tot += a;
    ker += b + c + d;  // (the kernels' own time: with the overlap, more than their share of the step)
    ovl += d;          // (the part that ran on the SECOND stream, beside the exchange: not to be subtracted from the step when the exchange's
                       //  share is computed -- get_option "time_kernels_overlapped_us")
  }
  h->last_overlapped_us = (int64_t)(ovl / nrep * 1e3);
  h->kt_on = 0;
  if (rc) return rc;
  *ms_step = (float)(tot / nrep);
  *ms_kernels = (float)(ker / nrep);
  return HXV_OK;
}

// Where the exchange wants this rank's slab: its slot of the gather buffer (all-gather) / the front of the halo layout.  A caller that
// builds its vector THERE and passes that pointer to hxv_apply_device_slab saves the slab copy of every product (the vector's other
// slots are overwritten by the exchange; the slab itself is only read).  Complex layout: [qdw columns][pitch].
int hxv_slab_home(hxv_handle* h, void** d_slab) {
  if (!h || !d_slab) return fail(HXV_ERR_ARG, "hxv_slab_home: NULL argument");
  if (h->host.panel_rows > 0) return fail(HXV_ERR_STATE, "hxv_slab_home: not on a panel handle");
  if (h->host.exchange == 2) return fail(HXV_ERR_STATE, "hxv_slab_home: the all-to-all exchange has no gathered vector (any slab buffer serves)");
  HIPCHK(hipSetDevice(h->device));
  int rc = ensure_gather(h, h->stream);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));  // (the buffer is zeroed on the handle's stream)
  const size_t slot = (size_t)h->host.cmax * col_bytes(h, false);
  *d_slab = reinterpret_cast<char*>(h->d_gather) + (h->host.exchange == 1 ? 0 : (size_t)h->host.rank * slot);
  return HXV_OK;
}

int64_t hxv_exchange_count(const hxv_handle* h) { return h ? h->n_exchange : -1; }

// The plan, not the transport: what rank `rank` of an `nranks`-way split of the DimDw axis receives from and sends to every
// peer in the halo exchange, computed from the one-spin matrix H_dw alone (CSR in the reference's convention: 1-based columns, as
// hxv_get_csr returns and spH0dws(1) stores) -- no handle, no device, no communicator.  Lets one process check that rank p's send
// list towards q equals rank q's receive list from p for every pair.
// counts: [nranks] columns per peer; cols: GLOBAL 0-based column indices (recv: slot order = ascending; send: grouped by destination).
int hxv_halo_plan_from_csr(int32_t dimdw, const int64_t* dw_rowptr, const int32_t* dw_cols, int32_t rank, int32_t nranks, int32_t* recv_counts,
                           int32_t* send_counts, int32_t* recv_cols, int32_t* send_cols, int32_t* n_recv, int32_t* n_send) {
  if (dimdw < 1 || !dw_rowptr || !dw_cols || rank < 0 || nranks < 1 || rank >= nranks) return fail(HXV_ERR_ARG, "hxv_halo_plan_from_csr: bad argument");
  if (dw_rowptr[0] != 0) return fail(HXV_ERR_ARG, "hxv_halo_plan_from_csr: rowptr[0] must be 0");
  for (int32_t i = 0; i < dimdw; ++i)
    if (dw_rowptr[i + 1] < dw_rowptr[i]) return fail(HXV_ERR_ARG, "hxv_halo_plan_from_csr: rowptr must be non-decreasing");
  SectorHost s;
  s.dimdw = dimdw;
  s.dw.rowptr.assign(dw_rowptr, dw_rowptr + dimdw + 1);
  s.dw.cols.resize((size_t)dw_rowptr[dimdw]);
  for (size_t p = 0; p < s.dw.cols.size(); ++p) {
    if (dw_cols[p] < 1 || dw_cols[p] > dimdw) return fail(HXV_ERR_ARG, "hxv_halo_plan_from_csr: column index out of range (1-based expected)");
    s.dw.cols[p] = dw_cols[p] - 1;
  }
  s.rank = rank;
  s.nranks = nranks;
  dw_split(s.dimdw, rank, nranks, s.qdw, s.dw0);
  make_halo(s);
  for (int r = 0; r < nranks; ++r) {
    if (recv_counts) recv_counts[r] = s.halo_ptr[r + 1] - s.halo_ptr[r];
    if (send_counts) send_counts[r] = s.send_ptr[r + 1] - s.send_ptr[r];
  }
  if (n_recv) *n_recv = (int32_t)s.halo_cols.size();
  if (n_send) *n_send = (int32_t)s.send_cols.size();
  if (recv_cols) std::copy(s.halo_cols.begin(), s.halo_cols.end(), recv_cols);
  if (send_cols)
    for (size_t k = 0; k < s.send_cols.size(); ++k) send_cols[k] = s.send_cols[k] + s.dw0;  // local -> global
  return HXV_OK;
}

}  // extern "C"
