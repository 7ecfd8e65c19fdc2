// Device Lanczos behind the C-ABI (include/hxv.h): the single-vector recurrences with the SciFortran call shapes
// (sp_lanc_tridiag, sp_lanc_eigh; ED_GF_NORMAL.f90:215-220, ED_DIAG.f90:176-184), the tridiagonalisation with probe overlaps, the paired
// tridiagonalisation with and without them and the iteration timer of bench.py.  (The Green's-function start vectors, c / c^dagger on the ground state, are
// hxv_ladder.hip's.)
// Every driver -- and the local step hxv_eigh_lowest borrows -- takes its fused iteration from ONE function, fused_step_enqueue; the drivers
// differ in who provides s and c (a host upload, or lz_next on the device), in whether there is a previous vector, and in what they read back.
// The recurrence around it is ONE object, LzRunner, with one component or -- the paired drivers -- two, and the host-stepped loop of the single
// and of the paired tridiagonalisation is ONE function over it (host_stepped_loop); the probes' argument check (check_probe_list) and the
// carving of their scratch (ProbeScratch, hxv_call_scope.hpp) are shared with hxv_chebyshev.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "hxv_call_scope.hpp"
#include "hxv_lanczos_host.hpp"
#include "hxv_lanczos_kernels.hpp"

using namespace hxv;

// ===========================================================================================
// Device Lanczos
// ===========================================================================================
namespace {

// sum (op 0) or 2-norm (op 1) of the per-workgroup partials into scal[io]; on a split sector the sums of all ranks are added
int reduce_scalar(hxv_handle* h, const double* partial, int np, int io, int op, double* scal = nullptr) {
  if (!scal) scal = h->d_scalars;
  const bool dist = comm_ready(h);
  hipLaunchKernelGGL(lz_final, dim3(1), dim3(256), 0, h->stream, partial, np, scal, io, dist ? 0 : op);
  if (dist) {
    int rc = comm_allreduce_sum(h, scal + io, 1, h->stream);
    if (rc) return rc;
    if (op) hipLaunchKernelGGL(lz_sqrt, dim3(1), dim3(1), 0, h->stream, scal, io);
  }
  return HXV_OK;
}

// q = w / |w|   (q may be w); the norm stays in scal[slot]
int enqueue_normalise(hxv_handle* h, double2* q, const double2* w, int64_t n, int slot) {
  int rc = enqueue_norm(h, w, n, slot, 1);
  if (rc) return rc;
  hipLaunchKernelGGL(lz_scale, dim3(grid_for(n)), dim3(256), 0, h->stream, n, q, w, h->d_scalars, slot);
  return HXV_OK;
}

// double2 elements of one Lanczos vector of this rank (local slab: qdw == DimDw on an unsplit sector).  REAL-vector mode: the buffers hold
// double[DimDw][pitch_real]; every streaming kernel here is elementwise with real scalars, so it runs unchanged on that buffer viewed as double2
int64_t lz_len(const hxv_handle* h, bool real) {
  return real ? (int64_t)pitch_real_of(h) * h->host.qdw / 2 : (int64_t)h->host.pitch * h->host.qdw;
}
// workgroups of pass A = partial sums its epilogue leaves (a rank without columns launches nothing: one zero stands in)
int64_t lz_pass_a_workgroups(const hxv_handle* h, bool real) {
  return std::max<int64_t>(1, tiled_pass_up_workgroups(h->dev, h->plan, real, dw_part_in_pieces(h)));
}
// room for n partial sums of the epilogue
int ensure_lz_partial(hxv_handle* h, int64_t n) {
  if (n <= h->lz_partial_n) return HXV_OK;
  if (h->d_lz_partial) (void)hipFree(h->d_lz_partial);
  h->d_lz_partial = nullptr;
  h->lz_partial_n = 0;
  HIPCHK(hipMalloc((void**)&h->d_lz_partial, (size_t)n * sizeof(double)));
  HIPCHK(hipMemsetAsync(h->d_lz_partial, 0, (size_t)n * sizeof(double), h->stream));  // (a rank without columns launches nothing)
  h->lz_partial_n = n;
  return HXV_OK;
}

// THE fused Lanczos step, enqueued on the handle's stream; every device driver runs this one sequence, so what they promise each other bit
// for bit (paired = two single runs, captured = host-stepped, local step = normalised step) holds by construction.  With the stored vectors
// q = X_k, qm = X_{k-1} (null: no previous vector, c is not read) and s = scal[LZ_S], c = scal[LZ_C] ALREADY in device memory -- uploaded by
// the caller or left there by lz_next -- pass A's epilogue stores  w = s*H q - c*qm  and the partial sums of  alpha = <s q, w>  -> scal[LZ_ALPHA];
// with sub_alpha one more pass subtracts (alpha*s) q and reduces  beta = |w|  -> scal[LZ_BETA].  On a split sector alpha and beta are summed
// over the ranks.  pair: Re and Im of the vectors are two independent real recurrences, the second one's scalars LZ_PAIR behind the first's.
// Nothing here allocates, copies or synchronises once the buffers have their size, so the sequence can be captured into a hipGraph: the
// product's scratch and the partial sums grow on the first call (iteration 0 always runs uncaptured), and apply_slab's event marks are only
// armed inside hxv_time_apply_slab.
int fused_step_enqueue(hxv_handle* h, bool real, const double2* q, const double2* qm, double2* w, double* scal, bool pair, bool sub_alpha = true) {
  const int64_t n2 = lz_len(h, real), nwg = lz_pass_a_workgroups(h, real);
  const int g = grid_for(n2), nc = pair ? 2 : 1;
  int rc = ensure_lz_partial(h, nc * nwg);
  if (rc) return rc;
  LzEpilogue ep;
  ep.xm = qm;
  ep.scal = scal;
  ep.i_s = LZ_S;
  ep.i_c = LZ_C;
  ep.partial = h->d_lz_partial;
  if (pair) {
    ep.pair = 1;
    ep.i_s2 = LZ_PAIR + LZ_S;
    ep.i_c2 = LZ_PAIR + LZ_C;
    ep.partial2 = h->d_lz_partial + nwg;
  }
  // (apply_slab = exchange + product on a split sector, the plain product otherwise)
  rc = real ? apply_slab_real(h, (const double*)q, (double*)w, h->stream, &ep) : apply_slab(h, q, w, h->stream, &ep);
  for (int c = 0; c < nc && !rc; ++c) rc = reduce_scalar(h, h->d_lz_partial + c * nwg, (int)nwg, c * LZ_PAIR + LZ_ALPHA, 0, scal);
  if (rc || !sub_alpha) return rc;
  for (int c = 0; c < nc; ++c)  // alpha*s: the coefficient of the STORED q
    hipLaunchKernelGGL(lz_mul, dim3(1), dim3(1), 0, h->stream, scal, c * LZ_PAIR + LZ_ALPHA_S, c * LZ_PAIR + LZ_ALPHA, c * LZ_PAIR + LZ_S);
  double* pb[2] = {h->d_partials + RED_BLOCKS, h->d_partials};
  if (pair)
    hipLaunchKernelGGL(lz_sub_nrm_pair, dim3(g), dim3(256), 0, h->stream, n2, w, q, scal, LZ_ALPHA_S, LZ_PAIR + LZ_ALPHA_S, pb[0], pb[1]);
  else
    hipLaunchKernelGGL(lz_sub_nrm, dim3(g), dim3(256), 0, h->stream, n2, w, q, scal, LZ_ALPHA_S, pb[0]);
  for (int c = 0; c < nc && !rc; ++c) rc = reduce_scalar(h, pb[c], g, c * LZ_PAIR + LZ_BETA, 1, scal);
  return rc;
}

struct LzBuf {
  double2 *q, *qm, *w;
};

// Lanczos recurrence on device.  Two implementations of one step:
//  * plain : w = H q (any kernel), then lz_sub_dot / lz_sub_nrm / lz_scale on normalised vectors;
//  * fused : vectors are kept UNNORMALISED (q_k = s*X, s = 1/beta_k) and go through fused_step_enqueue.
//            144 B/state per iteration instead of 224.
// One component, or -- the paired drivers -- two: Re and Im of the vectors are two independent real recurrences on one product, each with its
// own scale factors, the second one's scalars LZ_PAIR behind the first one's in a block of 2*LZ_PAIR doubles the call brings.  Two components
// exist for the fused recurrence on complex vectors only; the plain recurrence and the device-only run are single-component.
struct LzRunner {
  hxv_handle* h;
  LzBuf b;
  int nc;               // components
  bool fused;
  bool real;            // REAL-vector mode (see lz_len)
  int64_t n2;           // double2 elements of one vector
  double* scal;         // the LzSlot block(s) in device memory
  bool first = true;
  LzScale sc[2];        // q = sc[c].s_cur * (component c of b.q) (fused) ; 1 (plain)
  bool alive[2] = {true, true};  // a component retire()d after a breakdown is multiplied away (s = c = 0): the other one goes on alone
  double last_beta[2] = {0.0, 0.0};

  // pair_scal: null, or the 2*LZ_PAIR scalars of a two-component run (which is fused whatever the plan: its driver has checked the option)
  LzRunner(hxv_handle* hh, double2* x, double2* xm, double2* w, bool real_vec = false, double* pair_scal = nullptr)
      : h(hh), b{x, xm, w}, nc(pair_scal ? 2 : 1), fused(pair_scal || lanczos_local_step_available(hh)), real(real_vec), n2(lz_len(hh, real_vec)),
        scal(pair_scal ? pair_scal : hh->d_scalars) {
    hh->last_real = nc == 2 ? 2 : real ? 1 : 0;
  }

  // b.q holds a vector of norm `nrm`, its second component one of norm `nrm_b` (pass 1.0 if already normalised)
  int begin(double nrm, double nrm_b = 1.0) {
    first = true;
    sc[0].begin(nrm);
    sc[1].begin(nrm_b);
    alive[0] = alive[1] = true;
    if (nc == 2 && real) return fail(HXV_ERR_STATE, "the paired Lanczos recurrence runs on complex vectors");
    if (!fused && nrm != 1.0) return fail(HXV_ERR_STATE, "plain Lanczos expects a normalised start vector");
    return HXV_OK;
  }

  // The library's own start vector: the deterministic one of `seed` in the run's layout (built in b.w), normalised into b.q; clears the scalars
  int begin_own(uint64_t seed) {
    if (real)
      launch_init_real(h, (double*)b.w, seed, h->stream);
    else
      launch_init(h, b.w, seed, h->stream);
    HIPCHK(hipMemsetAsync(h->d_scalars, 0, 8 * sizeof(double), h->stream));
    int rc = enqueue_normalise(h, b.q, b.w, n2, LZ_BETA);
    return rc ? rc : begin(1.0);
  }

  // one step: alpha[c], beta[c] of every component c < nc (those of a retired one mean nothing)
  int step(double* alpha, double* beta) {
    const int64_t n = n2;
    const int g = grid_for(n);
    int rc;
    double up[2][2], host[2 * LZ_PAIR];
    if (!fused) {
      // (apply_slab = exchange + product on a split sector, the plain product otherwise)
      rc = real ? apply_slab_real(h, (const double*)b.q, (double*)b.w, h->stream) : apply_slab(h, b.q, b.w, h->stream);
      if (rc) return rc;
      hipLaunchKernelGGL(lz_sub_dot, dim3(g), dim3(256), 0, h->stream, n, b.w, b.qm, b.q, h->d_scalars, first ? -1 : (int)LZ_S, h->d_partials);
      rc = reduce_scalar(h, h->d_partials, g, LZ_ALPHA, 0);
      if (rc) return rc;
      hipLaunchKernelGGL(lz_sub_nrm, dim3(g), dim3(256), 0, h->stream, n, b.w, b.q, h->d_scalars, LZ_ALPHA, h->d_partials + RED_BLOCKS);
      rc = reduce_scalar(h, h->d_partials + RED_BLOCKS, g, LZ_BETA, 1);
    } else {
      for (int c = 0; c < nc; ++c) {  // -> LZ_S, LZ_C of each component
        up[c][0] = alive[c] ? sc[c].s_cur : 0.0;
        up[c][1] = (first || !alive[c]) ? 0.0 : sc[c].c();
        HIPCHK(hipMemcpyAsync(scal + c * LZ_PAIR + LZ_S, up[c], 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
      }
      rc = fused_step_enqueue(h, real, b.q, first ? nullptr : b.qm, b.w, scal, nc == 2);
    }
    if (rc) return rc;
    // one component: alpha and beta, which lie side by side; two: both blocks in one copy
    const int lo = nc == 2 ? 0 : LZ_ALPHA, cnt = nc == 2 ? 2 * LZ_PAIR : 2;
    HIPCHK(hipMemcpyAsync(host + lo, scal + lo, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int c = 0; c < nc; ++c) {
      alpha[c] = host[c * LZ_PAIR + LZ_ALPHA];
      beta[c] = last_beta[c] = host[c * LZ_PAIR + LZ_BETA];
    }
    return HXV_OK;
  }

  // may a fixed-length run of nmax iterations without probes hand iterations 1..nmax-1 to the device (run_device_only)?  Serial sectors: the
  // all-reduces of a split one go through the host loop.
  bool device_only_ok(int nmax) const { return nc == 1 && fused && h->lz_graph && nmax >= 8 && !comm_ready(h); }

  // Iterations 1..nmax-1 of a fixed-length run on the device alone (after the hand-over of run_device_only): each one is the fused step on the
  // scalars lz_next left, then lz_next; alpha/beta go to device arrays.  The three-iteration pointer-rotation cycle is captured ONCE into a
  // hipGraph and replayed, so a small sector pays one graph launch per three iterations instead of ~9 kernel launches, two copies and a
  // synchronisation per iteration.  Leaves b.q/b.qm/b.w as after the last iteration.
  int run_device_iterations(int nmax, double* d_alpha, double* d_beta) {
    double2* buf[3] = {b.q, b.w, b.qm};  // iteration k uses q = buf[k%3] (k counted from 1: q = former w), w = buf[(k+1)%3], qm = buf[(k+2)%3]
    // after step() of iteration 0 and before any rotation: X_1 = b.w, X_0 = b.q, free = b.qm
    int k = 1;
    auto one = [&](int kk) -> int {
      int rc = fused_step_enqueue(h, real, buf[kk % 3], buf[(kk + 2) % 3], buf[(kk + 1) % 3], h->d_scalars, false);
      if (rc) return rc;
      hipLaunchKernelGGL(lz_next, dim3(1), dim3(1), 0, h->stream, h->d_scalars, d_alpha, d_beta, nmax);
      return HXV_OK;
    };
    const int cycles = (nmax - 1) / 3;
    if (cycles >= 2) {
      hipGraph_t graph = nullptr;
      hipGraphExec_t exec = nullptr;
      HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
      int rc = HXV_OK;
      for (int u = 0; u < 3 && rc == HXV_OK; ++u) rc = one(k + u);
      hipError_t ec = hipStreamEndCapture(h->stream, &graph);
      if (rc) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
      }
      if (ec != hipSuccess) return fail(HXV_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ec));
      ec = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
      if (ec != hipSuccess) {
        (void)hipGraphDestroy(graph);
        return fail(HXV_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ec));
      }
      for (int cy = 0; cy < cycles; ++cy) {
        ec = hipGraphLaunch(exec, h->stream);
        if (ec != hipSuccess) break;
      }
      k += 3 * cycles;  // (k-1) % 3 is unchanged: the remainder below continues the same rotation
      (void)hipGraphExecDestroy(exec);
      (void)hipGraphDestroy(graph);
      if (ec != hipSuccess) return fail(HXV_ERR_HIP, std::string("hipGraphLaunch: ") + hipGetErrorString(ec));
    }
    for (; k < nmax; ++k) {
      int rc = one(k);
      if (rc) return rc;
    }
    b.q = buf[(nmax - 1) % 3];
    b.w = buf[nmax % 3];
    b.qm = buf[(nmax + 1) % 3];
    first = false;
    return HXV_OK;
  }

  // The whole device-only run after step() of iteration 0 returned `beta`: the device arrays of alpha and beta (nmax each, zeroed, freed on
  // every way out), the hand-over -- the scalars of iteration 1 and the step counter go to device memory, where lz_next keeps them from then
  // on --, iterations 1..nmax-1 three per hipGraph.  ab (may be null): 2*nmax host doubles that receive the two arrays.  ev (may be null:
  // hxv_time_lanczos's pair): ev[0] is recorded after the hand-over and before the first captured iteration, ev[1]
  // after the last one, and waited for.
  int run_device_only(double beta, int nmax, double* ab, hipEvent_t* ev, const char* who) {
    if (nc != 1) return fail(HXV_ERR_STATE, std::string(who) + ": the device-only run is single-component");
    CallScope scratch(h);
    double* d_ab = nullptr;
    HIPCHK(scratch.take_device((size_t)2 * nmax * sizeof(double), &d_ab));
    HIPCHK(hipMemsetAsync(d_ab, 0, (size_t)2 * nmax * sizeof(double), h->stream));
    const double s1 = 1.0 / beta, bprev = 1.0 / sc[0].s_cur;
    const double init[2] = {s1, 1.0 / (s1 * bprev)};   // s_1 = 1/beta_1 ; c_1 = beta_1/beta_0, rounded like LzScale::next() + c()
    const double one = 1.0;
    hipError_t e = hipMemcpyAsync(h->d_scalars + LZ_S, init, 2 * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h->d_scalars + LZ_STEP, &one, sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // (init and one are read by asynchronous copies)
    if (e == hipSuccess && ev) e = hipEventRecord(ev[0], h->stream);
    if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    int rc = run_device_iterations(nmax, d_ab, d_ab + nmax);
    if (rc) return rc;
    if (ev) {
      e = hipEventRecord(ev[1], h->stream);
      if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
      if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    if (ab) {
      e = hipMemcpyAsync(ab, d_ab, (size_t)2 * nmax * sizeof(double), hipMemcpyDeviceToHost, h->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
      if (e != hipSuccess) return fail(HXV_ERR_HIP, std::string("reading alpha/beta back: ") + hipGetErrorString(e));
    }
    return HXV_OK;
  }

  // rotate to the next Lanczos vector (needs the beta returned by step())
  int advance() {
    const int64_t n = n2;
    if (!fused) {
      HIPCHK(hipMemcpyAsync(h->d_scalars + LZ_S, h->d_scalars + LZ_BETA, sizeof(double), hipMemcpyDeviceToDevice, h->stream));  // (plain: LZ_S holds beta_k)
      std::swap(b.q, b.qm);
      hipLaunchKernelGGL(lz_scale, dim3(grid_for(n)), dim3(256), 0, h->stream, n, b.q, b.w, h->d_scalars, LZ_S);
    } else {
      double2* old_m = b.qm;
      b.qm = b.q;      // X_{k-1}
      b.q = b.w;       // X_k = unnormalised residual
      b.w = old_m;
      for (int c = 0; c < nc; ++c)
        if (alive[c]) sc[c].next(last_beta[c]);
    }
    first = false;
    return HXV_OK;
  }
  // component c's Krylov space has closed: it makes no further step
  void retire(int c) { alive[c] = false; }
  bool any_alive() const { return alive[0] || (nc == 2 && alive[1]); }

  // current normalised Lanczos vector = scale() * vec(), per component
  const double2* vec() const { return b.q; }
  double scale(int c = 0) const { return fused ? sc[c].s_cur : 1.0; }
};

// the three work vectors of the single-vector Lanczos; `real` = layout of the coming run.  The pad rows of the two
// layouts sit at different places and must be zero (the reductions run over the padded arrays, the products never
// write pads), so the buffers are cleared whenever the layout changes.
int ensure_lz(hxv_handle* h, bool real) {
  if (int rcc = need_comm(h, "device Lanczos")) return rcc;
  HIPCHK(hipSetDevice(h->device));
  const size_t bytes = (size_t)h->host.pitch * std::max(h->host.qdw, 1) * sizeof(double2);
  if (comm_ready(h) && h->host.nranks > 1 && h->lz_inplace && h->host.exchange != 2) {
    // split sector: the three vectors live where the exchange wants the slab, in three gather buffers (hxv_exchange.cpp); when the memory for
    // them is not there the slab buffers below serve, with one slab copy per product
    int rc = comm_lz_homes(h, real, h->lz_vec);
    if (rc == HXV_OK) {
      h->lz_buf_mode = real ? 1 : 0;
      return HXV_OK;
    }
    if (rc != HXV_ERR_HIP) return rc;
  }
  for (auto& p : h->d_lz)
    if (!p) {
      HIPCHK(pool_alloc(h->device, bytes, (void**)&p));
      // on the handle's (non-blocking) stream: a null-stream memset is not ordered with the kernels that follow and could
      // land on a recycled pool block after the start vector had been written into it
      HIPCHK(hipMemsetAsync(p, 0, bytes, h->stream));
      h->device_bytes += (int64_t)bytes;
    }
  if (h->lz_buf_mode != (real ? 1 : 0)) {
    for (auto& p : h->d_lz) HIPCHK(hipMemsetAsync(p, 0, bytes, h->stream));
    h->lz_buf_mode = real ? 1 : 0;
  }
  for (int i = 0; i < 3; ++i) h->lz_vec[i] = h->d_lz[i];
  return HXV_OK;
}

// A start vector that lives in one of the handle's gather buffers (built at hxv_slab_home) would be zeroed by ensure_lz, which clears the
// slab's place in all three before the driver reads its input: such a vector is copied to a staging slab first (one slab copy per RUN).
// The staging buffer belongs to the call's scope, which returns it after the run.
int stage_start_vector(hxv_handle* h, const void*& d_vin, CallScope& pooled) {
  if (!comm_ready(h) || !comm_in_gather(h, d_vin)) return HXV_OK;
  const size_t bytes = (size_t)h->host.pitch * std::max(h->host.qdw, 1) * sizeof(double2);
  void* tmp = nullptr;
  HIPCHK(pooled.take(bytes, &tmp));
  HIPCHK(hipMemcpyAsync(tmp, d_vin, bytes, hipMemcpyDeviceToDevice, h->stream));
  d_vin = tmp;
  return HXV_OK;
}

// The probes of a run and where their overlaps go: which kernel takes the overlaps of a stored vector (lz_probe_dots<M, REAL> on complex or real
// vectors, or -- `pair` -- lz_probe_dots_pair<M> with the real probes shared by both components) and how the 2*m sums of a step map to a
// component's row of the caller's overlaps array.  m = 0: no probes, nothing is launched.  part, sums: ProbeScratch's.
struct LzProbeSet {
  int m = 0;
  bool real = false, pair = false;
  LzProbes pr{};       // single runs: complex vectors, or real ones viewed as double2
  LzRealProbes rp{};   // paired runs
  double *part = nullptr, *sums = nullptr;
  // sums[2*m] = the overlaps of x (n double2 elements of this rank) with the probes: ONE all-reduce for them on a split sector
  int enqueue(hxv_handle* h, int64_t n, const double2* x) const {
    if (pair)
      launch_probe_dots_pair(grid_for(n), h->stream, m, n, x, rp, part, sums);
    else if (real)
      launch_probe_dots<true>(grid_for(n), h->stream, m, n, x, pr, part, sums);
    else
      launch_probe_dots<false>(grid_for(n), h->stream, m, n, x, pr, part, sums);
    return comm_allreduce_sum(h, sums, (size_t)2 * m, h->stream);
  }
  // ov[2*m] of component c: the staged sums times s.  Single: (Re, Im) <p_j|x> as they lie.  Paired: the sums are <p_j|Re x>, <p_j|Im x>; component
  // c's go to the real slots, the imaginary ones stay the zeros the driver wrote.
  void store(const double* stage, int c, double s, double* ov) const {
    if (pair)
      for (int j = 0; j < m; ++j) ov[2 * j] = stage[2 * j + c] * s;
    else
      for (int j = 0; j < 2 * m; ++j) ov[j] = stage[j] * s;
  }
};

// what a tridiagonalisation returns per component: alanc[nlanc], blanc[nlanc], overlaps[2*nlanc*m] (null without probes), nsteps
struct LzOut {
  double *al, *bl, *ov;
  int nsteps = 0;
  void clear(int nlanc, int m) const {
    for (int k = 0; k < nlanc; ++k) al[k] = bl[k] = 0.0;
    for (size_t i = 0; i < (size_t)2 * nlanc * m; ++i) ov[i] = 0.0;
  }
};

// THE host-stepped loop of both tridiagonalisation drivers, over a runner that has begun: per step the overlaps of the STORED vector X_k,
// enqueued before the step that overwrites nothing of it -- one all-reduce, one copy into this step's slot of h->h_probe_ov (a slot per step:
// nothing is overwritten while a copy is in flight), which completes with the synchronisation step() makes for alpha and beta --, then the
// step, then per live component alpha, beta and the overlaps of q_k = s * X_k with the s of BEFORE the step, the breakdown rule, and the
// rotation.  out[c].nsteps = the steps component c made.
int host_stepped_loop(hxv_handle* h, LzRunner& lz, const LzProbeSet& pb, int nlanc, double threshold, LzOut* out) {
  const int m = pb.m;
  for (int k = 0; k < nlanc && lz.any_alive(); ++k) {
    double* stage = m > 0 ? h->h_probe_ov + (size_t)2 * m * k : nullptr;
    if (m > 0) {
      int rc = pb.enqueue(h, lz.n2, lz.vec());
      if (rc) return rc;
      HIPCHK(hipMemcpyAsync(stage, pb.sums, (size_t)2 * m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    const double s[2] = {lz.scale(0), lz.scale(1)};
    double a[2], bt[2];
    int rc = lz.step(a, bt);
    if (rc) return rc;
    for (int c = 0; c < lz.nc; ++c) {
      if (!lz.alive[c]) continue;
      if (m > 0) pb.store(stage, c, s[c], out[c].ov + (size_t)2 * m * k);
      out[c].al[k] = a[c];
      if (k + 1 < nlanc) out[c].bl[k + 1] = bt[c];
      out[c].nsteps = k + 1;
      // breakdown of this component's Krylov space.  The paired run also retires a component whose beta is not finite, so that the other one
      // goes on; the single run has no other one and, as sp_lanc_tridiag does, goes on to nlanc.
      if (std::fabs(bt[c]) < threshold || (lz.nc == 2 && !std::isfinite(bt[c]))) lz.retire(c);
    }
    // (not after the last step: the plain recurrence's advance() launches a kernel)
    if (k + 1 < nlanc && lz.any_alive() && (rc = lz.advance())) return rc;
  }
  return HXV_OK;
}

}  // namespace

namespace hxv {
// scal[slot] = |x|^2 (op 0) or |x| (op 1) of the n double2 elements of x, over all ranks of a split sector
int enqueue_norm(hxv_handle* h, const double2* x, int64_t n, int slot, int op) {
  const int g = grid_for(n);
  hipLaunchKernelGGL(lz_nrm, dim3(g), dim3(256), 0, h->stream, n, x, h->d_partials + RED_BLOCKS);
  return reduce_scalar(h, h->d_partials + RED_BLOCKS, g, slot, op);
}
void launch_to_real(const hxv_handle* h, const double2* src, double* dst, hipStream_t st) {
  const int pr = pitch_real_of(h);
  hipLaunchKernelGGL(lz_to_real, dim3(grid_for((int64_t)pr * h->host.qdw)), dim3(256), 0, st, h->host.dimup, h->host.qdw, h->host.pitch, pr,
                     src, dst, (double*)nullptr);
}
void launch_to_complex(const hxv_handle* h, const double* src, double2* dst, hipStream_t st) {
  hipLaunchKernelGGL(lz_to_complex, dim3(grid_for((int64_t)h->host.pitch * h->host.qdw)), dim3(256), 0, st, h->host.dimup, h->host.qdw,
                     h->host.pitch, pitch_real_of(h), src, dst);
}
// may a Lanczos run on this handle use real vectors?  (a start vector the caller brings must be purely real as well)
bool want_real(const hxv_handle* h) { return h->real_vectors && !real_mode_blocker(h); }
int need_comm(const hxv_handle* h, const char* who) {
  if (h->host.nranks == 1 || comm_ready(h)) return HXV_OK;
  return fail(HXV_ERR_STATE, std::string(who) + " on a split sector needs the communicator: call hxv_comm_init after opening the sector");
}
int check_probe_list(const hxv_handle* h, const char* who, int nprobes, const void* const* d_probes, bool have_outputs, const char* outputs,
                     const char* why_gather) {
  const std::string w = std::string(who) + ": ";
  if (nprobes < 0 || nprobes > HXV_MAX_PROBES) return fail(HXV_ERR_ARG, w + "nprobes must be 0 .. HXV_MAX_PROBES (8)");
  if (nprobes > 0 && (!d_probes || !have_outputs)) return fail(HXV_ERR_ARG, w + "nprobes > 0 needs the probe list and " + outputs);
  for (int j = 0; j < nprobes; ++j) {
    if (!d_probes[j]) return fail(HXV_ERR_ARG, w + "NULL entry in the probe list");
    if (comm_ready(h) && comm_in_gather(h, d_probes[j])) return fail(HXV_ERR_ARG, w + "a probe lies in a gather buffer of the handle (hxv_slab_home): " + why_gather);
  }
  return HXV_OK;
}
// may this handle use the fused product?  (split sectors included: the epilogue's partial sums are this rank's share, alpha and beta are
// all-reduced.)  When not, the drivers run the plain recurrence and hxv_eigh_lowest measures its two local projections itself.
bool lanczos_local_step_available(const hxv_handle* h) {
  return h->kernel == 1 && h->plan.usable && (!h->dev.nd.active || nd_folds(h->dev)) && h->plan.opt.passes == 3 && h->plan.opt.debug == 0 && h->lz_fused;
}

// The fused step for callers that keep their own basis (hxv_eigh_lowest), on an UNNORMALISED pair: q = sq * (unit q_j),
// qm = sqm * (unit q_{j-1}), qm may be null.  The product's epilogue stores   w = H q / sq - (beta / sqm) qm   and reduces
// alpha = <q / sq, w>;  with sub_alpha one more pass subtracts alpha (q / sq) and measures |w|, otherwise w is left as it is and *nrm_w is
// not set (the caller subtracts alpha together with other projections).  Scale factors 1.0 give the step on normalised vectors.
int lanczos_local_step(hxv_handle* h, bool real, const double2* q, double sq, const double2* qm, double sqm, double beta, double2* w,
                       bool sub_alpha, double* alpha, double* nrm_w) {
  const double up[2] = {1.0 / sq, qm ? beta / sqm : 0.0};  // -> LZ_S, LZ_C
  HIPCHK(hipMemcpyAsync(h->d_scalars + LZ_S, up, 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  int rc = fused_step_enqueue(h, real, q, qm, w, h->d_scalars, false, sub_alpha);
  if (rc) return rc;
  double host[2] = {0.0, 0.0};
  HIPCHK(hipMemcpyAsync(host, h->d_scalars + LZ_ALPHA, (sub_alpha ? 2 : 1) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *alpha = host[0];
  if (sub_alpha && nrm_w) *nrm_w = host[1];
  return HXV_OK;
}

void launch_init(const hxv_handle* h, double2* q, uint64_t seed, hipStream_t st) {
  const int64_t n = (int64_t)h->host.pitch * h->host.qdw;
  hipLaunchKernelGGL(lz_init, dim3(grid_for(n)), dim3(256), 0, st, n, q, seed, h->host.dimup, h->host.pitch, h->host.dw0, h->dev.up_iperm, h->dev.up_sign);
}
void launch_init_real(const hxv_handle* h, double* q, uint64_t seed, hipStream_t st) {
  const int64_t n = (int64_t)pitch_real_of(h) * h->host.qdw;
  hipLaunchKernelGGL(lz_init_real, dim3(grid_for(n)), dim3(256), 0, st, n, q, seed, h->host.dimup, pitch_real_of(h), h->host.dw0, h->dev.up_iperm, h->dev.up_sign);
}
}  // namespace hxv

namespace {
// THE tridiagonalisation driver behind hxv_lanczos_tridiag (nprobes = 0) and hxv_lanczos_tridiag_probes: start-up, then the host-stepped loop
// with the overlaps <p_j|q_k> of every Lanczos vector collected on the way, or -- a fixed-length run without probes on a serial sector -- the
// device-only run.  who: the entry's name, for the messages.  rc_args: what the entry decided from its own arguments; it goes INTO the first
// agreement (split sector: a rank whose arguments are bad tells its peers instead of leaving them in the first all-reduce), so nothing here
// looks at an argument before that agreement.  Collectives of a split sector: agree, the all-reduce of the real check when one is made, agree.
int tridiag_run(hxv_handle* h, const char* who, int rc_args, const void* d_vin, int nprobes, const void* const* d_probes, int nlanc,
                double* alanc, double* blanc, double* overlaps, double threshold, int32_t* nsteps) {
  HIPCHK(hipSetDevice(h->device));  // (before the first collective: thread ranks on several GPUs each have their own current device)
  // scratch of a run WITH probes (ProbeScratch): the real-vector check's partials are a row of RED_BLOCKS for the start vector and one per probe,
  // side by side; a slot of 2*nprobes staged sums per step.  Without probes the check's partials are the handle's own.
  ProbeScratch ws;
  CallScope pooled(h);  // (with the staged start vector and the real-mode copies of the probes)
  // what a rank decides from its own arguments and resources, agreed on before the first collective
  auto resources = [&]() -> int {
    if (rc_args || nprobes == 0) return rc_args;
    return ws.take(h, pooled, (size_t)(1 + nprobes) * RED_BLOCKS, (size_t)2 * nprobes * RED_BLOCKS, (size_t)2 * nprobes, (int64_t)2 * nprobes * nlanc);
  };
  if (int rca = comm_agree(h, resources())) return rca;
  if (int rcc = need_comm(h, "device Lanczos")) return rcc;
  double* d_chk = nprobes ? ws.chk : h->d_partials;
  const int64_t n = (int64_t)h->host.pitch * h->host.qdw;  // this rank's slab
  const size_t real_bytes = (size_t)pitch_real_of(h) * std::max(h->host.qdw, 1) * sizeof(double);
  double* real_probe[HXV_MAX_PROBES] = {};
  // REAL-vector mode: H real and the start vector purely real (c / c^dagger applied to a real ground state is) AND every probe purely real ->
  // the whole recurrence stays real; alanc/blanc are the same numbers at half the bytes per pass.  The sum of Im^2 over the start vector and
  // the probes, over ALL ranks, in ONE reduction (dst = null: reduction only): every rank must take the same path
  bool real = want_real(h);
  int rc_pre = HXV_OK;
  if (real) {
    const int pr = pitch_real_of(h);
    const int g = grid_for((int64_t)pr * h->host.qdw);
    for (int j = 0; j <= nprobes; ++j)
      hipLaunchKernelGGL(lz_to_real, dim3(g), dim3(256), 0, h->stream, h->host.dimup, h->host.qdw, h->host.pitch, pr,
                         (const double2*)(j ? d_probes[j - 1] : d_vin), (double*)nullptr, d_chk + (size_t)j * g);
    // (a rank that fails here must still meet its peers in the agreement below, not leave them there: ADVICE r4)
    rc_pre = reduce_scalar(h, d_chk, (1 + nprobes) * g, LZ_TMP, 0);
    double im2 = 0.0;
    if (!rc_pre && hipMemcpyAsync(&im2, h->d_scalars + LZ_TMP, sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc_pre = fail(HXV_ERR_HIP, std::string(who) + ": reading the real-vector check failed");
    if (!rc_pre && hipStreamSynchronize(h->stream) != hipSuccess) rc_pre = fail(HXV_ERR_HIP, std::string(who) + ": the real-vector check failed");
    real = im2 == 0.0;
  }
  auto prepare = [&]() -> int {
    if (rc_pre) return rc_pre;
    int r = stage_start_vector(h, d_vin, pooled);  // (a start vector at hxv_slab_home: staged before its home is cleared)
    if (!r) r = ensure_lz(h, real);
    for (int j = 0; real && j < nprobes && !r; ++j) HIPCHK(pooled.take(real_bytes, &real_probe[j]));
    return r;
  };
  int rc = comm_agree(h, prepare());  // (a rank that could not allocate tells its peers before the first all-reduce)
  if (rc) return rc;
  LzRunner lz(h, h->lz_vec[0], h->lz_vec[1], h->lz_vec[2], real);
  LzProbeSet pb;
  pb.m = nprobes;
  pb.real = real;
  pb.part = ws.part;
  pb.sums = ws.sums;
  for (int j = 0; j < nprobes; ++j) {
    if (real) launch_to_real(h, (const double2*)d_probes[j], real_probe[j], h->stream);
    pb.pr.p[j] = real ? (const double2*)real_probe[j] : (const double2*)d_probes[j];
  }
  if (real)
    launch_to_real(h, (const double2*)d_vin, (double*)lz.b.q, h->stream);
  else
    HIPCHK(hipMemcpyAsync(lz.b.q, d_vin, (size_t)n * sizeof(double2), hipMemcpyDeviceToDevice, h->stream));
  {  // measure the (global) norm and normalise only when it is not 1 (start_norm)
    rc = enqueue_norm(h, lz.b.q, lz.n2, LZ_TMP, 1);
    if (rc) return rc;
    double nrm = 0.0;
    HIPCHK(hipMemcpyAsync(&nrm, h->d_scalars + LZ_TMP, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!(nrm > 0.0) || !std::isfinite(nrm)) return fail(HXV_ERR_ARG, std::string(who) + ": the start vector is zero or not finite");
    nrm = start_norm(nrm);
    if (nrm != 1.0 && !lz.fused) {  // (the fused recurrence carries the scale factor; the plain one wants a unit vector)
      hipLaunchKernelGGL(lz_scale, dim3(grid_for(lz.n2)), dim3(256), 0, h->stream, lz.n2, lz.b.q, lz.b.q, h->d_scalars, LZ_TMP);
      nrm = 1.0;
    }
    rc = lz.begin(nrm);
  }
  if (rc) return rc;
  LzOut out{alanc, blanc, overlaps};
  out.clear(nlanc, nprobes);
  if (nprobes == 0 && lz.device_only_ok(nlanc)) {
    // Fixed-length run without probes (the Green's-function use, ED_GF_NORMAL.f90:204-220): iteration 0 with the host in the loop, the other
    // nlanc-1 on the device alone -- scalars stay in device memory, the pointer-rotation cycle of three iterations is one hipGraph -- and
    // alpha/beta come back once at the end.  A breakdown (beta < threshold) is found afterwards; whatever was computed past it is discarded.
    rc = lz.step(&alanc[0], &blanc[1]);
    if (rc) return rc;
    int k = 1;
    if (std::fabs(blanc[1]) >= threshold) {
      std::vector<double> ab((size_t)2 * nlanc, 0.0);
      rc = lz.run_device_only(blanc[1], nlanc, ab.data(), nullptr, who);
      if (rc) return rc;
      for (; k < nlanc; ++k) {
        alanc[k] = ab[k];
        const double b1 = k + 1 < nlanc ? ab[(size_t)nlanc + k + 1] : 1.0;
        if (k + 1 < nlanc) blanc[k + 1] = b1;
        if (!std::isfinite(alanc[k]) || !std::isfinite(b1) || (k + 1 < nlanc && std::fabs(b1) < threshold)) {
          if (!std::isfinite(alanc[k])) alanc[k] = 0.0;
          if (k + 1 < nlanc && !std::isfinite(b1)) blanc[k + 1] = 0.0;
          ++k;
          break;
        }
      }
    }
    out.nsteps = k;
  } else if ((rc = host_stepped_loop(h, lz, pb, nlanc, threshold, &out))) {
    return rc;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  if (nsteps) *nsteps = out.nsteps;
  return HXV_OK;
}
}  // namespace

extern "C" {

int hxv_lanczos_tridiag(hxv_handle* h, const void* d_vin, int32_t nlanc, double* alanc, double* blanc, double threshold,
                        int32_t* nsteps) {
  if (!h) return fail(HXV_ERR_ARG, "hxv_lanczos_tridiag: NULL handle");
  const int rc_args = (!d_vin || nlanc < 1 || !alanc || !blanc) ? fail(HXV_ERR_ARG, "hxv_lanczos_tridiag: bad argument") : HXV_OK;
  return tridiag_run(h, "hxv_lanczos_tridiag", rc_args, d_vin, 0, nullptr, nlanc, alanc, blanc, nullptr, threshold, nsteps);
}

// The tridiagonalisation with the overlaps <p_j|q_k> of every Lanczos vector (include/hxv.h): the off-diagonal Green's functions G_ij of one
// orbital i from ONE run instead of the reference's mixed channels (ED_GF_NORMAL.f90:315-903).
int hxv_lanczos_tridiag_probes(hxv_handle* h, const void* d_vin, int32_t nprobes, const void* const* d_probes, int32_t nlanc, double* alanc,
                               double* blanc, double* overlaps, double threshold, int32_t* nsteps) {
  if (!h) return fail(HXV_ERR_ARG, "hxv_lanczos_tridiag_probes: NULL handle");
  auto check_args = [&]() -> int {
    if (!d_vin || nlanc < 1 || !alanc || !blanc || !nsteps) return fail(HXV_ERR_ARG, "hxv_lanczos_tridiag_probes: bad argument (NULL start vector or output, or nlanc < 1)");
    // (ensure_lz clears the slab's place in the gather buffers; a START vector there is staged, a probe is the caller's to keep elsewhere)
    return check_probe_list(h, "hxv_lanczos_tridiag_probes", nprobes, d_probes, overlaps != nullptr, "the overlaps array", "the driver clears that place");
  };
  return tridiag_run(h, "hxv_lanczos_tridiag_probes", check_args(), d_vin, nprobes, d_probes, nlanc, alanc, blanc, overlaps, threshold, nsteps);
}

// Poles and weights of <p_j|(z - H)^{-1}|v> from one run of hxv_lanczos_tridiag_probes (include/hxv.h).  Host code only.
int hxv_gf_from_probes(int32_t nsteps, const double* alanc, const double* blanc, int32_t nprobes, const double* overlaps, double norm,
                       double* poles, double* weights) {
  if (nsteps < 1 || !alanc || !blanc || !poles || nprobes < 0 || (nprobes > 0 && (!overlaps || !weights)))
    return fail(HXV_ERR_ARG, "hxv_gf_from_probes: bad argument (nsteps < 1, nprobes < 0 or a NULL array)");
  const int m = nsteps;
  std::vector<double> d(alanc, alanc + m), e(blanc, blanc + m), z((size_t)m * m, 0.0);
  for (int i = 0; i < m; ++i) z[i + (size_t)i * m] = 1.0;
  if (!tridiag_ql(m, d, e, &z)) return fail(HXV_ERR_STATE, "hxv_gf_from_probes: tridiagonal QL did not converge");
  std::vector<int> order(m);
  for (int i = 0; i < m; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return d[a] < d[b] || (d[a] == d[b] && a < b); });  // poles ascending
  for (int o = 0; o < m; ++o) {
    const double* zn = &z[(size_t)order[o] * m];  // eigenvector of pole o: T = Z diag(poles) Z^T
    poles[o] = d[order[o]];
    for (int j = 0; j < nprobes; ++j) {
      double re = 0.0, im = 0.0;  // sum_k o_kj Z_kn
      for (int k = 0; k < m; ++k) {
        re += overlaps[2 * ((size_t)k * nprobes + j)] * zn[k];
        im += overlaps[2 * ((size_t)k * nprobes + j) + 1] * zn[k];
      }
      weights[2 * ((size_t)o * nprobes + j)] = norm * zn[0] * re;
      weights[2 * ((size_t)o * nprobes + j) + 1] = norm * zn[0] * im;
    }
  }
  return HXV_OK;
}

int hxv_lanczos_eigh(hxv_handle* h, int32_t nitermax, double threshold, double* egs, void* d_vect, int32_t* niter) {
  if (!h || nitermax < 1 || !egs) return fail(HXV_ERR_ARG, "hxv_lanczos_eigh: bad argument");
  HIPCHK(hipSetDevice(h->device));  // (before the first collective)
  const bool real = want_real(h);  // the start vector is ours: real when H is (REAL-vector mode)
  int rc = comm_agree(h, ensure_lz(h, real));
  if (rc) return rc;
  const int64_t n = lz_len(h, real);
  const int g = grid_for(n);
  const int nmax = (int)std::min<int64_t>(nitermax, h->host.dim);
  const uint64_t seed = 0x5EED5EEDull;
  LzRunner lz(h, h->lz_vec[0], h->lz_vec[1], h->lz_vec[2], real);
  rc = lz.begin_own(seed);
  if (rc) return rc;
  std::vector<double> al, be(1, 0.0), y;
  double e_old = 1e300, e_new = 0;
  int k = 0;
  for (; k < nmax; ++k) {
    double a, bt;
    rc = lz.step(&a, &bt);
    if (rc) return rc;
    al.push_back(a);
    if (!lowest_ritz(al, be, &e_new, nullptr)) return fail(HXV_ERR_STATE, "tridiagonal QL did not converge");
    bool conv = std::fabs(e_new - e_old) < threshold;
    e_old = e_new;
    if (conv && d_vect) {
      // the energy converges quadratically faster than the vector: before accepting, require the Ritz
      // residual estimate |beta_{k+1} * y_k| (last component of the tridiagonal eigenvector) to be small too
      double e_y;
      if (!lowest_ritz(al, be, &e_y, &y)) return fail(HXV_ERR_STATE, "tridiagonal QL did not converge");
      const double resid = std::fabs(bt * y.back());
      conv = resid < 1e-11 * std::max(1.0, std::fabs(e_new));
    }
    if (conv || std::fabs(bt) < 1e-14 || k + 1 == nmax) {
      ++k;
      break;
    }
    be.push_back(bt);
    rc = lz.advance();
    if (rc) return rc;
  }
  *egs = e_new;
  if (niter) *niter = k;
  if (d_vect) {
    // second pass: re-run the recurrence and accumulate the Ritz vector sum_j y_j q_j
    const int m = (int)al.size();
    double e_y;
    if (!lowest_ritz(al, be, &e_y, &y)) return fail(HXV_ERR_STATE, "tridiagonal QL did not converge");
    double2* out = (double2*)d_vect;
    LzRunner lz2(h, h->lz_vec[0], h->lz_vec[1], h->lz_vec[2], real);
    rc = lz2.begin_own(seed);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(out, 0, (size_t)n * sizeof(double2), h->stream));
    for (int j = 0; j < m; ++j) {
      hipLaunchKernelGGL(lz_axpy, dim3(g), dim3(256), 0, h->stream, n, out, lz2.vec(), y[j] * lz2.scale());
      if (j + 1 == m) break;
      double a, bt;
      rc = lz2.step(&a, &bt);
      if (rc) return rc;
      rc = lz2.advance();
      if (rc) return rc;
    }
    // normalise the Ritz vector
    rc = enqueue_normalise(h, out, out, n, LZ_BETA);
    if (rc) return rc;
    if (real) {
      // the Ritz vector was accumulated as a real vector in d_vect's memory: expand it to the complex layout of the API
      HIPCHK(hipMemcpyAsync(h->lz_vec[2], out, (size_t)n * sizeof(double2), hipMemcpyDeviceToDevice, h->stream));
      launch_to_complex(h, (const double*)h->lz_vec[2], out, h->stream);
    }
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return HXV_OK;
}

namespace {
// THE paired driver behind hxv_lanczos_tridiag_pair (nprobes = 0) and hxv_lanczos_tridiag_pair_probes.
// Two REAL Lanczos runs on one complex product (real H): the start vectors travel as real and imaginary part of one
// complex vector -- H(x + i y) = H x + i H y -- and every scalar of the recurrence exists once per component.  The channels of
// one Green's-function solve are independent (ED_GF_NORMAL.f90:123-306: one sp_lanc_tridiag per channel), so two of them share
// the product's passes.  The arithmetic of each component is, operation for operation, that of hxv_lanczos_tridiag on (x, 0)
// through the same kernels (options real_vectors = 0, job_up = 0): alanc/blanc are bit-identical to two such runs -- after the start-up
// below the recurrence is tridiag_run's own code, a two-component LzRunner in host_stepped_loop.
// With probes (real ones, shared by both components; converted once into pooled double[qdw][pitch] buffers) the overlaps of the STORED
// complex vector are taken before each step's product, as in tridiag_run, by lz_probe_dots_pair: overlaps_x as hxv_lanczos_tridiag_probes
// lays them out, imaginary parts zero.  rc_args: what the entry decided from its own arguments; it goes into the agreement in front of the
// first collective.  The imaginary parts of the start vectors AND of the probes are checked in ONE reduction, whose sum every rank sees.
int tridiag_pair_run(hxv_handle* h, const char* who, int rc_args, const void* d_vin_a, const void* d_vin_b, int nprobes,
                     const void* const* d_probes, int nlanc, double* alanc_a, double* blanc_a, double* overlaps_a, double* alanc_b,
                     double* blanc_b, double* overlaps_b, double threshold, int32_t* nsteps_a, int32_t* nsteps_b) {
  if (const char* why = real_mode_blocker(h)) return fail(HXV_ERR_UNSUPPORTED, std::string(who) + ": unavailable: " + why);
  if (int rcc = need_comm(h, "device Lanczos")) return rcc;
  if (!h->lz_fused) return fail(HXV_ERR_UNSUPPORTED, std::string(who) + " needs the fused recurrence (option lanczos_fused)");
  HIPCHK(hipSetDevice(h->device));
  CallScope pooled(h);  // (the scalar blocks; staged start vectors; with probes their real copies and the scratch of the check and the overlaps)
  const int64_t n = lz_len(h, false);
  const int g = grid_for(n);
  // scalars: the LzSlot block of component a, the one of b LZ_PAIR behind it (the handle's d_scalars has room for one only); the block
  // partials of the start vectors' check behind them
  double* d_sc_mem = nullptr;
  // scratch of a run WITH probes (ProbeScratch): the partials of Im^2 are the start vectors' row, then one row of RED_BLOCKS per probe, g of each
  // used, side by side for the one reduction
  ProbeScratch ws;
  LzProbeSet pb;
  pb.m = std::max(nprobes, 0);
  pb.pair = true;
  // every rank-local preparation that can fail comes BEFORE the agreement: a rank that cannot go on makes all ranks return
  auto prepare = [&]() -> int {
    if (rc_args) return rc_args;
    int r = stage_start_vector(h, d_vin_a, pooled);  // (start vectors at hxv_slab_home: staged before their home is cleared)
    if (!r) r = stage_start_vector(h, d_vin_b, pooled);
    if (!r) r = ensure_lz(h, false);  // (split sector: vectors are this rank's slab, every sum below is all-reduced)
    if (!r) r = ensure_wt(h);
    if (!r) r = ensure_lz_partial(h, 2 * lz_pass_a_workgroups(h, false));
    if (r) return r;
    HIPCHK(pooled.take_device((size_t)(2 * LZ_PAIR + 3 * RED_BLOCKS) * sizeof(double), &d_sc_mem));
    if (nprobes == 0) return HXV_OK;
    r = ws.take(h, pooled, (size_t)(1 + nprobes) * RED_BLOCKS, (size_t)2 * nprobes * RED_BLOCKS, (size_t)2 * nprobes, (int64_t)2 * nprobes * nlanc);
    for (int j = 0; j < nprobes && !r; ++j) HIPCHK(pooled.take((size_t)std::max<int64_t>(n, 1) * sizeof(double), &pb.rp.p[j]));
    return r;
  };
  int rc = comm_agree(h, prepare());
  if (rc) return rc;
  double* const d_sc = d_sc_mem;
  double* d_p0 = nprobes ? ws.chk : d_sc + 2 * LZ_PAIR;  // (Im^2 of the start vectors; the probes' rows follow it at a distance of g)
  double* d_p1 = d_sc + 2 * LZ_PAIR + RED_BLOCKS;
  double* d_p2 = d_p1 + RED_BLOCKS;
  pb.part = ws.part;
  pb.sums = ws.sums;
  HIPCHK(hipMemsetAsync(d_sc, 0, 2 * LZ_PAIR * sizeof(double), h->stream));
  hipLaunchKernelGGL(lz_pack_pair, dim3(g), dim3(256), 0, h->stream, n, (const double2*)d_vin_a, (const double2*)d_vin_b, h->lz_vec[0], d_p0, d_p1, d_p2);
  for (int j = 0; j < nprobes; ++j)
    hipLaunchKernelGGL(lz_probe_real_pc, dim3(g), dim3(256), 0, h->stream, n, h->host.dimup, h->host.pitch, (const double2*)d_probes[j],
                       const_cast<double*>(pb.rp.p[j]), d_p0 + (size_t)(1 + j) * g);
  // (its own block: the three sums of the check sit in a row from LZ_TMP on)
  if ((rc = reduce_scalar(h, d_p0, (1 + nprobes) * g, LZ_TMP, 0, d_sc)) || (rc = reduce_scalar(h, d_p1, g, LZ_TMP + 1, 1, d_sc)) || (rc = reduce_scalar(h, d_p2, g, LZ_TMP + 2, 1, d_sc))) return rc;
  double head[3];
  HIPCHK(hipMemcpyAsync(head, d_sc + LZ_TMP, 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  // (head[0] is the sum over all ranks: every rank returns here together)
  if (head[0] != 0.0)
    return fail(HXV_ERR_ARG, std::string(who) + (nprobes ? ": the start vectors and the probes must be real (zero imaginary parts)" : ": the start vectors must be real (zero imaginary parts)"));
  for (int c = 0; c < 2; ++c)
    if (!(head[1 + c] > 0.0) || !std::isfinite(head[1 + c])) return fail(HXV_ERR_ARG, std::string(who) + ": a start vector is zero or not finite");
  LzOut out[2] = {{alanc_a, blanc_a, overlaps_a}, {alanc_b, blanc_b, overlaps_b}};
  for (const LzOut& o : out) o.clear(nlanc, nprobes);
  // the two-component runner on the packed vector: q = s*X per component, s = 1/beta_k (each start vector's norm carried as its beta_0)
  LzRunner lz(h, h->lz_vec[0], h->lz_vec[1], h->lz_vec[2], false, d_sc);
  if ((rc = lz.begin(start_norm(head[1]), start_norm(head[2]))) || (rc = host_stepped_loop(h, lz, pb, nlanc, threshold, out))) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (nsteps_a) *nsteps_a = out[0].nsteps;
  if (nsteps_b) *nsteps_b = out[1].nsteps;
  return HXV_OK;
}
}  // namespace

int hxv_lanczos_tridiag_pair(hxv_handle* h, const void* d_vin_a, const void* d_vin_b, int32_t nlanc, double* alanc_a, double* blanc_a,
                             double* alanc_b, double* blanc_b, double threshold, int32_t* nsteps_a, int32_t* nsteps_b) {
  if (!h || !d_vin_a || !d_vin_b || nlanc < 1 || !alanc_a || !blanc_a || !alanc_b || !blanc_b)
    return fail(HXV_ERR_ARG, "hxv_lanczos_tridiag_pair: bad argument");
  return tridiag_pair_run(h, "hxv_lanczos_tridiag_pair", HXV_OK, d_vin_a, d_vin_b, 0, nullptr, nlanc, alanc_a, blanc_a, nullptr, alanc_b, blanc_b,
                          nullptr, threshold, nsteps_a, nsteps_b);
}

// Two probe runs on one product (include/hxv.h): hxv_lanczos_tridiag_pair with the overlaps of hxv_lanczos_tridiag_probes for each component.
int hxv_lanczos_tridiag_pair_probes(hxv_handle* h, const void* d_vin_a, const void* d_vin_b, int32_t nprobes, const void* const* d_probes,
                                    int32_t nlanc, double* alanc_a, double* blanc_a, double* overlaps_a, double* alanc_b, double* blanc_b,
                                    double* overlaps_b, double threshold, int32_t* nsteps_a, int32_t* nsteps_b) {
  if (!h) return fail(HXV_ERR_ARG, "hxv_lanczos_tridiag_pair_probes: NULL handle");
  auto check_args = [&]() -> int {
    if (!d_vin_a || !d_vin_b || nlanc < 1 || !alanc_a || !blanc_a || !alanc_b || !blanc_b)
      return fail(HXV_ERR_ARG, "hxv_lanczos_tridiag_pair_probes: bad argument (NULL start vector or output, or nlanc < 1)");
    return check_probe_list(h, "hxv_lanczos_tridiag_pair_probes", nprobes, d_probes, overlaps_a && overlaps_b, "both overlaps arrays", "the driver clears that place");
  };
  return tridiag_pair_run(h, "hxv_lanczos_tridiag_pair_probes", check_args(), d_vin_a, d_vin_b, nprobes, d_probes, nlanc, alanc_a, blanc_a,
                          overlaps_a, alanc_b, blanc_b, overlaps_b, threshold, nsteps_a, nsteps_b);
}

namespace {
int ensure_stage(hxv_handle* h) {
  const size_t bytes = (size_t)h->host.pitch * std::max(h->host.qdw, 1) * sizeof(double2);
  if (!h->d_stage_v) {
    HIPCHK(pool_alloc(h->device, bytes, (void**)&h->d_stage_v));
    HIPCHK(pool_alloc(h->device, bytes, (void**)&h->d_stage_hv));
    HIPCHK(hipMemsetAsync(h->d_stage_v, 0, bytes, h->stream));  // (on the handle's stream: it does not synchronise with the null stream)
    HIPCHK(hipMemsetAsync(h->d_stage_hv, 0, bytes, h->stream));
    h->device_bytes += 2 * (int64_t)bytes;
  }
  return HXV_OK;
}
}  // namespace

int hxv_lanczos_tridiag_host(hxv_handle* h, const void* vin_host, int32_t nlanc, double* alanc, double* blanc, double threshold,
                             int32_t* nsteps) {
  if (!h || !vin_host) return fail(HXV_ERR_ARG, "hxv_lanczos_tridiag_host: NULL argument");
  HIPCHK(hipSetDevice(h->device));
  int rc = ensure_stage(h);
  if (rc) return rc;
  rc = slab_from_host(h, vin_host, h->d_stage_v);
  if (rc) return rc;
  return hxv_lanczos_tridiag(h, h->d_stage_v, nlanc, alanc, blanc, threshold, nsteps);
}

int hxv_lanczos_tridiag_pair_host(hxv_handle* h, const void* vin_a_host, const void* vin_b_host, int32_t nlanc, double* alanc_a,
                                  double* blanc_a, double* alanc_b, double* blanc_b, double threshold, int32_t* nsteps_a, int32_t* nsteps_b) {
  if (!h || !vin_a_host || !vin_b_host) return fail(HXV_ERR_ARG, "hxv_lanczos_tridiag_pair_host: NULL argument");
  HIPCHK(hipSetDevice(h->device));
  int rc = ensure_stage(h);
  if (rc) return rc;
  rc = slab_from_host(h, vin_a_host, h->d_stage_v);
  if (rc) return rc;
  rc = slab_from_host(h, vin_b_host, h->d_stage_hv);
  if (rc) return rc;
  return hxv_lanczos_tridiag_pair(h, h->d_stage_v, h->d_stage_hv, nlanc, alanc_a, blanc_a, alanc_b, blanc_b, threshold, nsteps_a, nsteps_b);
}

int hxv_lanczos_eigh_host(hxv_handle* h, int32_t nitermax, double threshold, double* egs, void* vect_host, int32_t* niter) {
  if (!h) return fail(HXV_ERR_ARG, "hxv_lanczos_eigh_host: NULL handle");
  HIPCHK(hipSetDevice(h->device));
  int rc = ensure_stage(h);
  if (rc) return rc;
  rc = hxv_lanczos_eigh(h, nitermax, threshold, egs, vect_host ? h->d_stage_hv : nullptr, niter);
  if (rc) return rc;
  if (vect_host) return slab_to_host(h, h->d_stage_hv, vect_host);
  return HXV_OK;
}

int hxv_time_lanczos(hxv_handle* h, void* d_work3, int32_t nrep, float* ms_per_iter) {
  if (!h || !d_work3 || nrep < 1 || !ms_per_iter) return fail(HXV_ERR_ARG, "hxv_time_lanczos: bad argument");
  if (h->host.nranks != 1) return fail(HXV_ERR_STATE, "hxv_time_lanczos needs nranks==1");
  HIPCHK(hipSetDevice(h->device));
  int64_t n = (int64_t)h->host.pitch * h->host.dimdw;
  HIPCHK(hipMemsetAsync(d_work3, 0, (size_t)3 * n * sizeof(double2), h->stream));
  const bool real = want_real(h);
  LzRunner lz(h, (double2*)d_work3, (double2*)d_work3 + n, (double2*)d_work3 + 2 * n, real);
  n = lz.n2;
  int rc = lz.begin_own(0x1234ull);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(lz.b.qm, 0, (size_t)n * sizeof(double2), h->stream));
  double a, bt;
  rc = lz.step(&a, &bt);  // untimed first step (lazy allocations)
  if (rc) return rc;
  if (lz.device_only_ok(nrep)) {
    // the fixed-length device-only path of hxv_lanczos_tridiag: iterations 1..nrep, three per hipGraph
    hipEvent_t ev[2] = {h->ev0, h->ev1};
    rc = lz.run_device_only(bt, nrep + 1, nullptr, ev, "hxv_time_lanczos");
    if (rc) return rc;
    float msg = 0;
    HIPCHK(hipEventElapsedTime(&msg, h->ev0, h->ev1));
    *ms_per_iter = msg / (float)nrep;
    return HXV_OK;
  }
  rc = lz.advance();
  if (rc) return rc;
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  for (int k = 0; k < nrep; ++k) {
    rc = lz.step(&a, &bt);
    if (rc) return rc;
    rc = lz.advance();
    if (rc) return rc;
  }
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  HIPCHK(hipEventSynchronize(h->ev1));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  *ms_per_iter = ms / (float)nrep;
  return HXV_OK;
}

}  // extern "C"
