// Chebyshev recurrence on device behind the C-ABI (include/hxv.h): hxv_chebyshev_moments (the moments <p_j|T_n(Ht)|v> and the doubled
// self-moments <v|T_k(Ht)|v>) and hxv_chebyshev_apply (sum_n coef_n T_n(Ht) v), Ht = (H - b)/a, and their REAL-vector forms
// hxv_chebyshev_moments_real / hxv_chebyshev_apply_real for a real H with real vectors.  ONE driver runs all four: per order one product
// through apply_slab / apply_slab_real (no epilogue: the product kernels are the engine's, untouched) and one fused streaming pass
// (hxv_chebyshev_kernels.hpp, hxv_chebyshev_real_kernels.hpp), whose 2*nprobes + 3 (real: nprobes + 2) sums go through ONE all-reduce on a
// split sector and reach the host with ONE stream synchronisation per order, where the window guard reads them.
// The four entries check their arguments through two helpers (check_moments, check_apply); the probe list's check and the carving of the
// small scratch block are the Lanczos drivers' (check_probe_list, ProbeScratch).
// Also here: hxv_vector_random, the seeded random device state the typical-state uses of the recurrence start from.
#include <cmath>
#include <cstring>

#include "hxv_call_scope.hpp"
#include "hxv_chebyshev_real_kernels.hpp"  // (and through it hxv_chebyshev_kernels.hpp)

using namespace hxv;

namespace {

// THE recurrence, on complex vectors or -- `real` -- on real ones.  norder orders t_0 .. t_{norder-1}, norder - 1 products.  coef/d_out: the
// running sum of hxv_chebyshev_apply[_real] (null: none; coef complex, interleaved, or `real`: real); moments/self_moments: what
// hxv_chebyshev_moments[_real] returns (either may be null; moments complex or `real`: real).  rc_args: what the entry decided from its own
// arguments; it goes INTO the first agreement of a split sector, and nothing here looks at an argument before that.
// Scratch, through the call's scope: three vector-sized blocks (H t_n and the two vectors of the recurrence; d_vin is copied into one of them
// before the first exchange, which is what stages a start vector at hxv_slab_home) and one small block for the partial sums.
// `real`: every block is a real one, double[qdw][pitch_real] viewed as double2 (half the bytes), and there are 1 + nprobes more of them: the
// real copies of the probes and the running sum.  d_vin and the probes arrive in the complex layout and are converted once (ch_to_real), with
// the sum of |Im| over all of them and all ranks in ONE reduction: any imaginary part is refused, on every rank alike.  The running sum goes
// back to the complex layout once, after the last order, so d_out is written only when the whole recurrence went through.
int chebyshev_run(hxv_handle* h, const char* who, bool real, int rc_args, const void* d_vin, int nprobes, const void* const* d_probes, int norder,
                  double a, double b, const double* coef, double2* d_out, double* moments, double* self_moments, double* norm2) {
  HIPCHK(hipSetDevice(h->device));  // (before the first collective: thread ranks on several GPUs each have their own current device)
  CallScope pooled(h);
  const int pitr = pitch_real_of(h);
  const int64_t n = real ? (int64_t)pitr * h->host.qdw / 2 : (int64_t)h->host.pitch * h->host.qdw;  // this rank's slab, in double2 elements
  const size_t bytes = real ? (size_t)pitr * std::max(h->host.qdw, 1) * sizeof(double) : (size_t)h->host.pitch * std::max(h->host.qdw, 1) * sizeof(double2);
  const int np = std::max(nprobes, 0);
  const int g = grid_for(n), nc = real ? ch_sums_real(np) : ch_sums(np);
  const int g_chk = real ? grid_for((int64_t)pitr * h->host.qdw) : 0;  // (workgroups of one conversion = its partial sums of |Im|)
  ProbeScratch ws;  // (partials of an order's sums, the sums, and the partials of the conversions' |Im|; an order's sums staged in the handle's array)
  double2 *d_hv = nullptr, *d_a = nullptr, *d_b = nullptr, *d_sum = nullptr;
  double* real_probe[HXV_MAX_PROBES] = {};
  auto resources = [&]() -> int {
    if (rc_args) return rc_args;
    if (int rcc = need_comm(h, who)) return rcc;
    if (int rcw = ws.take(h, pooled, (size_t)(1 + np) * g_chk, (size_t)g * nc, (size_t)nc, nc)) return rcw;
    HIPCHK(pooled.take(bytes, &d_hv));
    HIPCHK(pooled.take(bytes, &d_a));
    HIPCHK(pooled.take(bytes, &d_b));
    for (int j = 0; real && j < np; ++j) HIPCHK(pooled.take(bytes, &real_probe[j]));
    if (real && d_out) HIPCHK(pooled.take(bytes, &d_sum));
    return HXV_OK;
  };
  if (int rca = comm_agree(h, resources())) return rca;  // (a rank with bad arguments or without memory tells its peers before the first all-reduce)
  double *d_part = ws.part, *d_sums = ws.sums, *d_chk = ws.chk, *stage = h->h_probe_ov;
  if (!real) d_sum = d_out;
  LzProbes pr{};
  for (int j = 0; j < nprobes; ++j) pr.p[j] = real ? (const double2*)real_probe[j] : (const double2*)d_probes[j];
  // the product never writes pad rows: H t_n's are zeroed once.  t_0 = v goes into the recurrence's own buffer, so d_vin is only ever read.
  HIPCHK(hipMemsetAsync(d_hv, 0, bytes, h->stream));
  if (real) {
    for (int j = 0; j <= nprobes; ++j)
      hipLaunchKernelGGL(ch_to_real, dim3(g_chk), dim3(256), 0, h->stream, h->host.dimup, h->host.qdw, h->host.pitch, pitr,
                         (const double2*)(j ? d_probes[j - 1] : d_vin), j ? real_probe[j - 1] : (double*)d_b, d_chk + (size_t)j * g_chk);
    hipLaunchKernelGGL(lz_probe_final, dim3(1), dim3(256), 0, h->stream, d_chk, (1 + nprobes) * g_chk, 1, d_sums);
    if (int rci = comm_allreduce_sum(h, d_sums, 1, h->stream)) return rci;
    HIPCHK(hipMemcpyAsync(stage, d_sums, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!(stage[0] == 0.0))  // (the all-reduced sum: every rank decides alike)
      return fail(HXV_ERR_ARG, std::string(who) + ": the start vector or a probe has a non-zero (or non-finite) imaginary part: the real form takes purely real vectors");
  } else {
    HIPCHK(hipMemcpyAsync(d_b, d_vin, (size_t)n * sizeof(double2), hipMemcpyDeviceToDevice, h->stream));
  }
  // all sums of an order: this rank's share -> ONE all-reduce -> the host, with the order's one synchronisation
  auto read_sums = [&]() -> int {
    int rc = comm_allreduce_sum(h, d_sums, (size_t)nc, h->stream);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(stage, d_sums, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return HXV_OK;
  };
  auto all_finite = [&]() {
    bool finite = true;
    for (int j = 0; j < nc; ++j) finite = finite && std::isfinite(stage[j]);
    return finite;
  };
  const int nmo = real ? nprobes : 2 * nprobes;  // doubles of one order's moments; behind them <t|t>, then (Re) <t|t_cur>
  auto record = [&](int order) {
    if (moments)
      for (int j = 0; j < nmo; ++j) moments[(size_t)nmo * order + j] = stage[j];
  };
  auto cre = [&](int k) { return coef ? coef[real ? k : 2 * k] : 0.0; };
  auto cim = [&](int k) { return coef ? coef[2 * k + 1] : 0.0; };
  if (real)
    launch_ch_init_real(g, h->stream, nprobes, n, d_b, d_sum, pr, cre(0), d_part, d_sums);
  else
    launch_ch_init(g, h->stream, nprobes, n, d_b, d_sum, pr, cre(0), cim(0), d_part, d_sums);
  int rc = read_sums();
  if (rc) return rc;
  const double mu0 = stage[nmo];
  if (!(mu0 > 0.0) || !std::isfinite(mu0)) return fail(HXV_ERR_ARG, std::string(who) + ": the start vector is zero or not finite");
  if (!all_finite()) return fail(HXV_ERR_ARG, std::string(who) + ": an overlap of a probe with the start vector is not finite (a probe that is not finite)");
  record(0);
  if (self_moments) self_moments[0] = mu0;
  double mu1 = 0.0;
  double2 *cur = d_b, *prev = d_a;  // (order 1 has no t_prev: its form writes t_1 into `prev` without reading it)
  for (int k = 1; k < norder; ++k) {
    rc = real ? apply_slab_real(h, (const double*)cur, (double*)d_hv, h->stream) : apply_slab(h, cur, d_hv, h->stream);
    if (rc) return rc;
    const bool first = k == 1;
    const double ch = (first ? 1.0 : 2.0) / a, cc = (first ? 1.0 : 2.0) * b / a;
    if (real)
      launch_ch_step_real(g, h->stream, nprobes, first, n, d_hv, cur, prev, d_sum, pr, ch, cc, cre(k), d_part, d_sums);
    else
      launch_ch_step(g, h->stream, nprobes, first, n, d_hv, cur, prev, d_sum, pr, ch, cc, cre(k), cim(k), d_part, d_sums);
    rc = read_sums();
    if (rc) return rc;
    // THE WINDOW GUARD: |t_k| <= |v| for a spectrum inside [b - a, b + a].  The sums are the all-reduced ones, the same on every rank, so all
    // ranks leave together.  4 is a guard, not a tolerance: a window that is too narrow grows geometrically and passes it within a few steps.
    const double tt = stage[nmo], tc = stage[nmo + 1];
    if (!all_finite() || tt > 4.0 * mu0)
      return fail(HXV_ERR_ARG, std::string(who) + ": spectrum outside the window [b - a, b + a] (order " + std::to_string(k) + ": <t|t> = " +
                                   std::to_string(tt) + ", <v|v> = " + std::to_string(mu0) + ")");
    record(k);
    if (first) mu1 = tc;
    if (self_moments) {  // mu_{2k-1} = 2 Re<t_k|t_{k-1}> - mu_1,  mu_{2k} = 2 <t_k|t_k> - mu_0
      self_moments[2 * k - 1] = first ? mu1 : 2.0 * tc - mu1;
      self_moments[2 * k] = 2.0 * tt - mu0;
    }
    std::swap(cur, prev);  // t_k was stored over t_{k-2}
  }
  if (d_out) {
    rc = enqueue_norm(h, d_sum, n, LZ_TMP, 0);  // (a real vector viewed as double2: the same sum of squares)
    if (rc) return rc;
    double nrm2 = 0.0;
    HIPCHK(hipMemcpyAsync(&nrm2, h->d_scalars + LZ_TMP, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (real) launch_to_complex(h, (const double*)d_sum, d_out, h->stream);  // (the imaginary part, and every pad, +0.0)
    HIPCHK(hipStreamSynchronize(h->stream));
    if (norm2) *norm2 = nrm2;
  }
  return HXV_OK;
}

// The argument checks of the two moments entries and of the two apply entries (who: the entry's name; real: the REAL-vector form, asked for by
// name, so option "real_vectors" is not consulted: what makes real vectors impossible on this handle is an HXV_ERR_UNSUPPORTED with the
// blocker's text).
int check_window(const std::string& who, double a, double b) {
  if (std::isfinite(a) && std::isfinite(b) && a > 0.0) return HXV_OK;
  return fail(HXV_ERR_ARG, who + ": the window needs a > 0 and finite a, b");
}
int check_real(const hxv_handle* h, const std::string& who, bool real) {
  const char* why = real ? real_mode_blocker(h) : nullptr;
  return why ? fail(HXV_ERR_UNSUPPORTED, who + ": real vectors unavailable: " + why) : HXV_OK;
}
int check_moments(const hxv_handle* h, const char* who, bool real, const void* d_vin, int nprobes, const void* const* d_probes, int nmom, double a,
                  double b, const double* moments) {
  if (int rc = check_real(h, who, real)) return rc;
  if (!d_vin || nmom < 1) return fail(HXV_ERR_ARG, std::string(who) + ": bad argument (NULL start vector or nmom < 1)");
  if (int rc = check_window(who, a, b)) return rc;
  // (the exchange of a product writes this rank's slab into its place in a gather buffer)
  return check_probe_list(h, who, nprobes, d_probes, moments != nullptr, "the moments array", "the exchange overwrites that place");
}
int check_apply(const hxv_handle* h, const char* who, bool real, const void* d_vin, int ncoef, const double* coef, double a, double b, const void* d_out) {
  const std::string w = who;
  if (int rc = check_real(h, w, real)) return rc;
  if (!d_vin || !d_out || !coef || ncoef < 1) return fail(HXV_ERR_ARG, w + ": bad argument (NULL vector or coefficients, or ncoef < 1)");
  if (d_out == d_vin) return fail(HXV_ERR_ARG, w + ": d_out must not be d_vin");
  if (int rc = check_window(w, a, b)) return rc;
  for (int k = 0; k < (real ? ncoef : 2 * ncoef); ++k)  // (complex coefficients are interleaved)
    if (!std::isfinite(coef[k])) return fail(HXV_ERR_ARG, w + ": a coefficient is not finite");
  if (comm_ready(h) && comm_in_gather(h, d_out)) return fail(HXV_ERR_ARG, w + ": d_out lies in a gather buffer of the handle (hxv_slab_home): the exchange overwrites that place");
  return HXV_OK;
}

}  // namespace

extern "C" {

int hxv_chebyshev_moments(hxv_handle* h, const void* d_vin, int32_t nprobes, const void* const* d_probes, int32_t nmom, double a, double b,
                          double* moments, double* self_moments) {
  const char* who = "hxv_chebyshev_moments";
  if (!h) return fail(HXV_ERR_ARG, std::string(who) + ": NULL handle");
  const int rc_args = check_moments(h, who, false, d_vin, nprobes, d_probes, nmom, a, b, moments);
  return chebyshev_run(h, who, false, rc_args, d_vin, nprobes, d_probes, nmom, a, b, nullptr, nullptr, moments, self_moments, nullptr);
}

int hxv_chebyshev_apply(hxv_handle* h, const void* d_vin, int32_t ncoef, const double* coef, double a, double b, void* d_out, double* norm2) {
  const char* who = "hxv_chebyshev_apply";
  if (!h) return fail(HXV_ERR_ARG, std::string(who) + ": NULL handle");
  const int rc_args = check_apply(h, who, false, d_vin, ncoef, coef, a, b, d_out);
  return chebyshev_run(h, who, false, rc_args, d_vin, 0, nullptr, ncoef, a, b, coef, (double2*)d_out, nullptr, nullptr, norm2);
}

// REAL-vector forms (include/hxv.h): the same checks, then the one driver with `real`.
int hxv_chebyshev_moments_real(hxv_handle* h, const void* d_vin, int32_t nprobes, const void* const* d_probes, int32_t nmom, double a, double b,
                               double* moments, double* self_moments) {
  const char* who = "hxv_chebyshev_moments_real";
  if (!h) return fail(HXV_ERR_ARG, std::string(who) + ": NULL handle");
  const int rc_args = check_moments(h, who, true, d_vin, nprobes, d_probes, nmom, a, b, moments);
  return chebyshev_run(h, who, true, rc_args, d_vin, nprobes, d_probes, nmom, a, b, nullptr, nullptr, moments, self_moments, nullptr);
}

int hxv_chebyshev_apply_real(hxv_handle* h, const void* d_vin, int32_t ncoef, const double* coef, double a, double b, void* d_out, double* norm2) {
  const char* who = "hxv_chebyshev_apply_real";
  if (!h) return fail(HXV_ERR_ARG, std::string(who) + ": NULL handle");
  const int rc_args = check_apply(h, who, true, d_vin, ncoef, coef, a, b, d_out);
  return chebyshev_run(h, who, true, rc_args, d_vin, 0, nullptr, ncoef, a, b, coef, (double2*)d_out, nullptr, nullptr, norm2);
}

// The seeded random state (include/hxv.h): one streaming kernel over this rank's slab, local, on any handle.
int hxv_vector_random(hxv_handle* h, uint64_t seed, int32_t complex_valued, void* d_vec) {
  if (!h || !d_vec) return fail(HXV_ERR_ARG, "hxv_vector_random: NULL handle or vector");
  if (complex_valued != 0 && complex_valued != 1) return fail(HXV_ERR_ARG, "hxv_vector_random: complex_valued must be 0 or 1");
  HIPCHK(hipSetDevice(h->device));
  const int64_t n = (int64_t)h->host.pitch * h->host.qdw;
  hipLaunchKernelGGL(vec_random, dim3(grid_for(n)), dim3(256), 0, h->stream, n, (double2*)d_vec, vr_mix(seed), (int)complex_valued, h->host.dimup,
                     h->host.pitch, h->host.dw0, h->dev.up_iperm, h->dev.up_sign);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return HXV_OK;
}

}  // extern "C"
