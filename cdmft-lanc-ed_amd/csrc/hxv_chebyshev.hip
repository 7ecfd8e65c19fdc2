// Chebyshev recurrence on device behind the C-ABI (include/hxv.h): hxv_chebyshev_moments (the moments <p_j|T_n(Ht)|v> and the doubled
// self-moments <v|T_k(Ht)|v>) and hxv_chebyshev_apply (sum_n coef_n T_n(Ht) v), Ht = (H - b)/a.  ONE driver runs both: per order one product
// through apply_slab (no epilogue: the product kernels are the engine's, untouched) and one fused streaming pass (hxv_chebyshev_kernels.hpp),
// whose 2*nprobes + 3 sums go through ONE all-reduce on a split sector and reach the host with ONE stream synchronisation per order, where
// the window guard reads them.  Complex vectors only.
#include <cmath>
#include <cstring>

#include "hxv_call_scope.hpp"
#include "hxv_chebyshev_kernels.hpp"

using namespace hxv;

namespace {

// THE recurrence.  norder orders t_0 .. t_{norder-1}, norder - 1 products.  coef/d_out: the running sum of hxv_chebyshev_apply (null: none);
// moments/self_moments: what hxv_chebyshev_moments returns (either may be null).  rc_args: what the entry decided from its own arguments; it
// goes INTO the first agreement of a split sector, and nothing here looks at an argument before that.
// Scratch, through the call's scope: three vector-sized blocks (H t_n and the two vectors of the recurrence; d_vin is copied into one of them
// before the first exchange, which is what stages a start vector at hxv_slab_home) and one small block for the partial sums.
int chebyshev_run(hxv_handle* h, const char* who, int rc_args, const void* d_vin, int nprobes, const void* const* d_probes, int norder, double a,
                  double b, const double* coef, double2* d_out, double* moments, double* self_moments, double* norm2) {
  HIPCHK(hipSetDevice(h->device));  // (before the first collective: thread ranks on several GPUs each have their own current device)
  CallScope pooled(h);
  const int64_t n = (int64_t)h->host.pitch * h->host.qdw;  // this rank's slab
  const size_t bytes = (size_t)h->host.pitch * std::max(h->host.qdw, 1) * sizeof(double2);
  const int g = grid_for(n), nc = ch_sums(std::max(nprobes, 0));
  double* d_ws = nullptr;
  double2 *d_hv = nullptr, *d_a = nullptr, *d_b = nullptr;
  auto resources = [&]() -> int {
    if (rc_args) return rc_args;
    if (int rcc = need_comm(h, who)) return rcc;
    HIPCHK(pooled.take((size_t)(g + 1) * nc * sizeof(double), &d_ws));
    HIPCHK(pooled.take(bytes, &d_hv));
    HIPCHK(pooled.take(bytes, &d_a));
    HIPCHK(pooled.take(bytes, &d_b));
    return ensure_probe_stage(h, nc);  // (page-locked staging for an order's sums: the handle's own array)
  };
  if (int rca = comm_agree(h, resources())) return rca;  // (a rank with bad arguments or without memory tells its peers before the first all-reduce)
  double *d_part = d_ws, *d_sums = d_ws + (size_t)g * nc, *stage = h->h_probe_ov;
  LzProbes pr{};
  for (int j = 0; j < nprobes; ++j) pr.p[j] = (const double2*)d_probes[j];
  // the product never writes pad rows: H t_n's are zeroed once.  t_0 = v goes into the recurrence's own buffer, so d_vin is only ever read.
  HIPCHK(hipMemsetAsync(d_hv, 0, bytes, h->stream));
  HIPCHK(hipMemcpyAsync(d_b, d_vin, (size_t)n * sizeof(double2), hipMemcpyDeviceToDevice, h->stream));
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
  auto record = [&](int order) {
    if (moments)
      for (int j = 0; j < 2 * nprobes; ++j) moments[(size_t)2 * nprobes * order + j] = stage[j];
  };
  launch_ch_init(g, h->stream, nprobes, n, d_b, d_out, pr, coef ? coef[0] : 0.0, coef ? coef[1] : 0.0, d_part, d_sums);
  int rc = read_sums();
  if (rc) return rc;
  const double mu0 = stage[2 * nprobes];
  if (!(mu0 > 0.0) || !std::isfinite(mu0)) return fail(HXV_ERR_ARG, std::string(who) + ": the start vector is zero or not finite");
  if (!all_finite()) return fail(HXV_ERR_ARG, std::string(who) + ": an overlap of a probe with the start vector is not finite (a probe that is not finite)");
  record(0);
  if (self_moments) self_moments[0] = mu0;
  double mu1 = 0.0;
  double2 *cur = d_b, *prev = d_a;  // (order 1 has no t_prev: its form writes t_1 into `prev` without reading it)
  for (int k = 1; k < norder; ++k) {
    rc = apply_slab(h, cur, d_hv, h->stream);
    if (rc) return rc;
    const bool first = k == 1;
    launch_ch_step(g, h->stream, nprobes, first, n, d_hv, cur, prev, d_out, pr, (first ? 1.0 : 2.0) / a, (first ? 1.0 : 2.0) * b / a,
                   coef ? coef[2 * k] : 0.0, coef ? coef[2 * k + 1] : 0.0, d_part, d_sums);
    rc = read_sums();
    if (rc) return rc;
    // THE WINDOW GUARD: |t_k| <= |v| for a spectrum inside [b - a, b + a].  The sums are the all-reduced ones, the same on every rank, so all
    // ranks leave together.  4 is a guard, not a tolerance: a window that is too narrow grows geometrically and passes it within a few steps.
    const double tt = stage[2 * nprobes], tc = stage[2 * nprobes + 1];
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
    rc = enqueue_norm(h, d_out, n, LZ_TMP, 0);
    if (rc) return rc;
    double nrm2 = 0.0;
    HIPCHK(hipMemcpyAsync(&nrm2, h->d_scalars + LZ_TMP, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (norm2) *norm2 = nrm2;
  }
  return HXV_OK;
}

bool window_ok(double a, double b) { return std::isfinite(a) && std::isfinite(b) && a > 0.0; }

}  // namespace

extern "C" {

int hxv_chebyshev_moments(hxv_handle* h, const void* d_vin, int32_t nprobes, const void* const* d_probes, int32_t nmom, double a, double b,
                          double* moments, double* self_moments) {
  if (!h) return fail(HXV_ERR_ARG, "hxv_chebyshev_moments: NULL handle");
  auto check_args = [&]() -> int {
    if (!d_vin || nmom < 1) return fail(HXV_ERR_ARG, "hxv_chebyshev_moments: bad argument (NULL start vector or nmom < 1)");
    if (!window_ok(a, b)) return fail(HXV_ERR_ARG, "hxv_chebyshev_moments: the window needs a > 0 and finite a, b");
    if (nprobes < 0 || nprobes > HXV_MAX_PROBES) return fail(HXV_ERR_ARG, "hxv_chebyshev_moments: nprobes must be 0 .. HXV_MAX_PROBES (8)");
    if (nprobes > 0 && (!d_probes || !moments)) return fail(HXV_ERR_ARG, "hxv_chebyshev_moments: nprobes > 0 needs the probe list and the moments array");
    for (int j = 0; j < nprobes; ++j) {
      if (!d_probes[j]) return fail(HXV_ERR_ARG, "hxv_chebyshev_moments: NULL entry in the probe list");
      // (the exchange of a product writes this rank's slab into its place in a gather buffer)
      if (comm_ready(h) && comm_in_gather(h, d_probes[j])) return fail(HXV_ERR_ARG, "hxv_chebyshev_moments: a probe lies in a gather buffer of the handle (hxv_slab_home): the exchange overwrites that place");
    }
    return HXV_OK;
  };
  return chebyshev_run(h, "hxv_chebyshev_moments", check_args(), d_vin, nprobes, d_probes, nmom, a, b, nullptr, nullptr, moments, self_moments, nullptr);
}

int hxv_chebyshev_apply(hxv_handle* h, const void* d_vin, int32_t ncoef, const double* coef, double a, double b, void* d_out, double* norm2) {
  if (!h) return fail(HXV_ERR_ARG, "hxv_chebyshev_apply: NULL handle");
  auto check_args = [&]() -> int {
    if (!d_vin || !d_out || !coef || ncoef < 1) return fail(HXV_ERR_ARG, "hxv_chebyshev_apply: bad argument (NULL vector or coefficients, or ncoef < 1)");
    if (d_out == d_vin) return fail(HXV_ERR_ARG, "hxv_chebyshev_apply: d_out must not be d_vin");
    if (!window_ok(a, b)) return fail(HXV_ERR_ARG, "hxv_chebyshev_apply: the window needs a > 0 and finite a, b");
    for (int k = 0; k < 2 * ncoef; ++k)
      if (!std::isfinite(coef[k])) return fail(HXV_ERR_ARG, "hxv_chebyshev_apply: a coefficient is not finite");
    if (comm_ready(h) && comm_in_gather(h, d_out)) return fail(HXV_ERR_ARG, "hxv_chebyshev_apply: d_out lies in a gather buffer of the handle (hxv_slab_home): the exchange overwrites that place");
    return HXV_OK;
  };
  return chebyshev_run(h, "hxv_chebyshev_apply", check_args(), d_vin, 0, nullptr, ncoef, a, b, coef, (double2*)d_out, nullptr, nullptr, norm2);
}

}  // extern "C"
