// The host routines of the Lanczos drivers (hxv_lanczos.hip): the eigen-solver of the tridiagonal matrix, the lowest Ritz pair taken from it,
// the host's copy of the fused recurrence's scale factors and the rule for the norm a recurrence starts from.  Host C++ only, no HIP: the header lives apart so that
// tests/host/lanczos_host_check.cpp can compile it with a plain host compiler, under sanitizers, and
// tests/device/lanczos_kernels_check.hip can set LzScale beside lz_next.  Anonymous namespace: each including file gets its own copy,
// exactly as when the text stood in hxv_lanczos.hip.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace {

// Symmetric tridiagonal eigen-solver (implicit QL with Wilkinson shifts): d[n] diagonal,
// e[n] sub-diagonal in e[1..n-1] (e[0] unused).  On exit d = eigenvalues (unsorted) and, if z,
// z (n x n, column-major, initialised to identity by the caller) = eigenvectors.
bool tridiag_ql(int n, std::vector<double>& d, std::vector<double>& e, std::vector<double>* z) {
  for (int i = 1; i < n; ++i) e[i - 1] = e[i];
  e[n - 1] = 0.0;
  for (int l = 0; l < n; ++l) {
    int iter = 0, m;
    do {
      for (m = l; m < n - 1; ++m) {
        double dd = std::fabs(d[m]) + std::fabs(d[m + 1]);
        if (std::fabs(e[m]) <= 2.3e-16 * dd) break;
      }
      if (m != l) {
        if (iter++ == 200) return false;
        double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
        double r = std::hypot(g, 1.0);
        g = d[m] - d[l] + e[l] / (g + (g >= 0 ? std::fabs(r) : -std::fabs(r)));
        double s = 1.0, c = 1.0, p = 0.0;
        int i;
        for (i = m - 1; i >= l; --i) {
          double f = s * e[i], b = c * e[i];
          r = std::hypot(f, g);
          e[i + 1] = r;
          if (r == 0.0) {
            d[i + 1] -= p;
            e[m] = 0.0;
            break;
          }
          s = f / r;
          c = g / r;
          g = d[i + 1] - p;
          r = (d[i] - g) * s + 2.0 * c * b;
          p = s * r;
          d[i + 1] = g + p;
          g = c * r - b;
          if (z)
            for (int k = 0; k < n; ++k) {
              double* zz = z->data();
              f = zz[k + (size_t)(i + 1) * n];
              zz[k + (size_t)(i + 1) * n] = s * zz[k + (size_t)i * n] + c * f;
              zz[k + (size_t)i * n] = c * zz[k + (size_t)i * n] - s * f;
            }
        }
        if (r == 0.0 && i >= l) continue;
        d[l] -= p;
        e[l] = g;
        e[m] = 0.0;
      }
    } while (m != l);
  }
  return true;
}

// The lowest Ritz pair of a Lanczos matrix: al[m] its diagonal, be its sub-diagonal as the drivers keep it (be[0] unused, be[i] couples i - 1
// and i; entries be does not have are zero).  -> false when the QL iteration did not converge.  *e_min: the lowest eigenvalue, *j_min (may be
// null) its index in tridiag_ql's order (the first of equal ones); y (may be null: eigenvalues only) its eigenvector, m entries.
inline bool lowest_ritz(const std::vector<double>& al, const std::vector<double>& be, double* e_min, std::vector<double>* y, int* j_min = nullptr) {
  const int m = (int)al.size();
  std::vector<double> d = al, e = be, z;
  e.resize(m, 0.0);
  if (y) {
    z.assign((size_t)m * m, 0.0);
    for (int i = 0; i < m; ++i) z[i + (size_t)i * m] = 1.0;
  }
  if (!tridiag_ql(m, d, e, y ? &z : nullptr)) return false;
  const int j = (int)(std::min_element(d.begin(), d.end()) - d.begin());
  *e_min = d[j];
  if (j_min) *j_min = j;
  if (y) y->assign(z.begin() + (size_t)j * m, z.begin() + (size_t)(j + 1) * m);
  return true;
}

// The norm a recurrence starts from.  SciFortran's sp_lanc_tridiag normalises vin on its first iteration; the reference's call sites pass a
// normalised vector already (ED_GF_NORMAL.f90:197-199): a measured norm that is 1 to rounding is taken as exactly 1.
inline double start_norm(double nrm) { return std::fabs(nrm - 1.0) <= 1e-14 ? 1.0 : nrm; }

// The host's copy of one component's scale factors in the fused recurrence: the stored vector X_k times s_cur = 1/beta_k is the unit Lanczos
// vector, beta_prev = beta_{k-1} (the start vector's norm is carried as beta_0).
struct LzScale {
  double s_cur = 1.0, beta_prev = 1.0;
  void begin(double nrm) {
    s_cur = 1.0 / nrm;
    beta_prev = nrm;
  }
  double c() const { return 1.0 / (s_cur * beta_prev); }  // beta_k / beta_{k-1}: what LZ_C holds from the second step on
  // after a step that returned beta_{k+1}  (lz_next does the same operations, in the same order, on the device: bit-identical recurrences)
  void next(double beta) {
    beta_prev = 1.0 / s_cur;
    s_cur = 1.0 / beta;
  }
};

}  // namespace
