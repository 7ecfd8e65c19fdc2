// The host routines of hxv_eigh_lowest (hxv_eigh.hip): the dense eigensolver of the projected matrix, the restart's keep rule and the
// orthogonality estimate that decides when the whole basis is cleaned.
// Pure C++17, no HIP include: tests/host/eigh_small_check.cpp builds this file with a host compiler (and its sanitizers) alone.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

namespace {

// Cyclic Jacobi for a small dense real symmetric matrix (column-major n x n in A, destroyed).
// On exit w = eigenvalues ascending, Z[:, i] = eigenvector i.
bool jacobi_eigh(int n, std::vector<double>& A, std::vector<double>& w, std::vector<double>& Z) {
  Z.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) Z[i + (size_t)i * n] = 1.0;
  auto a = [&](int i, int j) -> double& { return A[i + (size_t)j * n]; };
  double scale = 0.0;
  for (double x : A) scale = std::max(scale, std::fabs(x));
  if (scale == 0.0) scale = 1.0;
  bool done = false;
  for (int sweep = 0; sweep < 100 && !done; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) off += a(p, q) * a(p, q);
    if (std::sqrt(off) <= 1e-15 * scale) {
      done = true;
      break;
    }
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = a(p, q);
        if (std::fabs(apq) <= 1e-300) continue;
        const double tau = (a(q, q) - a(p, p)) / (2.0 * apq);
        const double t = (tau >= 0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
        for (int r = 0; r < n; ++r) {  // columns p, q
          const double arp = a(r, p), arq = a(r, q);
          a(r, p) = c * arp - s * arq;
          a(r, q) = s * arp + c * arq;
        }
        for (int r = 0; r < n; ++r) {  // rows p, q
          const double apr = a(p, r), aqr = a(q, r);
          a(p, r) = c * apr - s * aqr;
          a(q, r) = s * apr + c * aqr;
        }
        a(p, q) = a(q, p) = 0.0;
        for (int r = 0; r < n; ++r) {
          const double zrp = Z[r + (size_t)p * n], zrq = Z[r + (size_t)q * n];
          Z[r + (size_t)p * n] = c * zrp - s * zrq;
          Z[r + (size_t)q * n] = s * zrp + c * zrq;
        }
      }
  }
  std::vector<int> idx(n);
  for (int i = 0; i < n; ++i) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](int x, int y) { return a(x, x) < a(y, y); });
  w.resize(n);
  std::vector<double> Zs((size_t)n * n);
  for (int i = 0; i < n; ++i) {
    w[i] = a(idx[i], idx[i]);
    std::memcpy(&Zs[(size_t)i * n], &Z[(size_t)idx[i] * n], (size_t)n * sizeof(double));
  }
  Z.swap(Zs);
  return done;
}

// Ritz pairs kept at a restart: the wanted ones, those already converged, and a share of the rest of the basis (option "eigh_keep_pct",
// per cent of m - neigen; the restart cycle then has m - k new products)
int keep_count(int m, int neigen, int nconv, int pct) {
  int k = neigen + std::min(nconv, (m - neigen) / 2) + std::max(1, (m - neigen) * pct / 100);
  return std::max(1, std::min(k, m - 1));
}

// Partial re-orthogonalisation (Simon 1984) in its thick-restart form: the loss of orthogonality of the next Lanczos vector against
// every earlier basis vector is ESTIMATED from the recurrence the exact quantities obey (<q_j, v_b>: prev = step j-1, cur = step j,
// next = step j+1, indexed by the ABSOLUTE basis slot b), so the whole basis is only touched when an estimate says so.  The active
// basis starts at slot nlock; T is its projected matrix (column-major ma x ma), whose first k rows are the kept Ritz pairs
// (theta_keep) with their arrow (s_keep).
struct OmegaEstimate {
  static constexpr double EPS = 2.220446049250313e-16;
  std::vector<double> prev, cur, next;
  explicit OmegaEstimate(int size = 0) : prev(size, EPS), cur(size, EPS), next(size, EPS) {}
  // a restart: the new cycle's estimates start from rounding level (next is written before it is read)
  void reset() {
    std::fill(prev.begin(), prev.end(), EPS);
    std::fill(cur.begin(), cur.end(), EPS);
  }
  // the rounding level of a step's estimates: |T|'s diagonal up to row j against the new vector's length
  static double noise_level(const std::vector<double>& T, int ma, int j, double nrm) {
    double tsc = 1.0;
    for (int a = 0; a <= j; ++a) tsc = std::max(tsc, std::fabs(T[a + (size_t)a * ma]));
    return 2.0 * EPS * tsc / std::max(nrm, 1e-300);
  }
  // the new vector was measured against slots 0..jt and those projections removed: orthogonal to rounding
  void cleaned(int jt, double noise) { std::fill_n(next.begin(), jt + 1, noise); }
  // step j of the active basis (slot jt = nlock + j) took the two local projections only; nrm = the new vector's length.
  // Returns the largest estimate among the slots b < jt - 1 that the step did not touch.
  double local_step(const std::vector<double>& T, int ma, int nlock, int k, int j, const std::vector<double>& theta_keep,
                    const std::vector<double>& s_keep, double noise, double nrm) {
    const int jt = nlock + j;
    auto t_at = [&](int a, int b) { return T[a + (size_t)b * ma]; };
    auto omc = [&](int x) -> double { return x == jt ? 1.0 : (x == jt - 1 ? noise : cur[x]); };
    const double alpha_j = t_at(j, j), beta_j = j > k ? t_at(j, j - 1) : 0.0;
    double maxom = 0.0;
    for (int b = 0; b < jt - 1; ++b) {
      if (b < nlock) {
        next[b] = noise;  // measured and removed at every step (gs_local)
        continue;
      }
      const int l = b - nlock;
      double at;
      if (l < k) {
        at = theta_keep[l] * cur[b] + s_keep[l] * omc(nlock + k);
      } else {
        at = t_at(l, l) * cur[b] + t_at(l + 1, l) * omc(b + 1);
        if (l > k)
          at += t_at(l, l - 1) * omc(b - 1);
        else
          for (int i2 = 0; i2 < k; ++i2) at += s_keep[i2] * omc(nlock + i2);
      }
      double val = (at - alpha_j * cur[b] - beta_j * prev[b]) / std::max(nrm, 1e-300);
      val += std::copysign(noise, val);
      next[b] = val;
      maxom = std::max(maxom, std::fabs(val));
    }
    next[jt - 1 < 0 ? 0 : jt - 1] = noise;
    next[jt] = noise;
    return maxom;
  }
  void advance() { prev.swap(cur), cur.swap(next); }  // the step is taken: j becomes j + 1
};

}  // namespace
