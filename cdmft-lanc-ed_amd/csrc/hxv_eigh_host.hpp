// The two host routines of hxv_eigh_lowest (hxv_eigh.hip): the dense eigensolver of the projected matrix and the restart's keep rule.
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

}  // namespace
