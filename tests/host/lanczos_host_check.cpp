// TEST-ONLY: the host routines of the Lanczos drivers run alone (csrc/hxv_lanczos_host.hpp, nothing else of the project): no HIP, no device.
// Driven by tests/test_host_lanczos_check.py, plain and under -fsanitize=address,undefined.
//
//   lanczos_host_check ql FILE     FILE: any number of matrices, each "n" followed by d[0..n-1] and e[0..n-1] (e[0] unused, e[i] couples i-1 and
//                                  i, as the drivers pass them; strtod: hex floats are exact).  tridiag_ql runs twice, with eigenvectors and
//                                  without.  Per matrix one line:
//                                    conv=<0|1> conv_noz=<0|1> same=<0|1> n=<n> res=<max|T z - lambda z|> orth=<max|Z^T Z - I|> | lambda_0 .. lambda_{n-1}
//                                  same: the eigenvalues without z have the bits of those with z; res and orth are evaluated in long double;
//                                  lambda in the order tridiag_ql leaves them; numbers as hex floats (%a)
//   lanczos_host_check scale FILE  FILE: lines "nrm beta_1 beta_2 ...".  Per line: LzScale::begin(nrm), then next(beta_k) in turn; after begin
//                                  and after every next one triple "s_cur beta_prev c()" (hex floats), all on one line
//   lanczos_host_check norm X...   start_norm(X) for every argument (hex floats), one per line
//   lanczos_host_check ritz FILE   FILE: matrices as for ql.  lowest_ritz, with the eigenvector and without, beside the sequence it stands for
//                                  written out here: identity, tridiag_ql, std::min_element.  Per matrix one line:
//                                    ok=<0|1> ok_ref=<0|1> same=<0|1> same_noy=<0|1> j=<index of the lowest eigenvalue> n=<n> e=<it>
//                                  same: eigenvalue, index and vector have the bits of the written-out sequence; same_noy: so has the
//                                  eigenvalue asked for without the vector (against tridiag_ql without z); after a failure only the flags count
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "hxv_lanczos_host.hpp"

static bool read_double(FILE* f, double* out) {
  char tok[128];
  char* end = nullptr;
  if (std::fscanf(f, "%127s", tok) != 1) return false;
  *out = std::strtod(tok, &end);
  return *end == 0;
}

static int run_ql(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    return 2;
  }
  int n = 0;
  while (std::fscanf(f, "%d", &n) == 1) {
    if (n < 1 || n > 4096) {  // (n = 0 is outside tridiag_ql's contract: it writes e[n-1])
      std::fprintf(stderr, "bad n %d\n", n);
      std::fclose(f);
      return 2;
    }
    std::vector<double> d0(n), e0(n);
    for (int pass = 0; pass < 2; ++pass)
      for (int i = 0; i < n; ++i)
        if (!read_double(f, pass ? &e0[i] : &d0[i])) {
          std::fprintf(stderr, "bad number in %s\n", path);
          std::fclose(f);
          return 2;
        }
    std::vector<double> d = d0, e = e0, z((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) z[i + (size_t)i * n] = 1.0;
    const bool conv = tridiag_ql(n, d, e, &z);
    std::vector<double> d2 = d0, e2 = e0;
    const bool conv2 = tridiag_ql(n, d2, e2, nullptr);
    const bool same = std::memcmp(d.data(), d2.data(), (size_t)n * sizeof(double)) == 0;
    // residual and orthogonality in long double, against the matrix as it was given
    long double res = 0.0L, orth = 0.0L;
    for (int j = 0; j < n; ++j) {
      const double* zj = &z[(size_t)j * n];
      for (int k = 0; k < n; ++k) {
        long double t = (long double)d0[k] * zj[k] - (long double)d[j] * zj[k];
        if (k > 0) t += (long double)e0[k] * zj[k - 1];
        if (k + 1 < n) t += (long double)e0[k + 1] * zj[k + 1];
        const long double a = fabsl(t);
        if (!(a <= res)) res = a;  // (a NaN stays)
      }
      for (int i = 0; i <= j; ++i) {
        const double* zi = &z[(size_t)i * n];
        long double s = i == j ? -1.0L : 0.0L;
        for (int k = 0; k < n; ++k) s += (long double)zi[k] * zj[k];
        const long double a = fabsl(s);
        if (!(a <= orth)) orth = a;
      }
    }
    std::printf("conv=%d conv_noz=%d same=%d n=%d res=%a orth=%a |", conv ? 1 : 0, conv2 ? 1 : 0, same ? 1 : 0, n, (double)res, (double)orth);
    for (double x : d) std::printf(" %a", x);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}

static int run_ritz(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    return 2;
  }
  int n = 0;
  while (std::fscanf(f, "%d", &n) == 1) {
    if (n < 1 || n > 4096) {
      std::fprintf(stderr, "bad n %d\n", n);
      std::fclose(f);
      return 2;
    }
    std::vector<double> al(n), be(n);
    for (int pass = 0; pass < 2; ++pass)
      for (int i = 0; i < n; ++i)
        if (!read_double(f, pass ? &be[i] : &al[i])) {
          std::fprintf(stderr, "bad number in %s\n", path);
          std::fclose(f);
          return 2;
        }
    // the sequence as hxv_lanczos_eigh wrote it out before the helper existed
    std::vector<double> d = al, e = be, z((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) z[i + (size_t)i * n] = 1.0;
    const bool ok_ref = tridiag_ql(n, d, e, &z);
    const int j_ref = (int)(std::min_element(d.begin(), d.end()) - d.begin());
    std::vector<double> d2 = al, e2 = be;
    const bool ok_ref2 = tridiag_ql(n, d2, e2, nullptr);
    const double e_ref2 = *std::min_element(d2.begin(), d2.end());
    double e_min = 0.0, e_noy = 0.0;
    int j = -1;
    std::vector<double> y;
    const bool ok = lowest_ritz(al, be, &e_min, &y, &j);
    const bool ok2 = lowest_ritz(al, be, &e_noy, nullptr);
    const bool same = ok && ok_ref && j == j_ref && std::memcmp(&e_min, &d[j_ref], sizeof(double)) == 0 && y.size() == (size_t)n &&
                      std::memcmp(y.data(), &z[(size_t)j_ref * n], (size_t)n * sizeof(double)) == 0;
    const bool same_noy = ok2 && ok_ref2 && std::memcmp(&e_noy, &e_ref2, sizeof(double)) == 0;
    std::printf("ok=%d ok_ref=%d same=%d same_noy=%d j=%d n=%d e=%a\n", (ok && ok2) ? 1 : 0, (ok_ref && ok_ref2) ? 1 : 0, same ? 1 : 0, same_noy ? 1 : 0, j, n, e_min);
  }
  std::fclose(f);
  return 0;
}

static int run_scale(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    return 2;
  }
  char line[1 << 16];
  while (std::fgets(line, sizeof line, f)) {
    LzScale sc;
    bool first = true;
    for (char* tok = std::strtok(line, " \t\n"); tok; tok = std::strtok(nullptr, " \t\n")) {
      char* end = nullptr;
      const double x = std::strtod(tok, &end);
      if (*end != 0) {
        std::fprintf(stderr, "bad number in %s\n", path);
        std::fclose(f);
        return 2;
      }
      if (first)
        sc.begin(x);
      else
        sc.next(x);
      first = false;
      std::printf("%a %a %a ", sc.s_cur, sc.beta_prev, sc.c());
    }
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "ql" && argc == 3) return run_ql(argv[2]);
  if (mode == "scale" && argc == 3) return run_scale(argv[2]);
  if (mode == "ritz" && argc == 3) return run_ritz(argv[2]);
  if (mode == "norm" && argc >= 3) {
    for (int a = 2; a < argc; ++a) std::printf("%a\n", start_norm(std::strtod(argv[a], nullptr)));
    return 0;
  }
  std::fprintf(stderr, "usage: lanczos_host_check ql FILE | scale FILE | ritz FILE | norm X...\n");
  return 2;
}
