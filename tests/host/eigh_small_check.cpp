// TEST-ONLY: the two host routines of hxv_eigh_lowest run alone (csrc/hxv_eigh_host.hpp, nothing else of the project): no HIP, no device.
// Driven by tests/test_host_eigh_small_check.py, plain and under -fsanitize=address,undefined.
//
//   eigh_small_check eigh FILE    FILE: any number of matrices, each "n" followed by n*n numbers, column-major (strtod: hex floats are exact).
//                                 Per matrix one line:  done=<0|1> n=<n> | w_0 .. w_{n-1} | Z column-major     numbers as hex floats (%a)
//   eigh_small_check keep PCT..   one line "m neigen nconv pct k" for every 2 <= m <= 64, 1 <= neigen < m, 0 <= nconv <= neigen and every PCT
#include <cstdio>
#include <cstdlib>
#include <string>

#include "hxv_eigh_host.hpp"

static int run_eigh(const char* path) {
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
    std::vector<double> A((size_t)n * n), w, Z;
    char tok[128];
    for (size_t i = 0; i < A.size(); ++i) {
      char* end = nullptr;
      if (std::fscanf(f, "%127s", tok) != 1 || (A[i] = std::strtod(tok, &end), *end != 0)) {
        std::fprintf(stderr, "bad number in %s\n", path);
        std::fclose(f);
        return 2;
      }
    }
    const bool done = jacobi_eigh(n, A, w, Z);
    if ((int)w.size() != n || Z.size() != (size_t)n * n) {
      std::fprintf(stderr, "FAIL: output sizes %zu %zu for n = %d\n", w.size(), Z.size(), n);
      std::fclose(f);
      return 1;
    }
    std::printf("done=%d n=%d |", done ? 1 : 0, n);
    for (double x : w) std::printf(" %a", x);
    std::printf(" |");
    for (double x : Z) std::printf(" %a", x);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}

static int run_keep(int argc, char** argv) {
  for (int a = 2; a < argc; ++a) {
    const int pct = std::atoi(argv[a]);
    for (int m = 2; m <= 64; ++m)
      for (int neigen = 1; neigen < m; ++neigen)
        for (int nconv = 0; nconv <= neigen; ++nconv) std::printf("%d %d %d %d %d\n", m, neigen, nconv, pct, keep_count(m, neigen, nconv, pct));
  }
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "eigh" && argc == 3) return run_eigh(argv[2]);
  if (mode == "keep" && argc >= 3) return run_keep(argc, argv);
  std::fprintf(stderr, "usage: eigh_small_check eigh FILE | eigh_small_check keep PCT...\n");
  return 2;
}
