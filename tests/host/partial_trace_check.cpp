// Stand-alone check of the partial-trace tables (csrc/hxv_partial_trace_host.hpp).  No HIP runtime call, no device.
//
//   partial_trace_check MODEL nup ndw RANKS SPEC [SPEC ...]
//
// MODEL is a file with the fields of hxv_model in the array order of HxvSector._model_struct (tests/test_host_plan_check.py writes it); RANKS a
// comma-separated list of rank counts; SPEC is "cluster" (the cluster density matrix) or MASK:FERMI[:SMALL_N] (the subset density matrix of
// the orbital mask, hexadecimal, in the sign convention FERMI; SMALL_N 0 = the hook that sends every class to the tile kernel).  For every
// (SPEC, rank count) and every rank, the sector is built by build_sector_from_model, its groups by the front end's enumeration and its tables
// by pt_build, for 256 compute units and for one.  Every table is then read through one bounds-checked accessor, the way the kernels and the
// scatter read it:
//   partition   over the ranks, every (device row < DimUp, column of the sector) is named by exactly one (class, pair, component); no pad row,
//               no unused slot of the gathered copy
//   work list   the items of a class are contiguous slices covering its pairs, in the order of the three launches; the partial blocks are
//               disjoint and inside the partial buffer; the reduction's tables name exactly the element's copies; the class blocks of the
//               output are disjoint
//   kernels     what pt_pair_kernel and pt_tile_kernel assume of a class (batch, stride, tile count, nrep, tile words, n <= 4)
//   signs       recomputed from their definitions: row bit = basis sign of the device row xor the Fermi parity of the configuration, column
//               bit = the Fermi parity
//   replay      rho formed from the tables by plain loops (class -> pair -> outer product -> dense matrix), summed over the ranks, against
//               the partial trace taken straight from the basis maps: within 1e-13 at trace 0.7
// Nothing here calls a helper of the builder or of the enumerations.  Output: one line "CASE ..." per (SPEC, rank count), and one line
// "REACH ..." with the paths the 256-CU work list makes the tile kernel take.  Exit status 0, or
// 1 with the first failed check on stderr; abort() from the accessor on an out-of-range table read.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hxv_internal.hpp"
#include "hxv_partial_trace_host.hpp"

using namespace hxv;

namespace {
// what the kernels hard-code: restated, and held equal to the header's
constexpr int K_THREADS = 256, K_XS = 2048, K_PAIR_N = 4;
static_assert(K_THREADS == PT_THREADS && K_XS == PT_XS && K_PAIR_N == PT_PAIR_N, "the partial-trace kernels' constants changed");
constexpr double TOL = 1e-13, TRACE = 0.7;

std::string fmt(const char* f, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}
std::string g_case;
[[noreturn]] void die(const std::string& msg) {
  fflush(stdout);
  fprintf(stderr, "partial_trace_check: FAIL: %s: %s\n", g_case.c_str(), msg.c_str());
  exit(1);
}
#define REQUIRE(cond, ...)              \
  do {                                  \
    if (!(cond)) die(fmt(__VA_ARGS__)); \
  } while (0)

int64_t g_words = 0;  // table words read through the accessor
template <typename T>
struct Tab {
  const char* name;
  const std::vector<T>& v;
  const T& operator[](int64_t i) const {
    if (i < 0 || (size_t)i >= v.size()) {
      fflush(stdout);
      fprintf(stderr, "partial_trace_check: OUT OF RANGE: %s: table %s index %" PRId64 " size %zu\n", g_case.c_str(), name, i, v.size());
      abort();
    }
    ++g_words;
    return v[(size_t)i];
  }
};

struct ModelFile {
  hxv_model m{};
  std::vector<double> h, hb, vb;
};
void read_model(const char* path, ModelFile& f) {
  FILE* fp = fopen(path, "rb");
  REQUIRE(fp != nullptr, "cannot open model file %s", path);
  int32_t head[6];
  double sc[10];
  int64_t len[3];
  REQUIRE(fread(head, sizeof head, 1, fp) == 1 && fread(sc, sizeof sc, 1, fp) == 1 && fread(len, sizeof len, 1, fp) == 1, "model file %s: short header", path);
  f.m.nlat = head[0], f.m.norb = head[1], f.m.nspin = head[2], f.m.nbath = head[3], f.m.hfmode = head[4], f.m.reserved = 0;
  for (int i = 0; i < 5; ++i) f.m.uloc[i] = sc[i];
  f.m.ust = sc[5], f.m.jh = sc[6], f.m.jx = sc[7], f.m.jp = sc[8], f.m.xmu = sc[9];
  std::vector<double>* arr[3] = {&f.h, &f.hb, &f.vb};
  for (int a = 0; a < 3; ++a) {
    REQUIRE(len[a] >= 0 && len[a] < ((int64_t)1 << 28), "model file %s: bad array length", path);
    arr[a]->resize((size_t)len[a]);
    if (len[a]) REQUIRE(fread(arr[a]->data(), sizeof(double), (size_t)len[a], fp) == (size_t)len[a], "model file %s: short array", path);
  }
  fclose(fp);
  f.m.imphloc = f.h.data();
  f.m.hbath = f.m.nbath > 0 ? f.hb.data() : nullptr;
  f.m.vbath = f.m.nbath > 0 ? f.vb.data() : nullptr;
}

// ---- the definitions, written out -------------------------------------------------------------------------------------------------------
// the bits of S in m, compressed in ascending orbital order
uint32_t compress(uint32_t m, uint32_t S) {
  uint32_t a = 0;
  for (int o = 0, k = 0; o < 32; ++o)
    if (S >> o & 1u) a |= (m >> o & 1u) << k++;
  return a;
}
// parity of the number of (occupied r in S, occupied o outside S, o < r)
uint32_t fermi_parity(uint32_t m, uint32_t S) {
  int n = 0;
  for (int r = 0; r < 32; ++r)
    for (int o = 0; o < r; ++o)
      if ((S >> r & 1u) && (m >> r & 1u) && !(S >> o & 1u) && (m >> o & 1u)) ++n;
  return (uint32_t)(n & 1);
}
// amplitude of (reference row i, column j): a fixed pseudo-random complex number
std::complex<double> amplitude(int64_t i, int64_t j) {
  uint64_t x = (uint64_t)(i * 1000003 + j) * 0x9E3779B97F4A7C15ull + 0x1234567ull;
  auto next = [&]() {
    x ^= x >> 30, x *= 0xBF58476D1CE4E5B9ull, x ^= x >> 27, x *= 0x94D049BB133111EBull, x ^= x >> 31;
    return (double)(x >> 11) / (double)(1ull << 53) - 0.5;
  };
  const double re = next();
  return {re, next()};
}

struct Spec {
  bool cluster = false;
  uint32_t mask = 0;
  int fermi = 0, small_n = 0;
  std::string text;
};

using cd = std::complex<double>;
// the sign bit of every up configuration (by reference row) and dw configuration of the sector in the case's convention
struct Parity {
  std::vector<uint8_t> up, dw;
};

// the partial trace straight from the basis maps: rho(a, a') = sum over the traced configurations of psi(a, e) conj psi(a', e)
std::vector<cd> direct(const SectorHost& s, uint32_t S, int nsub, const Parity& par, const std::vector<cd>& psi) {
  const int64_t nn = (int64_t)1 << (2 * nsub);
  std::vector<cd> rho((size_t)(nn * nn));
  struct Amp {
    uint64_t env;  // the traced bits of both spins
    int64_t a;     // the kept configuration
    cd v;
  };
  std::vector<Amp> amps;
  for (int j = 0; j < s.dimdw; ++j)
    for (int i = 0; i < s.dimup; ++i) {
      const uint32_t mu = s.map_up[i], md = s.map_dw[j];
      const double sg = (par.up[i] ^ par.dw[j]) ? -1.0 : 1.0;
      amps.push_back({(uint64_t)(mu & ~S) | ((uint64_t)(md & ~S) << 32), (int64_t)compress(mu, S) + ((int64_t)compress(md, S) << nsub), sg * psi[(size_t)((int64_t)j * s.dimup + i)]});
    }
  std::stable_sort(amps.begin(), amps.end(), [](const Amp& x, const Amp& y) { return x.env < y.env; });
  for (size_t b = 0, e; b < amps.size(); b = e) {
    for (e = b + 1; e < amps.size() && amps[e].env == amps[b].env; ++e) {
    }
    for (size_t x = b; x < e; ++x)
      for (size_t y = b; y < e; ++y) rho[(size_t)(amps[x].a + nn * amps[y].a)] += amps[x].v * std::conj(amps[y].v);
  }
  return rho;
}

struct Totals {
  int64_t classes = 0, pairs = 0, items = 0;
};

// one rank's tables: everything but the partition's and the replay's sums, which go into seen / rho
void check_rank(const SectorHost& s, const Spec& sp, uint32_t S, int nsub, const PtHostTables& t, const Parity& par, const std::vector<cd>& psi,
                const PtHostTables* rank0, std::vector<uint8_t>& seen, std::vector<cd>& rho, Totals& tot) {
  const Tab<PtClass> cls{"cls", t.cls};
  const Tab<PtClassHost> hcls{"hcls", t.hcls};
  const Tab<PtItem> items{"items", t.items};
  const Tab<uint32_t> rows{"rows", t.rows}, cols{"cols", t.cols}, tiles{"tiles", t.tiles};
  const Tab<int64_t> el_src{"el_src", t.el_src};
  const Tab<int32_t> el_cnt{"el_cnt", t.el_cnt}, el_stride{"el_stride", t.el_stride};
  const int ncls = (int)t.cls.size();
  REQUIRE(t.nsub == nsub && t.hcls.size() == t.cls.size(), "nsub %d, %zu classes with %zu host records", t.nsub, t.cls.size(), t.hcls.size());
  REQUIRE((int64_t)t.items.size() == (int64_t)t.nitems[0] + t.nitems[1] + t.nitems[2], "%zu items, the three launches take %d + %d + %d", t.items.size(),
          t.nitems[0], t.nitems[1], t.nitems[2]);
  REQUIRE((int64_t)t.el_src.size() == t.out_elems && (int64_t)t.el_cnt.size() == t.out_elems && (int64_t)t.el_stride.size() == t.out_elems,
          "the reduction's tables do not have out_elems = %" PRId64 " entries", t.out_elems);
  if (rank0) REQUIRE(rank0->cls.size() == t.cls.size() && rank0->out_elems == t.out_elems, "rank %d has another class list than rank 0", s.rank);
  // the columns of each rank, by dw_split itself
  std::vector<int> rq(s.nranks), rc0(s.nranks);
  for (int p = 0; p < s.nranks; ++p) dw_split(s.dimdw, p, s.nranks, rq[p], rc0[p]);
  // the work list: which launch an item belongs to, and the slices of each class
  std::vector<int> first_item(ncls, -1), n_items(ncls, 0), launch(ncls, -1);
  for (int k = 0; k < (int)t.items.size(); ++k) {
    const PtItem it = items[k];
    REQUIRE(it.cls >= 0 && it.cls < ncls, "item %d names class %d of %d", k, it.cls, ncls);
    const int l = k < t.nitems[0] ? 0 : k < t.nitems[0] + t.nitems[1] ? 1 : 2;
    if (first_item[it.cls] < 0) first_item[it.cls] = k, launch[it.cls] = l;
    REQUIRE(launch[it.cls] == l && first_item[it.cls] + n_items[it.cls] == k, "item %d: the items of class %d are not one run of one launch", k, it.cls);
    ++n_items[it.cls];
  }
  std::vector<std::pair<int64_t, int64_t>> pblocks, oblocks;  // [first, end) of every partial block and of every class block
  for (int ci = 0; ci < ncls; ++ci) {
    const PtClass c = cls[ci];
    const PtClassHost& h = hcls[ci];
    ++tot.classes;
    // ---- what the kernels assume
    REQUIRE(c.du >= 1 && c.dd >= 1 && c.n == c.du * c.dd && (int)h.au.size() == c.du && (int)h.ad.size() == c.dd, "class %d: shape %d x %d, n %d", ci, c.du, c.dd, c.n);
    REQUIRE(c.t == 2 || c.t == 4, "class %d: tile edge %d", ci, c.t);
    const int NT = c.t == 2 ? 1 : 2;
    REQUIRE(c.nt == (c.n + c.t - 1) / c.t && c.ntiles == c.nt * (c.nt + 1) / 2 && c.ntiles <= NT * K_THREADS, "class %d: n %d in %d tiles of edge %d (nt %d)", ci, c.n,
            c.ntiles, c.t, c.nt);
    REQUIRE(c.batch >= 1 && (int64_t)c.dd * c.stride <= K_XS && c.stride % 16 == c.du % 16 && c.stride >= c.batch * c.du, "class %d: batch %d stride %d for %d x %d", ci,
            c.batch, c.stride, c.du, c.dd);
    const int64_t npairs = (int64_t)c.ngu * h.ngd, sz = (int64_t)c.ntiles * c.t * c.t;
    // a class without pairs on this rank has no item: its launch is the one its shape says
    const bool pair_class = n_items[ci] ? launch[ci] == 0 : c.n <= sp.small_n;
    if (n_items[ci]) REQUIRE(pair_class || launch[ci] == (c.t == 2 ? 1 : 2), "class %d with tile edge %d is in launch %d", ci, c.t, launch[ci]);
    if (pair_class) REQUIRE(c.n <= K_PAIR_N && c.t == 2 && c.ntiles * 4 <= K_THREADS, "class %d with n = %d is given to the pair kernel", ci, c.n);
    REQUIRE(pair_class == (c.n <= sp.small_n), "class %d with n = %d: pair kernel %d, small_n %d", ci, c.n, (int)pair_class, sp.small_n);
    REQUIRE(c.nrep == ((!pair_class && c.ntiles <= 64) ? 4 : 1), "class %d: nrep %d with %d tiles, pair kernel %d", ci, c.nrep, c.ntiles, (int)pair_class);
    std::vector<int> met((size_t)c.nt * c.nt, 0);
    for (int k = 0; k < c.ntiles; ++k) {
      const uint32_t pk = tiles[c.tile_off + k];
      const int ti = (int)(pk & 0xffffu), tj = (int)(pk >> 16);
      REQUIRE(ti <= tj && tj < c.nt && !met[(size_t)ti * c.nt + tj]++ && (int)h.tiles.size() == c.ntiles && h.tiles[k] == pk, "class %d: tile word %d = (%d, %d)", ci, k, ti, tj);
    }
    if (rank0) {
      const PtClass& c0 = rank0->cls[ci];
      const PtClassHost& h0 = rank0->hcls[ci];
      REQUIRE(c0.du == c.du && c0.dd == c.dd && c0.t == c.t && c0.ntiles == c.ntiles && h0.out_off == h.out_off && h0.au == h.au && h0.ad == h.ad && h0.tiles == h.tiles,
              "class %d of rank %d differs from rank 0's", ci, s.rank);
    }
    // ---- the work list of the class
    oblocks.push_back({h.out_off, h.out_off + sz});
    int64_t next = 0;
    for (int k = 0; k < n_items[ci]; ++k) {
      const PtItem it = items[first_item[ci] + k];
      REQUIRE(it.p0 == next && it.p1 > it.p0 && it.p1 <= npairs, "class %d: item %d takes pairs [%d, %d), %" PRId64 " were taken, of %" PRId64, ci, k, it.p0, it.p1, next, npairs);
      next = it.p1;
      pblocks.push_back({it.out_off, it.out_off + sz * c.nrep});
      for (int64_t e = 0; e < sz; ++e)
        for (int r = 0; r < c.nrep; ++r) {
          const int64_t q = (int64_t)k * c.nrep + r, oe = h.out_off + e;
          REQUIRE(el_src[oe] + q * el_stride[oe] == it.out_off + r * sz + e, "class %d: copy %" PRId64 " of element %" PRId64 " is not item %d's", ci, q, e, k);
        }
    }
    REQUIRE(next == npairs, "class %d: the items cover %" PRId64 " of %" PRId64 " pairs", ci, next, npairs);
    for (int64_t e = 0; e < sz; ++e) {
      const int64_t oe = h.out_off + e;
      REQUIRE(el_cnt[oe] == n_items[ci] * c.nrep && el_src[oe] >= 0 && (el_cnt[oe] == 0 || el_src[oe] + (int64_t)(el_cnt[oe] - 1) * el_stride[oe] < t.partial_elems),
              "class %d: element %" PRId64 " sums %d partials from %" PRId64 " by %d, the buffer holds %" PRId64, ci, e, el_cnt[oe], el_src[oe], el_stride[oe], t.partial_elems);
    }
    // ---- the pairs: partition, signs, replay
    std::vector<cd> block((size_t)c.n * c.n), x((size_t)c.n);
    const int ktr_up = s.nup - __builtin_popcount(h.au[0]), ktr_dw = s.ndw - __builtin_popcount(h.ad[0]);  // traced particles of the class
    for (int gd = 0; gd < h.ngd; ++gd)
      for (int g = 0; g < c.ngu; ++g) {
        ++tot.pairs;
        uint32_t env_up = 0, env_dw = 0;
        for (int k = 0; k < c.n; ++k) {
          const int iu = k % c.du, id = k / c.du;
          const uint32_t r = rows[c.rows_off + g * c.du + iu], cc = cols[c.cols_off + gd * c.dd + id];
          const int row = (int)(r & 0x7fffffffu), slot = (int)(cc & 0x7fffffffu);
          REQUIRE(row < s.dimup, "class %d pair (%d, %d): row %d of %d (a pad row?)", ci, g, gd, row, s.dimup);
          int col = slot;
          if (s.nranks > 1) {
            const int o = slot / s.cmax, off = slot % s.cmax;
            REQUIRE(o < s.nranks && off < rq[o], "class %d pair (%d, %d): slot %d is column %d of rank %d, which has %d", ci, g, gd, slot, off, o, o < s.nranks ? rq[o] : -1);
            col = rc0[o] + off;
          }
          REQUIRE(col < s.dimdw, "class %d pair (%d, %d): column %d of %d", ci, g, gd, col, s.dimdw);
          REQUIRE(seen[(size_t)col * s.dimup + row]++ == 0, "class %d pair (%d, %d): (row %d, column %d) is named twice", ci, g, gd, row, col);
          const int ref = s.row_order() ? s.up_iperm[row] : row;
          const uint32_t mu = s.map_up[ref], md = s.map_dw[col];
          REQUIRE(compress(mu, S) == h.au[iu] && compress(md, S) == h.ad[id], "class %d pair (%d, %d) component %d: kept bits 0x%x 0x%x, the block says 0x%x 0x%x", ci, g, gd, k,
                  compress(mu, S), compress(md, S), h.au[iu], h.ad[id]);
          if (k == 0) env_up = mu & ~S, env_dw = md & ~S;
          REQUIRE((mu & ~S) == env_up && (md & ~S) == env_dw && __builtin_popcount(env_up) == ktr_up && __builtin_popcount(env_dw) == ktr_dw,
                  "class %d pair (%d, %d) component %d: another traced configuration than component 0's", ci, g, gd, k);
          const uint32_t want_r = (s.row_order() && s.up_sign[row] ? 1u : 0u) ^ par.up[ref], want_c = par.dw[col];
          REQUIRE((r >> 31) == want_r && (cc >> 31) == want_c, "class %d pair (%d, %d) component %d: sign bits %u %u, by definition %u %u", ci, g, gd, k, r >> 31, cc >> 31,
                  want_r, want_c);
          // the device vector's element: the reference's times the basis sign of the device row
          const cd v = (s.row_order() && s.up_sign[row] ? -1.0 : 1.0) * psi[(size_t)((int64_t)col * s.dimup + ref)];
          x[k] = (((r ^ cc) >> 31) ? -1.0 : 1.0) * v;
        }
        for (int i = 0; i < c.n; ++i)
          for (int j = i; j < c.n; ++j) block[(size_t)i * c.n + j] += x[i] * std::conj(x[j]);
      }
    const int64_t nn = (int64_t)1 << (2 * nsub);
    for (int i = 0; i < c.n; ++i)
      for (int j = i; j < c.n; ++j) {
        const int64_t io = (int64_t)h.au[i % c.du] + ((int64_t)h.ad[i / c.du] << nsub), jo = (int64_t)h.au[j % c.du] + ((int64_t)h.ad[j / c.du] << nsub);
        rho[(size_t)(io + nn * jo)] += block[(size_t)i * c.n + j];
        if (i != j) rho[(size_t)(jo + nn * io)] += std::conj(block[(size_t)i * c.n + j]);
      }
  }
  tot.items += (int64_t)t.items.size();
  for (auto* b : {&pblocks, &oblocks}) {
    std::sort(b->begin(), b->end());
    const int64_t lim = b == &pblocks ? t.partial_elems : t.out_elems;
    for (size_t k = 0; k < b->size(); ++k)
      REQUIRE((*b)[k].first >= (k ? (*b)[k - 1].second : 0) && (*b)[k].second <= lim, "%s block [%" PRId64 ", %" PRId64 ") overlaps its neighbour or leaves the buffer of %" PRId64,
              b == &pblocks ? "partial" : "class", (*b)[k].first, (*b)[k].second, lim);
  }
}

// which paths of pt_tile_kernel the work list of one rank makes it take (read from items / cls as the kernel reads them): printed as a
// "REACH" line per (SPEC, rank count) for the 256-CU tables, for the coverage table of LABNOTES.md (scripts/partial_trace_reach.py)
struct Reach {
  int64_t t2_items = 0, t4_items = 0;
  int tile_classes = 0, classes_second_trip = 0;  // tile-kernel classes; those with an item whose batch loop takes a second trip
  int max_batches = 0;                            // most trips of the batch loop over one dw group of one item
  int t4_max_bc = 0, nrep4_max_bc = 0;            // most pairs staged at once by a <4,2> item / by an item of a four-wave class
  int max_groups = 0, max_rounds = 0;             // most dw groups one tile item spans; most staging rounds of one batch
  void take(const Reach& o) {
    t2_items += o.t2_items, t4_items += o.t4_items;
    tile_classes = std::max(tile_classes, o.tile_classes), classes_second_trip = std::max(classes_second_trip, o.classes_second_trip);
    max_batches = std::max(max_batches, o.max_batches), t4_max_bc = std::max(t4_max_bc, o.t4_max_bc);
    nrep4_max_bc = std::max(nrep4_max_bc, o.nrep4_max_bc), max_groups = std::max(max_groups, o.max_groups);
    max_rounds = std::max(max_rounds, o.max_rounds);
  }
};
Reach reach_of(const PtHostTables& t) {
  Reach r;
  std::vector<char> second(t.cls.size(), 0), tile(t.cls.size(), 0);
  for (size_t k = (size_t)t.nitems[0]; k < t.items.size(); ++k) {
    const PtItem& it = t.items[k];
    const PtClass& c = t.cls[(size_t)it.cls];
    const bool t4 = k >= (size_t)(t.nitems[0] + t.nitems[1]);
    (t4 ? r.t4_items : r.t2_items) += 1;
    tile[(size_t)it.cls] = 1;
    const int gd0 = it.p0 / c.ngu, gd1 = (it.p1 - 1) / c.ngu;
    r.max_groups = std::max(r.max_groups, gd1 - gd0 + 1);
    for (int gd = gd0; gd <= gd1; ++gd) {
      const int lo = gd == gd0 ? it.p0 - gd0 * c.ngu : 0, hi = gd == gd1 ? it.p1 - gd1 * c.ngu : c.ngu;
      const int nb = (hi - lo + c.batch - 1) / c.batch, bc = std::min(c.batch, hi - lo);
      r.max_batches = std::max(r.max_batches, nb);
      if (nb > 1) second[(size_t)it.cls] = 1;
      if (t4) r.t4_max_bc = std::max(r.t4_max_bc, bc);
      if (c.nrep > 1) r.nrep4_max_bc = std::max(r.nrep4_max_bc, bc);
      r.max_rounds = std::max(r.max_rounds, (bc * c.du + PT_THREADS - 1) / PT_THREADS);
    }
  }
  for (size_t c = 0; c < t.cls.size(); ++c) r.tile_classes += tile[c], r.classes_second_trip += second[c];
  return r;
}

// one SPEC on the sectors of the ranks of one split
void run_case(const std::vector<SectorHost>& ranks, int nimp, const Spec& sp, const std::vector<cd>& psi) {
  const SectorHost& s0 = ranks[0];
  const int nranks = (int)ranks.size();
  const uint32_t S = sp.cluster ? (nimp >= 32 ? 0xffffffffu : (1u << nimp) - 1u) : sp.mask;
  const int nsub = __builtin_popcount(S);
  const int64_t nn = (int64_t)1 << (2 * nsub), words0 = g_words;
  Parity par;
  for (uint32_t m : s0.map_up) par.up.push_back((uint8_t)(sp.fermi ? fermi_parity(m, S) : 0u));
  for (uint32_t m : s0.map_dw) par.dw.push_back((uint8_t)(sp.fermi ? fermi_parity(m, S) : 0u));
  const std::vector<cd> ref = direct(s0, S, nsub, par, psi);
  Totals tot;
  Reach reach;
  for (int ncu : {256, 1}) {
    std::vector<uint8_t> seen((size_t)s0.dimup * s0.dimdw, 0);
    std::vector<cd> rho((size_t)(nn * nn));
    PtHostTables rank0;
    for (const SectorHost& s : ranks) {
      g_case = fmt("%s nranks=%d rank=%d ncu=%d", sp.text.c_str(), nranks, s.rank, ncu);
      PtGroups up, dw;
      std::string e = sp.cluster ? cluster_dm_groups(s, nimp, up, dw) : reduced_dm_groups(s, S, sp.fermi, up, dw);
      REQUIRE(e.empty(), "the group enumeration: %s", e.c_str());
      PtHostTables t;
      e = pt_build(PtSector{nsub, s.nup, s.ndw, s.dimup, s.dimdw, s.nranks, s.cmax, s.qdw, s.dw0}, up, dw, sp.small_n, ncu, "check", t);
      REQUIRE(e.empty(), "pt_build: %s", e.c_str());
      check_rank(s, sp, S, nsub, t, par, psi, s.rank ? &rank0 : nullptr, seen, rho, tot);
      if (s.rank == 0) rank0 = t;
      if (ncu == 256) reach.take(reach_of(t));
    }
    g_case = fmt("%s nranks=%d ncu=%d", sp.text.c_str(), nranks, ncu);
    if (ncu == 256) {  // (before the replay's verdict: the line describes the work list, whatever becomes of the sums)
      printf("REACH spec=%s nranks=%d ncu=256 t2_items=%" PRId64 " t4_items=%" PRId64 " tile_classes=%d classes_second_trip=%d max_batches=%d t4_max_bc=%d nrep4_max_bc=%d max_groups=%d max_rounds=%d\n",
           sp.text.c_str(), nranks, reach.t2_items, reach.t4_items, reach.tile_classes, reach.classes_second_trip, reach.max_batches, reach.t4_max_bc,
           reach.nrep4_max_bc, reach.max_groups, reach.max_rounds);
      fflush(stdout);
    }
    for (size_t k = 0; k < seen.size(); ++k)
      REQUIRE(seen[k] == 1, "(row %zu, column %zu) is named by no pair of any rank", k % (size_t)s0.dimup, k / (size_t)s0.dimup);
    double err = 0, tr = 0;
    for (size_t k = 0; k < ref.size(); ++k) err = std::max(err, std::abs(ref[k] - rho[k]));
    for (int64_t a = 0; a < nn; ++a) tr += rho[(size_t)(a + nn * a)].real();
    REQUIRE(err <= TOL && std::fabs(tr - TRACE) <= TOL, "replay: max |rho(tables) - rho(maps)| = %.3e, trace %.15f", err, tr);
  }
  printf("CASE spec=%s nranks=%d dimup=%d dimdw=%d row_order=%d classes=%" PRId64 " pairs=%" PRId64 " items=%" PRId64 " words_read=%" PRId64 "\n", sp.text.c_str(), nranks,
         s0.dimup, s0.dimdw, (int)s0.row_order(), tot.classes, tot.pairs, tot.items, g_words - words0);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: partial_trace_check MODEL nup ndw RANKS{,RANKS} cluster|MASK:FERMI[:SMALL_N] ...\n");
    return 1;
  }
  ModelFile mf;
  read_model(argv[1], mf);
  const int nup = atoi(argv[2]), ndw = atoi(argv[3]);
  const int nimp = mf.m.nlat * mf.m.norb;
  std::vector<std::vector<SectorHost>> splits;  // the sectors of every rank of every rank count
  for (const char* p = argv[4]; *p; p += strcspn(p, ","), p += *p == ',') {
    const int nranks = atoi(p);
    REQUIRE(nranks >= 1, "bad rank count in %s", argv[4]);
    splits.emplace_back(nranks);
    for (int rank = 0; rank < nranks; ++rank) {
      const std::string e = build_sector_from_model(mf.m, nup, ndw, rank, nranks, splits.back()[rank]);
      REQUIRE(e.empty(), "build_sector_from_model, rank %d of %d: %s", rank, nranks, e.c_str());
    }
  }
  const SectorHost& s0 = splits[0][0];
  std::vector<cd> psi((size_t)s0.dimup * s0.dimdw);
  double nrm = 0;
  for (int j = 0; j < s0.dimdw; ++j)
    for (int i = 0; i < s0.dimup; ++i) nrm += std::norm(psi[(size_t)((int64_t)j * s0.dimup + i)] = amplitude(i, j));
  for (cd& v : psi) v *= std::sqrt(TRACE / nrm);
  for (int a = 5; a < argc; ++a) {
    Spec sp;
    sp.text = argv[a];
    if (sp.text == "cluster")
      sp.cluster = true;
    else {
      unsigned mask = 0;
      int fermi = 0, small_n = K_PAIR_N;
      REQUIRE(sscanf(argv[a], "%x:%d:%d", &mask, &fermi, &small_n) >= 2 && mask && (fermi == 0 || fermi == 1), "bad SPEC %s", argv[a]);
      sp.mask = mask, sp.fermi = fermi, sp.small_n = small_n;
    }
    for (const auto& ranks : splits) run_case(ranks, nimp, sp, psi);
  }
  fflush(stdout);
  return 0;
}
