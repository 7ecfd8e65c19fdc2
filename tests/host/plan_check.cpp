// Stand-alone tile-plan checker ("plan checker").  No HIP runtime call, no device.
//
//   plan_check MODEL nup ndw rank nranks exchange [--panel ROWS] [--dump DIR [--dump-diag]] [--job-reach] [name=value ...] [/ name=value ...] ...
//
// MODEL is a file with the fields of hxv_model in the array order of HxvSector._model_struct (tests/test_host_plan_check.py writes it).
// The sector is built by build_sector_from_model (the halo layout with exchange = 1; the row panel of the all-to-all exchange by
// make_panel_host with --panel), then make_tile_plan runs with an uploader that keeps host copies -- once per option set, the sets are
// separated by a lone "/".  Every table is then read the way the KERNELS read it (hxv_pass_up / hxv_pass_dw of hxv_tiled.hip, the register
// re-packing of hxv_up_job in hxv_jobs.hip): per block, per thread, per slot, through one bounds-checked accessor, and expanded back into
// (row, source, coefficient) triplets.  The triplets of a row must be exactly the stored elements of that row of the sector's one-spin CSR.
// Nothing here calls a helper of the plan builder.
//
// Output: one line "PLAN ..." per accepted option set (the statistics under the names hxv_get_option reports, the number of triplets compared
// and of table words read), one line "REFUSED ..." per set the plan refused with a documented message.
// Exit status: 0 all sets passed; 2 no failure, but a set was refused ("block larger", "does not fit", "must be"); 1 a check failed (the
// first mismatch is printed); abort() from the accessor on an out-of-range table read.
#include <algorithm>
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <string>
#include <vector>

#include "hxv_tiles.hpp"

using namespace hxv;

namespace {

// what the kernels hard-code (hxv_tiles.hpp): restated, the checker uses no name of the builder's, and held equal to the header's
constexpr int K_HOP_CHUNK = 8;                                  // table rows a thread fetches at once
constexpr uint32_t K_OFFM = (1u << TILE_COEF_SHIFT) - 1u;       // offset field of a 32-bit table word
constexpr int K_JOB_KIN = 24, K_JOB_KO = 8, K_JOB_LOADER = 15, K_JOB_MAX_STAGES = 8;
constexpr int K_LDS_BYTES = 160 * 1024;
static_assert(K_HOP_CHUNK == HOP_CHUNK && K_OFFM == TILE_OFF_MASK, "the tile kernels' constants changed");
static_assert(K_JOB_KIN == JOB_KIN && K_JOB_KO == JOB_KO && K_JOB_LOADER == JOB_LOADER && K_JOB_MAX_STAGES == JOB_MAX_STAGES, "the job kernel's constants changed");

std::string fmt(const char* f, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

[[noreturn]] void fail(const std::string& msg) {
  fflush(stdout);
  fprintf(stderr, "plan_check: FAIL: %s\n", msg.c_str());
  exit(1);
}
#define REQUIRE(cond, ...) \
  do {                     \
    if (!(cond)) fail(fmt(__VA_ARGS__)); \
  } while (0)

// ---- the uploader: host copies of exactly the uploaded size, found again by their address --------------------------------------------
struct HostMem {
  std::deque<std::vector<uint32_t>> u32;
  std::deque<std::vector<double2>> d2;
  std::map<const void*, size_t> size;
  PlanUploader uploader() {
    return PlanUploader{[this](const std::vector<uint32_t>& v, uint32_t** p) {
                          u32.emplace_back(v);
                          u32.back().shrink_to_fit();
                          *p = u32.back().data();
                          size[*p] = v.size();
                          return hipSuccess;
                        },
                        [this](const std::vector<double2>& v, double2** p) {
                          d2.emplace_back(v);
                          d2.back().shrink_to_fit();
                          *p = d2.back().data();
                          size[*p] = v.size();
                          return hipSuccess;
                        }};
  }
};

int64_t g_words = 0;  // table words read through the accessor

template <typename T>
struct Tab {
  std::string name;
  const T* p = nullptr;
  size_t n = 0;
  bool present() const { return p != nullptr; }
  T operator[](size_t i) const {
    if (i >= n) {
      fflush(stdout);
      fprintf(stderr, "plan_check: OUT OF RANGE: table %s index %zu size %zu\n", name.c_str(), i, n);
      abort();
    }
    ++g_words;
    return p[i];
  }
};
template <typename T>
Tab<T> table(const HostMem& hm, const char* spin, const char* name, const T* p) {
  Tab<T> t;
  t.name = std::string(name) + "(" + spin + ")";
  t.p = p;
  if (p) {
    auto it = hm.size.find(p);
    REQUIRE(it != hm.size.end(), "table %s was not handed to the uploader", t.name.c_str());
    t.n = it->second;
  }
  return t;
}

// ---- triplets ----------------------------------------------------------------------------------------------------------------------
struct Trip {
  int64_t src;
  double re, im;
  const char* tab;  // where it was decoded from (for the message)
  int64_t idx;
};
bool trip_less(const Trip& a, const Trip& b) {
  if (a.src != b.src) return a.src < b.src;
  if (a.re != b.re) return a.re < b.re;
  return a.im < b.im;
}
using Rows = std::vector<std::vector<Trip>>;

// one spin of the plan and what its kernel sees of the sector
struct Spin {
  const char* name;       // "up" (pass A) / "dw" (pass B)
  bool pass_b;
  const SpinOp* op;       // CSR between the rows this pass works on (device rows for pass A)
  const SpinTiles* t;
  int dim, threads, nscoef;
  Tab<uint32_t> start, tstart, perm, gstart, gmax, ell_in, ell16, bh_ptr, bh, rs_ptr, rs_off, rs_tab, rs_base, rs_neg, rs16, rs16_off, order,
      order_pc;
  Tab<double2> scoef;
  int64_t nsrc;                     // out-of-block sources must be below this (rows of a column / gather slots)
  std::vector<int64_t> slot_col;    // pass B: gather slot -> global column (-1: a pad slot)
  int dw0 = 0, qdw = 0;             // pass B: local columns
  bool local_only = false;          // pass B, halo layout: only local columns see all their sources
};

struct Decoder {
  const Spin& s;
  explicit Decoder(const Spin& sp) : s(sp) {}
  // coefficient ci of the signed table; the LAST entry is the zero of the empty slots
  bool coef(uint32_t ci, bool neg, double& re, double& im) const {
    const double2 c = s.scoef[ci];
    re = neg ? -c.x : c.x;
    im = neg ? -c.y : c.y;
    return (int)ci != s.nscoef - 1;
  }
  // an empty slot is exactly (offset 0, last coefficient entry)
  void empty_rule(uint32_t ci, uint32_t off, const Tab<uint32_t>& tab, size_t idx) const {
    if ((int)ci == s.nscoef - 1) REQUIRE(off == 0, "%s[%zu]: an empty slot must be (offset 0, coefficient %d), offset is %u", tab.name.c_str(), idx, s.nscoef - 1, off);
  }
  int64_t source_of(int64_t gathered, const Tab<uint32_t>& tab, size_t idx, bool live) const {
    REQUIRE(gathered >= 0 && gathered < s.nsrc, "%s[%zu]: out-of-block source %" PRId64 " is not below %" PRId64, tab.name.c_str(), idx, gathered, s.nsrc);
    if (!s.pass_b) return gathered;
    const int64_t c = s.slot_col[(size_t)gathered];
    if (live && !s.local_only) REQUIRE(c >= 0, "%s[%zu]: gather slot %" PRId64 " holds no column", tab.name.c_str(), idx, gathered);
    return c;
  }
};

// Blocks pass B skips: no local output column (hxv_pass_dw returns before it reads a table)
bool block_visited(const Spin& s, int b0, int n) {
  if (!s.pass_b) return true;
  return !(b0 + n <= s.dw0 || b0 >= s.dw0 + s.qdw);
}

// The tile kernels.  half = false: 32-bit words (ell_in, rs_tab); half = true: the half-size copies (ell16 for the in-block hops, rs16 for
// the row slots -- decoded as hxv_pass_up decodes them; whichever copy does not exist falls back to the 32-bit words).
void decode_tile_kernels(const Spin& s, bool half, Rows& rows) {
  const Decoder d(s);
  const SpinTiles& t = *s.t;
  const int dim = s.dim;
  const bool in16 = half && s.ell16.present(), rs16 = half && t.rs16_on;
  const uint32_t p16m = (1u << t.p16_bits) - 1u;
  rows.assign(dim, {});
  for (int kb = 0; kb < t.nblocks; ++kb) {
    const int r0 = (int)s.start[kb], n = (int)s.start[kb + 1] - r0;
    if (!block_visited(s, r0, n)) continue;
    const int tb0 = (int)s.tstart[kb];
    const uint32_t g0 = s.gstart[kb];
    for (int p = 0; p < n; ++p) {  // thread p of the workgroup (the plan guarantees n <= blockDim.x)
      // ---- in-block hops: pass A thread p <-> row r0 + p; pass B thread p <-> sorted position p, column perm[tb0 + p] - tb0
      int out = r0 + p;
      if (s.pass_b) {
        const int c1 = (int)s.perm[tb0 + p] - tb0;
        REQUIRE(c1 >= 0 && c1 < n, "%s[%d]: sorted position leaves its block (%d of %d)", s.perm.name.c_str(), tb0 + p, c1, n);
        out = r0 + c1;
      }
      const int kin = (int)(s.gmax[g0 + (uint32_t)(p >> 6)] & 0xFFFFu);
      for (int k0 = 0; k0 < kin; k0 += K_HOP_CHUNK) {
        uint32_t e[K_HOP_CHUNK];
        size_t at[K_HOP_CHUNK];
        if (in16) {
          for (int u = 0; u < K_HOP_CHUNK / 2; ++u) {
            at[u] = (size_t)(k0 / 2 + u) * dim + tb0 + p;
            e[u] = s.ell16[at[u]];
          }
        } else {
          for (int u = 0; u < K_HOP_CHUNK; ++u) {
            at[u] = (size_t)(k0 + u) * dim + tb0 + p;
            e[u] = s.ell_in[at[u]];
          }
        }
        for (int u = 0; u < K_HOP_CHUNK; ++u) {
          if (k0 + u >= kin) continue;
          uint32_t ci, off;
          size_t where;
          if (in16) {
            const uint32_t hw = (u & 1) ? e[u >> 1] >> 16 : e[u >> 1] & 0xFFFFu;
            ci = hw >> t.p16_bits;
            off = hw & p16m;
            where = at[u >> 1];
          } else {
            ci = e[u] >> TILE_COEF_SHIFT;
            off = e[u] & K_OFFM;
            where = at[u];
          }
          const Tab<uint32_t>& tab = in16 ? s.ell16 : s.ell_in;
          REQUIRE((int)off < n, "%s[%zu]: in-block offset %u is not below the block size %d", tab.name.c_str(), where, off, n);
          d.empty_rule(ci, off, tab, where);
          double re, im;
          if (d.coef(ci, false, re, im)) rows[out].push_back({(int64_t)r0 + off, re, im, in16 ? "ell16" : "ell_in", (int64_t)where});
        }
      }
      // ---- out-of-block hops: lanes along the natural rows / columns of the block
      const int orow = r0 + p;
      for (uint32_t h = s.bh_ptr[kb]; h < s.bh_ptr[kb + 1]; ++h) {
        const uint32_t ci = s.bh[2 * h + 1];
        const int64_t src = d.source_of((int64_t)s.bh[2 * h] + p, s.bh, 2 * h, true);
        double re, im;
        REQUIRE(d.coef(ci, false, re, im), "%s[%u]: a block hop with the zero coefficient", s.bh.name.c_str(), 2 * h + 1);
        rows[orow].push_back({src, re, im, "bh", (int64_t)h});
      }
      const uint32_t rs0 = s.rs_ptr[kb], rs1 = s.rs_ptr[kb + 1];
      if (rs16) {
        for (uint32_t sl = rs0; sl < rs1; sl += 2) {
          const size_t where = (size_t)s.rs16_off[sl] + p;
          const uint32_t w = s.rs16[where];
          for (int hh = 0; hh < 2; ++hh) {
            if (sl + hh >= rs1) continue;
            const uint32_t e = hh ? w >> 16 : w & 0xFFFFu;
            const uint32_t ci = e >> t.p16_bits, off = e & p16m;
            d.empty_rule(ci, off, s.rs16, where);
            double re, im;
            const bool live = d.coef(ci, s.rs_neg[sl + hh] != 0, re, im);
            const int64_t src = d.source_of((int64_t)s.rs_base[sl + hh] + off, s.rs16, where, live);
            if (live) rows[orow].push_back({src, re, im, "rs16/rs_neg/rs_base slot", (int64_t)(sl + hh)});
          }
        }
      } else {
        for (uint32_t sl = rs0; sl < rs1; ++sl) {
          const size_t where = (size_t)s.rs_off[sl] + p;
          const uint32_t e = s.rs_tab[where];
          const uint32_t ci = e >> TILE_COEF_SHIFT, off = e & K_OFFM;
          d.empty_rule(ci, off, s.rs_tab, where);
          double re, im;
          const bool live = d.coef(ci, s.rs_neg[sl] != 0, re, im);
          const int64_t src = d.source_of((int64_t)s.rs_base[sl] + off, s.rs_tab, where, live);
          if (live) rows[orow].push_back({src, re, im, "rs_tab/rs_neg/rs_base slot", (int64_t)sl});
        }
      }
    }
  }
}

// The job kernel of pass A (hxv_up_job): the table words of a row are re-packed once per job into registers,
//   in-block      (coefficient's LDS byte address) << 16 | (source row * 16)
//   out-of-block  (coefficient index) << 23            | (source row of the column * 16)
// and the tile loop decodes THOSE.  Every packed word must give back what went in.
void decode_job_kernel(const Spin& s, int kin_rows, bool real_h, Rows& rows) {
  const Decoder d(s);
  const SpinTiles& t = *s.t;
  const int dim = s.dim, LCB = real_h ? 3 : 4;
  const int KIN = kin_rows <= 20 ? 20 : K_JOB_KIN, KO = K_JOB_KO;
  const uint32_t EMPTY = (uint32_t)(s.nscoef - 1) << TILE_COEF_SHIFT;
  rows.assign(dim, {});
  for (int ob = 0; ob < t.nblocks; ++ob) {
    const int kb = (int)s.order[ob];  // (jobs take their blocks from `order`)
    REQUIRE(kb >= 0 && kb < t.nblocks, "%s[%d] = %d is no block", s.order.name.c_str(), ob, kb);
    const int r0 = (int)s.start[kb], n = (int)s.start[kb + 1] - r0;
    REQUIRE(n <= 64 * K_JOB_LOADER, "job kernel: block %d has %d rows, the compute waves hold %d", kb, n, 64 * K_JOB_LOADER);
    const int tb0 = (int)s.tstart[kb];
    const int rs0 = (int)s.rs_ptr[kb], nrs = (int)s.rs_ptr[kb + 1] - rs0;
    const int bh0 = (int)s.bh_ptr[kb], nbh = (int)s.bh_ptr[kb + 1] - bh0;
    const int nouter = nrs + nbh;
    REQUIRE(nouter <= KO, "job kernel: block %d has %d out-of-block slots, the registers hold %d", kb, nouter, KO);
    for (int p = 0; p < n; ++p) {
      const int pr = p, row = r0 + p;
      uint32_t tin[K_JOB_KIN], tou[K_JOB_KO];
      for (int k = 0; k < KIN; ++k) {
        const size_t where = (size_t)k * dim + tb0 + pr;
        const uint32_t e = k < kin_rows ? s.ell_in[where] : EMPTY;
        tin[k] = ((e >> TILE_COEF_SHIFT) << (16 + LCB)) | ((e & K_OFFM) << 4);
        REQUIRE(((tin[k] >> 16) >> LCB) == (e >> TILE_COEF_SHIFT) && ((tin[k] & 0xFFFFu) >> 4) == (e & K_OFFM),
                "job kernel: %s[%zu] = 0x%08x does not survive the 16-bit fields of the packed in-block word", s.ell_in.name.c_str(), where, e);
      }
      for (int i = 0; i < KO; ++i) {
        uint32_t e = EMPTY;
        if (i < nrs) {
          const size_t where = (size_t)s.rs_off[rs0 + i] + pr;
          e = s.rs_tab[where];
          if (e != EMPTY) {
            const uint64_t off = (uint64_t)(e & K_OFFM) + s.rs_base[rs0 + i];
            REQUIRE(off <= K_OFFM, "job kernel: %s[%zu] + rs_base[%d] = %" PRIu64 " overflows the offset field", s.rs_tab.name.c_str(), where, rs0 + i, off);
            e = ((e ^ (s.rs_neg[rs0 + i] << TILE_COEF_SHIFT)) & ~K_OFFM) | (uint32_t)off;
          }
        } else if (i < nouter) {
          const int h = bh0 + i - nrs;
          const uint64_t off = (uint64_t)s.bh[2 * h] + (uint32_t)pr;
          REQUIRE(off <= K_OFFM, "job kernel: %s[%d] + row overflows the offset field", s.bh.name.c_str(), 2 * h);
          e = (s.bh[2 * h + 1] << TILE_COEF_SHIFT) | (uint32_t)off;
        }
        tou[i] = ((e >> TILE_COEF_SHIFT) << 23) | ((e & K_OFFM) << 4);
        REQUIRE((tou[i] >> 23) == (e >> TILE_COEF_SHIFT) && ((tou[i] & 0x7FFFFFu) >> 4) == (e & K_OFFM),
                "job kernel: out-of-block word 0x%08x of block %d, slot %d, row %d does not survive the 9/23-bit fields", e, kb, i, p);
      }
      const int kin = (int)(s.gmax[s.gstart[kb] + (uint32_t)(p >> 6)] & 0xFFFFu);
      for (int k4 = 0; k4 < KIN; k4 += 4) {
        if (k4 >= kin) continue;
        for (int u = 0; u < 4; ++u) {
          const uint32_t w = tin[k4 + u];
          const uint32_t ca = w >> 16, off = (w & 0xFFFFu) >> 4;
          REQUIRE((int)off < n, "job kernel: in-block offset %u of row %d is not below the block size %d", off, row, n);
          double re, im;
          if (d.coef(ca >> LCB, false, re, im)) rows[row].push_back({(int64_t)r0 + off, re, im, "ell_in (job)", (int64_t)(k4 + u)});
        }
      }
      REQUIRE(kin <= KIN, "job kernel: group bound %d of block %d exceeds the %d register words", kin, kb, KIN);
      for (int i = 0; i < KO; ++i) {
        if (!(i < 4 || i < nouter)) continue;  // (the first four gathers are issued whatever the block has)
        const uint32_t off = (tou[i] & 0x7FFFFFu) >> 4, ci = tou[i] >> 23;
        REQUIRE((int64_t)off < s.nsrc, "job kernel: gather %d of row %d reads row %u of a column of %" PRId64, i, row, off, s.nsrc);
        double re, im;
        if (d.coef(ci, false, re, im)) rows[row].push_back({(int64_t)off, re, im, "rs_tab/rs_neg/rs_base/bh (job) slot", (int64_t)i});
      }
    }
  }
}

// exact comparison, as multisets per row, with the CSR (values compare as IEEE numbers: build_ell merges amplitudes with ==, so the
// sign of a zero imaginary part is not a property of the tables)
int64_t compare_rows(const Spin& s, Rows& rows, const char* what) {
  const SpinOp& op = *s.op;
  const SpinTiles& t = *s.t;
  int64_t compared = 0;
  std::vector<Trip> want;
  for (int kb = 0; kb < t.nblocks; ++kb) {
    const int r0 = (int)t.start[kb], n = (int)t.start[kb + 1] - r0;
    if (!block_visited(s, r0, n)) continue;
    for (int i = r0; i < r0 + n; ++i) {
      if (s.local_only && (i < s.dw0 || i >= s.dw0 + s.qdw)) continue;
      want.clear();
      for (int64_t q = op.rowptr[i]; q < op.rowptr[i + 1]; ++q) want.push_back({op.cols[q], op.vals[q].real(), op.vals[q].imag(), "csr", q});
      std::vector<Trip>& got = rows[i];
      std::sort(want.begin(), want.end(), trip_less);
      std::sort(got.begin(), got.end(), trip_less);
      size_t a = 0;
      for (; a < std::min(want.size(), got.size()); ++a)
        if (want[a].src != got[a].src || want[a].re != got[a].re || want[a].im != got[a].im) break;
      if (a < want.size() || a < got.size()) {
        std::string m = fmt("%s, %s: row %d of block %d: the tables give %zu elements, the CSR stores %zu; first difference at sorted element %zu:", s.name,
                            what, i, kb, got.size(), want.size(), a);
        if (a < got.size()) m += fmt(" tables (source %" PRId64 ", %.17g%+.17gi) decoded from %s %" PRId64 ";", got[a].src, got[a].re, got[a].im, got[a].tab, got[a].idx);
        if (a < want.size()) m += fmt(" CSR (source %" PRId64 ", %.17g%+.17gi)", want[a].src, want[a].re, want[a].im);
        fail(m);
      }
      compared += (int64_t)want.size();
    }
  }
  return compared;
}

// ---- invariants the kernels assume ------------------------------------------------------------------------------------------------------
void check_invariants(const Spin& s) {
  const SpinTiles& t = *s.t;
  const SpinOp& op = *s.op;
  const int dim = s.dim, nb = t.nblocks;
  REQUIRE(nb >= 1 && s.start.n == (size_t)nb + 1 && t.start.size() == (size_t)nb + 1, "start(%s): %zu entries for %d blocks", s.name, s.start.n, nb);
  REQUIRE(s.start[0] == 0 && (int)s.start[nb] == dim, "start(%s) runs from %u to %u, the spin has %d states", s.name, s.start[0], s.start[nb], dim);
  int mx = 0;
  std::vector<int> block_of(dim);
  for (int k = 0; k < nb; ++k) {
    REQUIRE(s.start[k] < s.start[k + 1], "start(%s) is not increasing at block %d", s.name, k);
    REQUIRE(t.start[k] == s.start[k], "start(%s)[%d]: the host copy differs from the uploaded table", s.name, k);
    mx = std::max(mx, (int)(s.start[k + 1] - s.start[k]));
    for (uint32_t i = s.start[k]; i < s.start[k + 1]; ++i) block_of[i] = k;
  }
  REQUIRE(t.max_block == mx, "max_block(%s) = %d, the largest block has %d", s.name, t.max_block, mx);
  REQUIRE(t.max_block <= s.threads, "max_block(%s) = %d exceeds the workgroup of %d threads", s.name, t.max_block, s.threads);
  REQUIRE(t.k_in % K_HOP_CHUNK == 0 && t.k_in >= K_HOP_CHUNK, "k_in(%s) = %d is no multiple of the fetch chunk", s.name, t.k_in);
  REQUIRE(s.ell_in.n == (size_t)t.k_in * dim, "ell_in(%s) has %zu words, k_in x dim = %zu", s.name, s.ell_in.n, (size_t)t.k_in * dim);
  if (s.ell16.present()) REQUIRE(s.ell16.n == (size_t)(t.k_in / 2) * dim && t.p16_bits > 0, "ell16(%s) has %zu words, k_in/2 x dim = %zu", s.name, s.ell16.n, (size_t)(t.k_in / 2) * dim);
  REQUIRE(s.perm.n == (size_t)dim && s.tstart.n == (size_t)nb && s.gstart.n == (size_t)nb + 1, "perm/tstart/gstart(%s): wrong length", s.name);
  // entry counts by block membership
  std::vector<int> cin(dim, 0), cout(dim, 0);
  int64_t n_in = 0, n_out = 0;
  for (int i = 0; i < dim; ++i)
    for (int64_t q = op.rowptr[i]; q < op.rowptr[i + 1]; ++q) (block_of[op.cols[q]] == block_of[i] ? (++n_in, cin[i]) : (++n_out, cout[i]))++;
  REQUIRE(t.n_in == n_in && t.n_out == n_out, "n_in/n_out(%s) = %" PRId64 "/%" PRId64 ", the CSR has %" PRId64 "/%" PRId64, s.name, t.n_in, t.n_out, n_in, n_out);
  REQUIRE(t.k_in_real == *std::max_element(cin.begin(), cin.end()), "k_in_real(%s) = %d is not the longest in-block list", s.name, t.k_in_real);
  // visiting order: a permutation inside every block
  std::vector<char> seen(dim, 0);
  for (int k = 0; k < nb; ++k)
    for (uint32_t q = s.start[k]; q < s.start[k + 1]; ++q) {
      const uint32_t i = s.perm[q];
      REQUIRE(i >= s.start[k] && i < s.start[k + 1] && !seen[i], "perm(%s)[%u] = %u: not a permutation of block %d", s.name, q, i, k);
      seen[i] = 1;
    }
  // shared in-block tables: tstart names the first block of the class, with identical size, order and lists; gstart is aliased likewise
  size_t groups = 0;
  int classes = 0;
  for (int k = 0; k < nb; ++k) {
    const uint32_t nk = s.start[k + 1] - s.start[k], ng = (nk + 63) / 64;
    const uint32_t ts = s.tstart[k];
    int c = -1;
    for (int q = 0; q <= k; ++q)
      if (s.start[q] == ts) c = q;
    REQUIRE(c >= 0, "tstart(%s)[%d] = %u is not the start of a block at or before block %d", s.name, k, ts, k);
    REQUIRE(s.tstart[c] == s.start[c], "tstart(%s)[%d] names block %d, which shares another block's tables itself", s.name, k, c);
    REQUIRE(s.start[c + 1] - s.start[c] == nk, "tstart(%s)[%d]: block %d has %u rows, block %d has %u", s.name, k, c, s.start[c + 1] - s.start[c], k, nk);
    if (c == k) {
      ++classes;
      REQUIRE(s.gstart[k] == groups, "gstart(%s)[%d] = %u, its groups start at %zu", s.name, k, s.gstart[k], groups);
    } else {
      REQUIRE(s.gstart[k] == s.gstart[c], "gstart(%s)[%d] is not aliased to block %d", s.name, k, c);
      for (uint32_t q = 0; q < nk; ++q)
        REQUIRE(s.perm[s.start[k] + q] - s.start[k] == s.perm[ts + q] - ts, "tstart(%s)[%d]: blocks %d and %d visit their rows in different orders", s.name, k, c, k);
      for (int a = 0; a < t.k_in; ++a)
        for (uint32_t q = 0; q < nk; ++q)
          REQUIRE(s.ell_in[(size_t)a * dim + s.start[k] + q] == s.ell_in[(size_t)a * dim + ts + q],
                  "tstart(%s)[%d]: blocks %d and %d share in-block tables that differ at slot %d, position %u", s.name, k, c, k, a, q);
    }
    // the bounds of the 64-position groups: the true maxima (out-of-block half: of the block that owns the words)
    for (uint32_t g = 0; g < ng; ++g) {
      int mi = 0, mo = 0;
      for (uint32_t q = g * 64; q < std::min(nk, g * 64 + 64); ++q) {
        mi = std::max(mi, cin[s.perm[s.start[k] + q]]);
        mo = std::max(mo, cout[s.perm[s.start[k] + q]]);
      }
      const uint32_t w = s.gmax[s.gstart[k] + g];
      REQUIRE((int)(w & 0xFFFFu) == mi, "gmax(%s)[%u]: in-block bound %u, the longest list of group %u of block %d has %d", s.name, s.gstart[k] + g, w & 0xFFFFu, g, k, mi);
      if (c == k) REQUIRE((int)(w >> 16) == mo, "gmax(%s)[%u]: out-of-block bound %u, group %u of block %d has %d", s.name, s.gstart[k] + g, w >> 16, g, k, mo);
    }
    groups += ng;
  }
  REQUIRE(s.gstart[nb] == groups && s.gmax.n == groups, "gmax(%s) has %zu words and gstart ends at %u: the blocks have %zu groups", s.name, s.gmax.n, s.gstart[nb], groups);
  REQUIRE(t.table_classes == classes, "table_classes(%s) = %d, tstart shows %d", s.name, t.table_classes, classes);
  // job / dispatch orders
  for (const Tab<uint32_t>* o : {&s.order, &s.order_pc}) {
    REQUIRE(o->n == (size_t)nb, "%s has %zu entries for %d blocks", o->name.c_str(), o->n, nb);
    std::vector<char> hit(nb, 0);
    for (int k = 0; k < nb; ++k) {
      const uint32_t b = (*o)[k];
      REQUIRE(b < (uint32_t)nb && !hit[b], "%s[%d] = %u: not a permutation of the blocks", o->name.c_str(), k, b);
      hit[b] = 1;
    }
  }
  for (int k = 0; k + 1 < nb; ++k) {
    const uint32_t a = s.order[k], b = s.order[k + 1];
    REQUIRE(s.start[a + 1] - s.start[a] >= s.start[b + 1] - s.start[b], "%s is not largest first at %d", s.order.name.c_str(), k);
  }
  // out-of-block structure
  REQUIRE(s.bh_ptr.n == (size_t)nb + 1 && s.rs_ptr.n == (size_t)nb + 1, "bh_ptr/rs_ptr(%s): wrong length", s.name);
  REQUIRE(s.bh_ptr[0] == 0 && s.rs_ptr[0] == 0, "bh_ptr/rs_ptr(%s) do not start at 0", s.name);
  REQUIRE(s.rs_base.n == s.rs_off.n && s.rs_neg.n == s.rs_off.n && s.rs16_off.n == s.rs_off.n, "rs_off/rs_base/rs_neg/rs16_off(%s) differ in length", s.name);
  int max_outer = 0;
  for (int k = 0; k < nb; ++k) {
    const uint32_t nk = s.start[k + 1] - s.start[k];
    REQUIRE(s.bh_ptr[k] <= s.bh_ptr[k + 1] && s.rs_ptr[k] <= s.rs_ptr[k + 1], "bh_ptr/rs_ptr(%s) decrease at block %d", s.name, k);
    REQUIRE(2 * (size_t)s.bh_ptr[k + 1] <= s.bh.n && s.rs_ptr[k + 1] <= s.rs_off.n, "bh_ptr/rs_ptr(%s)[%d] point past their tables", s.name, k + 1);
    for (uint32_t sl = s.rs_ptr[k]; sl < s.rs_ptr[k + 1]; ++sl) {
      REQUIRE((size_t)s.rs_off[sl] + nk <= s.rs_tab.n, "rs_off(%s)[%u] = %u: a table of %u rows does not fit rs_tab (%zu words)", s.name, sl, s.rs_off[sl], nk, s.rs_tab.n);
      REQUIRE(s.rs_neg[sl] <= 1, "rs_neg(%s)[%u] = %u", s.name, sl, s.rs_neg[sl]);
      if (t.rs16_on && ((sl - s.rs_ptr[k]) & 1) == 0) REQUIRE((size_t)s.rs16_off[sl] + nk <= s.rs16.n, "rs16_off(%s)[%u]: a table of %u rows does not fit rs16", s.name, sl, nk);
    }
    max_outer = std::max(max_outer, (int)(s.bh_ptr[k + 1] - s.bh_ptr[k]) + (int)(s.rs_ptr[k + 1] - s.rs_ptr[k]));
  }
  REQUIRE(t.max_outer == max_outer, "max_outer(%s) = %d, the busiest block has %d row slots + block hops", s.name, t.max_outer, max_outer);
  // the signed coefficients: +c, -c per amplitude, the last entry zero
  REQUIRE(s.scoef.n == (size_t)s.nscoef && s.nscoef == 2 * (int)op.coef.size() + 1 && (int)op.coef.size() <= TILE_MAX_COEF, "scoef(%s): %zu entries for %zu amplitudes", s.name, s.scoef.n, op.coef.size());
  for (size_t i = 0; i < op.coef.size(); ++i) {
    const double2 a = s.scoef[2 * i], b = s.scoef[2 * i + 1];
    REQUIRE(a.x == op.coef[i].real() && a.y == op.coef[i].imag() && b.x == -a.x && b.y == -a.y, "scoef(%s)[%zu]: not +-amplitude %zu", s.name, 2 * i, i);
  }
  const double2 z = s.scoef[(size_t)s.nscoef - 1];
  REQUIRE(z.x == 0.0 && z.y == 0.0, "scoef(%s): the last entry is not zero", s.name);
}

// ---- device row order ---------------------------------------------------------------------------------------------------------------
void check_row_order(const SectorHost& S) {
  const int dim = S.dimup;
  REQUIRE((int)S.up_perm.size() == dim && (int)S.up_iperm.size() == dim && (int)S.up_sign.size() == dim && (int)S.key_up.size() == dim &&
              (int)S.map_up_dev.size() == dim && (int)S.a_up_dev.size() == dim && (int)S.up_pos.size() == S.ns,
          "row order: a table has the wrong length");
  for (int i = 0; i < dim; ++i) {
    const int d = S.up_perm[i];
    REQUIRE(d >= 0 && d < dim && S.up_iperm[d] == i, "up_perm/up_iperm: not inverse permutations at reference row %d", i);
  }
  std::vector<std::pair<int, int>> inv;
  for (int a = 0; a < S.ns; ++a)
    for (int b = a + 1; b < S.ns; ++b)
      if (S.up_pos[a] > S.up_pos[b]) inv.push_back({a, b});
  for (int d = 0; d < dim; ++d) {
    if (d) REQUIRE(S.key_up[d - 1] < S.key_up[d], "key_up does not ascend at device row %d", d);
    const uint32_t m = S.map_up[S.up_iperm[d]];
    uint32_t x = 0;
    int par = 0;
    for (int o = 0; o < S.ns; ++o)
      if ((m >> o) & 1u) x |= 1u << S.up_pos[o];
    for (const auto& pr : inv) par ^= (int)((m >> pr.first) & (m >> pr.second) & 1u);
    REQUIRE(S.key_up[d] == x, "key_up[%d] is not the relabelled configuration of reference row %d", d, S.up_iperm[d]);
    REQUIRE(S.up_sign[d] == par, "up_sign[%d] = %d, the relabelling reverses %d pairs (mod 2)", d, S.up_sign[d], par);
    REQUIRE(S.map_up_dev[d] == m, "map_up_dev[%d] is not map_up of reference row %d", d, S.up_iperm[d]);
    REQUIRE(S.a_up_dev[d] == S.a_up[S.up_iperm[d]], "a_up_dev[%d] is not a_up of reference row %d", d, S.up_iperm[d]);
  }
  // up_dev = S P up P^T S, element by element
  REQUIRE(S.up_dev.dim == dim && S.up_dev.rowptr.size() == (size_t)dim + 1 && S.up_dev.rowptr[dim] == S.up.rowptr[dim], "up_dev: wrong size");
  std::vector<Trip> a, b;
  for (int i = 0; i < dim; ++i) {
    const int di = S.up_perm[i];
    a.clear();
    b.clear();
    for (int64_t q = S.up.rowptr[i]; q < S.up.rowptr[i + 1]; ++q) {
      const int dj = S.up_perm[S.up.cols[q]];
      const double sg = (S.up_sign[di] ^ S.up_sign[dj]) ? -1.0 : 1.0;
      a.push_back({dj, sg * S.up.vals[q].real(), sg * S.up.vals[q].imag(), "", 0});
    }
    for (int64_t q = S.up_dev.rowptr[di]; q < S.up_dev.rowptr[di + 1]; ++q) b.push_back({S.up_dev.cols[q], S.up_dev.vals[q].real(), S.up_dev.vals[q].imag(), "", 0});
    std::sort(a.begin(), a.end(), trip_less);
    std::sort(b.begin(), b.end(), trip_less);
    REQUIRE(a.size() == b.size(), "up_dev: device row %d stores %zu elements, reference row %d stores %zu", di, b.size(), i, a.size());
    for (size_t q = 0; q < a.size(); ++q)
      REQUIRE(a[q].src == b[q].src && a[q].re == b[q].re && a[q].im == b[q].im, "up_dev: device row %d differs from S P up P^T S at its sorted element %zu", di, q);
  }
  if (!S.nd_up.empty()) {
    REQUIRE(S.nd_up_dev.size() == S.nd_up.size(), "nd_up_dev: wrong size");
    const size_t nq = S.nd_up.size() / (size_t)dim;
    for (size_t q = 0; q < nq; ++q)
      for (int i = 0; i < dim; ++i) {
        const uint32_t w = S.nd_up[q * dim + i], got = S.nd_up_dev[q * dim + S.up_perm[i]];
        uint32_t want = ND_INVALID;
        if (w != ND_INVALID) {
          const int di = S.up_perm[i], dj = S.up_perm[(int)(w & 0x7FFFFFFFu)];
          want = (uint32_t)dj | (((w >> 31) ^ S.up_sign[di] ^ S.up_sign[dj]) << 31);
        }
        REQUIRE(got == want, "nd_up_dev: move %zu of device row %d is 0x%08x, the permuted and re-signed reference entry is 0x%08x", q, S.up_perm[i], got, want);
      }
  }
}

// ---- input ------------------------------------------------------------------------------------------------------------------------------
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
  const int64_t L = f.m.nlat, S = f.m.nspin, O = f.m.norb, B = f.m.nbath;
  REQUIRE(L > 0 && S > 0 && O > 0 && B >= 0 && len[0] == 2 * L * L * S * S * O * O && (B == 0 || (len[1] == len[0] * B && len[2] == L * S * O * B)),
          "model file %s: array lengths do not match Nlat/Nspin/Norb/Nbath", path);
  f.m.imphloc = f.h.data();
  f.m.hbath = B > 0 ? f.hb.data() : nullptr;
  f.m.vbath = B > 0 ? f.vb.data() : nullptr;
}

// the TileOptions field behind an option name (hxv_set_option, include/hxv.h group 2)
void set_plan_option(TileOptions& o, const std::string& name, long v) {
  auto is = [&](const char* n) { return name == n; };
  if (is("cols_per_tile")) o.cols_per_tile = (int)v;
  else if (is("rows_per_tile")) o.rows_per_tile = (int)v;
  else if (is("lds_budget_kb")) o.lds_budget_kb_up = o.lds_budget_kb_dw = (int)v;
  else if (is("lds_budget_kb_up")) o.lds_budget_kb_up = (int)v;
  else if (is("lds_budget_kb_dw")) o.lds_budget_kb_dw = (int)v;
  else if (is("tile_bits_up")) o.force_bits_up = (int)v;
  else if (is("tile_bits_dw")) o.force_bits_dw = (int)v;
  else if (is("threads_up")) o.threads_up = (int)v;
  else if (is("threads_dw")) o.threads_dw = (int)v;
  else if (is("sort_mode")) o.sort_mode = (int)v;
  else if (is("sort_mode_dw")) o.sort_mode_dw = (int)v;
  else if (is("wt_cols")) o.wt_cols = (int)v;
  else if (is("spread_banks")) o.spread_banks = v ? 1 : 0;
  else if (is("job_up")) o.job_up = v < 0 ? 0 : (v > 2 ? 2 : (int)v);
  else if (is("job_cols")) o.job_cols = (int)v;
  else if (is("job_groups")) o.job_groups = (int)v;
  else if (is("job_stages")) o.job_stages = (int)v;
  else if (is("job_max_blocks")) o.job_max_blocks = (int)v;
  else if (is("lds_min_kb_up")) o.lds_min_kb_up = (int)v;
  else if (is("lds_min_kb_dw")) o.lds_min_kb_dw = (int)v;
  else if (is("wt_colmajor")) o.wt_colmajor = v ? 1 : 0;
  else if (is("real_dw_pairs")) o.real_dw_pairs = v ? 1 : 0;
  else if (is("pair_rows")) o.pair_rows = (int)v;
  else if (is("block_order")) o.block_order = (int)v;
  else fail("unknown plan option " + name);
}

void dump_raw(const std::string& dir, const char* name, const void* p, size_t bytes) {
  const std::string path = dir + "/" + name;
  FILE* fp = fopen(path.c_str(), "wb");
  REQUIRE(fp != nullptr, "cannot write %s", path.c_str());
  if (bytes) REQUIRE(fwrite(p, 1, bytes, fp) == bytes, "short write to %s", path.c_str());
  fclose(fp);
}
void dump_sector(const SectorHost& S, const std::string& dir) {
  for (int w = 0; w < 2; ++w) {
    const SpinOp& op = w ? S.dw : S.up;
    const std::string pre = w ? "dw_" : "up_";
    dump_raw(dir, (pre + "rowptr.i64").c_str(), op.rowptr.data(), op.rowptr.size() * sizeof(int64_t));
    dump_raw(dir, (pre + "cols.i32").c_str(), op.cols.data(), op.cols.size() * sizeof(int32_t));
    dump_raw(dir, (pre + "vals.c128").c_str(), op.vals.data(), op.vals.size() * sizeof(cplx));
  }
  dump_raw(dir, "map_up.u32", S.map_up.data(), S.map_up.size() * sizeof(uint32_t));
  dump_raw(dir, "map_dw.u32", S.map_dw.data(), S.map_dw.size() * sizeof(uint32_t));
}
// --dump-diag: what hxv_get_diag returns, this rank's DimUp x qdw elements (one double per element: small sectors only)
void dump_diag(const SectorHost& S, const std::string& dir) {
  std::vector<double> d((size_t)S.dimup * (size_t)S.qdw);
  for (int c = 0; c < S.qdw; ++c)
    for (int i = 0; i < S.dimup; ++i) d[(size_t)i + (size_t)c * S.dimup] = host_diag_element(S, i, c + S.dw0);
  dump_raw(dir, "diag.f64", d.data(), d.size() * sizeof(double));
}

// what the kernels and the job predicates see of the sector (hxv_capi.hip, upload_image), without the device pointers
DevSector host_view(const SectorHost& s) {
  DevSector d{};
  d.diag.mode = s.separable_diag ? 0 : 1;
  d.diag.cross = s.cross;
  d.dimup = s.dimup;
  d.dimdw = s.dimdw;
  d.pitch = s.pitch;
  d.qdw = s.qdw;
  d.dw0 = s.dw0;
  d.slab0 = s.exchange == 1 ? 0 : s.rank * s.cmax;
  d.vcol_identity = s.nranks == 1 ? 1 : 0;
  d.nd = s.nd;
  d.real_h = (s.dev_up().real_vals && s.dw.real_vals) ? 1 : 0;
  return d;
}

// --job-reach: one JOBREACH line per usable option set, ahead of its PLAN line: what scripts/job_kernel_reach.py needs to say which paths of
// hxv_up_job the set reaches (per up block: rows : out-of-block slots : in-block bound of each 64-row group)
bool g_job_reach = false;

// one option set: plan, expand, compare.  Returns false when the plan refused the options with a documented message.
bool check_plan(const SectorHost& S, const std::vector<std::pair<std::string, long>>& opts, int set_index) {
  TilePlan plan;
  std::string label;
  for (const auto& kv : opts) {
    if ((kv.first == "lds_min_kb_up" || kv.first == "lds_min_kb_dw") && (kv.second < 0 || kv.second > 160)) {
      printf("REFUSED set=%d lds_min_kb must be in [0,160]\n", set_index);
      return false;
    }
    set_plan_option(plan.opt, kv.first, kv.second);
    label += (label.empty() ? "" : ",") + kv.first + "=" + std::to_string(kv.second);
  }
  HostMem hm;
  const int64_t words0 = g_words;
  const std::string err = make_tile_plan(S, plan, hm.uploader());
  if (!err.empty()) {
    const bool documented = err.find("block larger") != std::string::npos || err.find("does not fit") != std::string::npos || err.find("must be") != std::string::npos;
    if (!documented) fail("make_tile_plan: " + err);
    printf("REFUSED set=%d opts=%s %s\n", set_index, label.c_str(), err.c_str());
    return false;
  }
  if (!plan.usable) {  // more amplitudes than the LDS coefficient table holds: the engine runs kernel 0, there are no tables
    REQUIRE(plan.ncoef_up > TILE_MAX_COEF || plan.ncoef_dw > TILE_MAX_COEF, "plan not usable with %d / %d amplitudes", plan.ncoef_up, plan.ncoef_dw);
    printf("PLAN set=%d opts=%s usable=0\n", set_index, label.c_str());
    return true;
  }
  const DevSector dev = host_view(S);
  Spin sp[2];
  for (int w = 0; w < 2; ++w) {
    Spin& s = sp[w];
    const SpinTiles& t = w ? plan.dw : plan.up;
    s.name = w ? "dw" : "up";
    s.pass_b = w == 1;
    s.op = w ? &S.dw : &S.dev_up();
    s.t = &t;
    s.dim = s.op->dim;
    s.threads = w ? plan.opt.threads_dw : plan.opt.threads_up;
    s.nscoef = 2 * (w ? plan.ncoef_dw : plan.ncoef_up) + 1;
    s.start = table(hm, s.name, "start", t.d_start);
    s.tstart = table(hm, s.name, "tstart", t.d_tstart);
    s.perm = table(hm, s.name, "perm", t.d_perm);
    s.gstart = table(hm, s.name, "gstart", t.d_gstart);
    s.gmax = table(hm, s.name, "gmax", t.d_gmax);
    s.ell_in = table(hm, s.name, "ell_in", t.d_ell_in);
    s.ell16 = table(hm, s.name, "ell16", t.d_ell16);
    s.bh_ptr = table(hm, s.name, "bh_ptr", t.d_bh_ptr);
    s.bh = table(hm, s.name, "bh", t.d_bh);
    s.rs_ptr = table(hm, s.name, "rs_ptr", t.d_rs_ptr);
    s.rs_off = table(hm, s.name, "rs_off", t.d_rs_off);
    s.rs_tab = table(hm, s.name, "rs_tab", t.d_rs_tab);
    s.rs_base = table(hm, s.name, "rs_base", t.d_rs_base);
    s.rs_neg = table(hm, s.name, "rs_neg", t.d_rs_neg);
    s.rs16 = table(hm, s.name, "rs16", t.d_rs16);
    s.rs16_off = table(hm, s.name, "rs16_off", t.d_rs16_off);
    s.order = table(hm, s.name, "order", t.d_order);
    s.order_pc = table(hm, s.name, "order_pc", t.d_order_pc);
    s.scoef = table(hm, s.name, "scoef", w ? plan.d_scoef_dw : plan.d_scoef_up);
    if (!w) {
      s.nsrc = S.dimup;  // pass A gathers rows of its own columns
    } else {
      // pass B gathers column slots of the gathered vector: all-gather layout nranks * cmax slots, halo layout qdw + received columns
      s.nsrc = S.exchange == 1 ? (int64_t)S.qdw + (int64_t)S.halo_cols.size() : (int64_t)S.nranks * S.cmax;
      s.slot_col.assign((size_t)s.nsrc, -1);
      if (S.exchange == 1) {
        for (int c = 0; c < S.qdw; ++c) s.slot_col[c] = S.dw0 + c;
        for (size_t k = 0; k < S.halo_cols.size(); ++k) s.slot_col[(size_t)S.qdw + k] = S.halo_cols[k];
      } else {
        for (int c = 0; c < S.dimdw; ++c) {
          REQUIRE((int64_t)S.vcol[c] < s.nsrc && s.slot_col[S.vcol[c]] < 0, "vcol[%d] = %u: outside the gather layout or taken twice", c, S.vcol[c]);
          s.slot_col[S.vcol[c]] = c;
        }
      }
      for (int c = 0; c < S.dimdw; ++c) REQUIRE((int64_t)S.vcol[c] < s.nsrc, "vcol[%d] = %u is no gather slot (%" PRId64 ")", c, S.vcol[c], s.nsrc);  // (the tile load of pass B)
      for (int c = 0; c < S.qdw; ++c) REQUIRE(s.slot_col[S.vcol[S.dw0 + c]] == S.dw0 + c, "vcol: local column %d is not found at its slot", c);
      s.dw0 = S.dw0;
      s.qdw = S.qdw;
      s.local_only = S.exchange == 1;
    }
  }
  int64_t compared[2] = {0, 0};
  for (int w = 0; w < 2; ++w) {
    const Spin& s = sp[w];
    check_invariants(s);
    Rows r32, r16;
    decode_tile_kernels(s, false, r32);
    compared[w] = compare_rows(s, r32, "32-bit tables");
    if (s.ell16.present() || s.t->rs16_on) {
      decode_tile_kernels(s, true, r16);
      const int64_t c16 = compare_rows(s, r16, "half-size tables");
      REQUIRE(c16 == compared[w], "%s: the half-size tables give %" PRId64 " elements, the 32-bit ones %" PRId64, s.name, c16, compared[w]);
    }
  }
  if (S.panel_rows == 0 && S.nranks == 1) REQUIRE(compared[0] == S.dev_up().rowptr[S.dimup] && compared[1] == S.dw.rowptr[S.dimdw], "not every stored element was compared");
  // the job kernel of pass A
  const bool usable = job_up_usable(dev, plan);
  int job_checked = 0;
  if (usable && S.panel_rows == 0) {
    const int kin_rows = std::min(plan.up.k_in, (plan.up.k_in_real + 3) & ~3);
    Rows rj;
    decode_job_kernel(sp[0], kin_rows, dev.real_h != 0, rj);
    const int64_t cj = compare_rows(sp[0], rj, "job kernel registers");
    REQUIRE(cj == compared[0], "up: the job kernel's registers give %" PRId64 " elements, the tile kernel's tables %" PRId64, cj, compared[0]);
    job_checked = 1;
    // LDS of the tile ring for every scratch width the launcher may ask for, with and without the Lanczos epilogue's second tile
    for (int lz = 0; lz < 2; ++lz)
      for (int wc : {std::max(plan.opt.job_cols, plan.opt.wt_cols), 2, 0}) {
        const int C = plan.opt.job_cols;
        const int ns = (plan.up.max_block + 63) & ~63;
        const int stage = (1 + lz) * C * ns * 16, wtb = ns * std::max(wc, 1) * 16;
        const int tab = (((2 * plan.ncoef_up + 1) * 16 + 255) & ~255) + 256;
        const int nst = std::min(std::min(plan.opt.job_stages, K_JOB_MAX_STAGES), (K_LDS_BYTES - tab - 2 * wtb) / stage);
        const bool fits = job_up_fits(dev, plan, lz != 0, wc);
        const bool mine = nst >= 2 && !(wc > 0 && wc % C != 0);
        REQUIRE(fits == mine, "job_up_fits(lz %d, wc %d) = %d, the ring geometry gives %d stages", lz, wc, (int)fits, nst);
        if (fits) REQUIRE(nst * stage + 2 * wtb + tab <= K_LDS_BYTES, "job ring (lz %d, wc %d): %d bytes of LDS", lz, wc, nst * stage + 2 * wtb + tab);
      }
  }
  if (g_job_reach) {
    const Spin& u = sp[0];
    printf("JOBREACH set=%d usable=%d qdw=%d ncoef_up=%d k_in=%d k_in_real=%d max_outer=%d job_groups=%d job_stages=%d wt_cols=%d blocks=", set_index, (int)usable,
           S.qdw, plan.ncoef_up, plan.up.k_in, plan.up.k_in_real, plan.up.max_outer, plan.opt.job_groups, plan.opt.job_stages, plan.opt.wt_cols);
    for (int kb = 0; kb < plan.up.nblocks; ++kb) {
      const int n = (int)u.start[kb + 1] - (int)u.start[kb];
      printf("%s%d:%d:", kb ? ";" : "", n, (int)(u.rs_ptr[kb + 1] - u.rs_ptr[kb]) + (int)(u.bh_ptr[kb + 1] - u.bh_ptr[kb]));
      for (int g = 0; g < (n + 63) / 64; ++g) printf("%s%d", g ? "/" : "", (int)(u.gmax[u.gstart[kb] + (uint32_t)g] & 0xFFFFu));
    }
    printf("\n");
  }
  const int job_active =
      (plan.opt.job_up == 1 && plan.opt.sort_mode == 0 && usable && job_up_fits(dev, plan, false, std::max(plan.opt.job_cols, plan.opt.wt_cols))) ? 1 : 0;
  printf("PLAN set=%d opts=%s usable=1 tile_bits_up=%d tile_bits_dw=%d nblocks_up=%d nblocks_dw=%d n_in_up=%" PRId64 " n_out_up=%" PRId64 " n_in_dw=%" PRId64
         " n_out_dw=%" PRId64 " k_in_up=%d k_out_up=%d k_in_dw=%d k_out_dw=%d max_block_up=%d max_block_dw=%d max_outer_up=%d max_outer_dw=%d"
         " table_classes_up=%d table_classes_dw=%d job_up_active=%d rows_per_tile=%d row_order=%d job_checked=%d triplets_up=%" PRId64 " triplets_dw=%" PRId64
         " words_read=%" PRId64 "\n",
         set_index, label.c_str(), plan.up.lowbits, plan.dw.lowbits, plan.up.nblocks, plan.dw.nblocks, plan.up.n_in, plan.up.n_out, plan.dw.n_in, plan.dw.n_out,
         plan.up.k_in, plan.up.k_out, plan.dw.k_in, plan.dw.k_out, plan.up.max_block, plan.dw.max_block, plan.up.max_outer, plan.dw.max_outer,
         plan.up.table_classes, plan.dw.table_classes, job_active, plan.opt.rows_per_tile, (int)S.row_order(), job_checked, compared[0], compared[1],
         g_words - words0);
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 7) {
    fprintf(stderr, "usage: plan_check MODEL nup ndw rank nranks exchange [--panel ROWS] [--dump DIR [--dump-diag]] [--job-reach] [name=value ...] [/ name=value ...]\n");
    return 1;
  }
  ModelFile mf;
  read_model(argv[1], mf);
  const int nup = atoi(argv[2]), ndw = atoi(argv[3]), rank = atoi(argv[4]), nranks = atoi(argv[5]), exchange = atoi(argv[6]);
  REQUIRE(exchange >= 0 && exchange <= 2, "exchange must be 0, 1 or 2");
  int panel = 0;
  std::string dump;
  bool with_diag = false;
  std::vector<std::vector<std::pair<std::string, long>>> sets(1);
  for (int a = 7; a < argc; ++a) {
    const std::string arg = argv[a];
    if (arg == "--panel" && a + 1 < argc) panel = atoi(argv[++a]);
    else if (arg == "--dump" && a + 1 < argc) dump = argv[++a];
    else if (arg == "--dump-diag") with_diag = true;
    else if (arg == "--job-reach") g_job_reach = true;
    else if (arg == "/") sets.emplace_back();
    else {
      const size_t eq = arg.find('=');
      REQUIRE(eq != std::string::npos && eq > 0, "argument %s is not name=value", arg.c_str());
      sets.back().push_back({arg.substr(0, eq), atol(arg.c_str() + eq + 1)});
    }
  }
  set_default_exchange(exchange);
  SectorHost main_sector, panel_sector;
  std::string e = build_sector_from_model(mf.m, nup, ndw, rank, nranks, main_sector);
  if (!e.empty()) fail("build_sector_from_model: " + e);
  if (nranks > 1 && exchange == 1) REQUIRE(main_sector.exchange == 1 && (int)main_sector.halo_ptr.size() == nranks + 1, "the halo layout was not made");
  if (!dump.empty()) dump_sector(main_sector, dump);
  if (!dump.empty() && with_diag) dump_diag(main_sector, dump);
  if (main_sector.row_order()) check_row_order(main_sector);
  const SectorHost* S = &main_sector;
  if (panel > 0) {
    e = make_panel_host(main_sector, panel, panel_sector);
    if (!e.empty()) fail("make_panel_host: " + e);
    S = &panel_sector;
  }
  bool refused = false;
  for (size_t k = 0; k < sets.size(); ++k) refused = !check_plan(*S, sets[k], (int)k) || refused;
  fflush(stdout);
  return refused ? 2 : 0;
}
