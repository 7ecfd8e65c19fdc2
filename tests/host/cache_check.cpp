// Stand-alone check of the sector-image cache (csrc/hxv_cache.cpp).  No HIP runtime call, no device: the images it
// inserts own no device allocation, so ~SectorImage returns before its first HIP call.
//
//   cache_check key                    the key holds every input of an open, one mutation at a time (and the mutations change H)
//   cache_check lru [MB]               HXV_SECTOR_CACHE_MB=MB (default 1): LRU order, the byte cap, the counters, image lifetimes, clear
//   cache_check cap MB MIB             HXV_SECTOR_CACHE_MB=MB must act as a cap of MIB whole MiB ("0.5" is 0, "1.9" is 1)
//   cache_check cap0                   = cap 0 0: nothing is ever inserted
//   cache_check disabled               HXV_SECTOR_CACHE=0: every key empty, find counts nothing, insert stores nothing
//   cache_check threads                eight threads of find / insert / stats / clear over a dozen keys (for -fsanitize=thread)
//
// The cap and the on/off switch are read once per process, so every mode is a process of its own and calls setenv before its first call
// into the cache.  Every failed check prints "cache_check: FAIL: ..." on stderr; the last line of stdout is
//   CACHE_CHECK mode=<mode> checks=<n> failures=<n> <OK|FAILED>
// and the exit status is 0 only without a failure.
#include <atomic>
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "hxv_handle.hpp"

using namespace hxv;

// a new field of hxv_model must be looked at here (and in sector_cache_key): 6 int32, 10 doubles, 3 pointers
static_assert(sizeof(hxv_model) == 6 * 4 + 10 * 8 + 3 * sizeof(void*), "hxv_model changed: does sector_cache_key hold the new field? then update this file");
static_assert(sizeof(void*) == 8, "64-bit hosts only");

namespace {

std::atomic<long> g_checks{0}, g_failures{0};

void check(bool ok, const char* f, ...) {
  ++g_checks;
  if (ok) return;
  ++g_failures;
  char buf[1024];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  fprintf(stderr, "cache_check: FAIL: %s\n", buf);
}

struct Stats {
  int64_t entries = -1, bytes = -1, hits = -1, misses = -1;
};
Stats stats() {
  Stats s;
  hxv_sector_cache_stats(&s.entries, &s.bytes, &s.hits, &s.misses);
  return s;
}

// ---- models written here ------------------------------------------------------------------------------------------------------------
struct Owned {
  hxv_model m{};
  std::vector<double> h, hb, vb;
  void bind() {
    m.imphloc = h.data();
    m.hbath = m.nbath > 0 ? hb.data() : nullptr;
    m.vbath = m.nbath > 0 ? vb.data() : nullptr;
  }
  Owned() = default;
  Owned(const Owned& o) : m(o.m), h(o.h), hb(o.hb), vb(o.vb) { bind(); }
  Owned& operator=(const Owned& o) {
    m = o.m; h = o.h; hb = o.hb; vb = o.vb;
    bind();
    return *this;
  }
  size_t nloc() const { return (size_t)m.nlat * m.nlat * m.nspin * m.nspin * m.norb * m.norb; }
};

// index of element (il,jl,is,js,io,jo[,ib]) in the reference's Fortran order, in complex elements
size_t i6(const hxv_model& m, int il, int jl, int is, int js, int io, int jo, int ib = 0) {
  const size_t L = m.nlat, S = m.nspin, O = m.norb;
  return il + L * (jl + L * (is + S * (js + S * (io + O * jo)))) + L * L * S * S * O * O * (size_t)ib;
}

// Hermitian one-body blocks on the spin diagonal: distinct on-site energies, a hop between every pair of (site, orbital), complex if asked
void fill_blocks(Owned& o, std::vector<double>& a, int ib, double scale, bool cmplx) {
  const hxv_model& m = o.m;
  for (int s = 0; s < m.nspin; ++s)
    for (int il = 0; il < m.nlat; ++il)
      for (int jl = 0; jl < m.nlat; ++jl)
        for (int io = 0; io < m.norb; ++io)
          for (int jo = 0; jo < m.norb; ++jo) {
            const int p = io + il * m.norb, q = jo + jl * m.norb;
            const size_t k = i6(m, il, jl, s, s, io, jo, ib);
            if (p == q) {
              a[2 * k] = scale * (0.1 + 0.07 * p - 0.05 * s + 0.03 * ib);
            } else {
              const int lo = p < q ? p : q, hi = p < q ? q : p;
              a[2 * k] = -scale * (0.25 + 0.01 * lo + 0.02 * hi + 0.005 * s);
              if (cmplx) a[2 * k + 1] = (p < q ? 1.0 : -1.0) * scale * (0.15 + 0.01 * hi + 0.004 * s);
            }
          }
}

Owned make_model(int nlat, int norb, int nspin, int nbath, bool cmplx) {
  Owned o;
  hxv_model& m = o.m;
  m.nlat = nlat; m.norb = norb; m.nspin = nspin; m.nbath = nbath;
  m.hfmode = 1;
  m.reserved = 0;
  const double u[5] = {2.0, 1.5, 1.25, 1.125, 0.75};
  for (int i = 0; i < 5; ++i) m.uloc[i] = u[i];
  m.ust = 0.4; m.jh = 0.1; m.jx = 0.25; m.jp = -0.1; m.xmu = 0.3;
  o.h.assign(2 * o.nloc(), 0.0);
  o.hb.assign(2 * o.nloc() * (size_t)nbath, 0.0);
  o.vb.assign((size_t)nlat * nspin * norb * nbath, 0.0);
  fill_blocks(o, o.h, 0, 1.0, cmplx);
  for (int ib = 0; ib < nbath; ++ib) fill_blocks(o, o.hb, ib, 0.5, cmplx);
  for (size_t k = 0; k < o.vb.size(); ++k) o.vb[k] = 0.5 + 0.03 * (double)k;
  o.bind();
  return o;
}

struct Sector {
  int nup, ndw, rank, nranks, device, exchange;
};
std::string key_of(const Owned& o, const Sector& s) { return sector_cache_key(o.m, s.nup, s.ndw, s.rank, s.nranks, s.device, s.exchange); }

// ---- is a mutation of the model a mutation of H? --------------------------------------------------------------------------------------
struct HostH {
  bool ok = false;
  std::vector<cplx> up, dw;
  std::vector<int32_t> upc, dwc;
  std::vector<double> diag;
  double jx = 0, jp = 0;
  int nd = 0;
  bool operator==(const HostH& b) const { return up == b.up && dw == b.dw && upc == b.upc && dwc == b.dwc && diag == b.diag && jx == b.jx && jp == b.jp && nd == b.nd; }
};
HostH host_h(const Owned& o, int nup, int ndw) {
  HostH r;
  SectorHost s;
  const std::string e = build_sector_from_model(o.m, nup, ndw, 0, 1, s);
  if (!e.empty()) {
    fprintf(stderr, "cache_check: build_sector_from_model: %s\n", e.c_str());
    return r;
  }
  r.ok = true;
  r.up = s.up.vals; r.dw = s.dw.vals; r.upc = s.up.cols; r.dwc = s.dw.cols;
  r.diag.reserve((size_t)s.dim);
  for (int c = 0; c < s.dimdw; ++c)
    for (int i = 0; i < s.dimup; ++i) r.diag.push_back(host_diag_element(s, i, c));
  r.jx = s.nd.jx; r.jp = s.nd.jp; r.nd = s.nd.active;
  return r;
}

void set_or_unset(const char* name, const char* value) {
  if (value)
    setenv(name, value, 1);
  else
    unsetenv(name);
}

// ---- mode "key" -------------------------------------------------------------------------------------------------------------------------
void key_one_model(const char* name, const Owned& base, const Sector& sec) {
  const std::string k0 = key_of(base, sec);
  check(!k0.empty(), "%s: the base key is empty", name);
  const HostH h0 = host_h(base, sec.nup, sec.ndw);
  check(h0.ok, "%s: the base sector does not build", name);
  // `enters`: the mutant must also be another host description (the mutation is not vacuous)
  auto differs = [&](const Owned& mut, const char* what, bool enters) {
    const std::string k = key_of(mut, sec);
    check(!k.empty() && k != k0, "%s: a changed %s leaves the key unchanged", name, what);
    if (enters) {
      const HostH h = host_h(mut, sec.nup, sec.ndw);
      check(h.ok && !(h == h0), "%s: a changed %s does not change the host description: the mutation is vacuous", name, what);
    }
  };
  const hxv_model& b = base.m;
  char what[128];
  // scalar fields
  {
    // another Nlat / Norb / Nspin / Nbath, with arrays of the matching sizes
    for (int f = 0; f < 4; ++f) {
      int d[4] = {b.nlat, b.norb, b.nspin, b.nbath};
      if (f == 2)
        d[2] = 3 - d[2];
      else
        d[f] += 1;
      Owned mut = make_model(d[0], d[1], d[2], d[3], true);
      const char* fn[4] = {"nlat", "norb", "nspin", "nbath"};
      differs(mut, fn[f], false);
    }
    // the same array bytes read as (Nlat, Norb) = (Norb, Nlat): nothing but the two scalars differs (skipped where they are equal)
    if (b.nlat != b.norb) {
      Owned mut = base;
      std::swap(mut.m.nlat, mut.m.norb);
      differs(mut, "nlat <-> norb over the same bytes", false);
    }
    Owned mut = base;
    mut.m.hfmode = !b.hfmode;
    differs(mut, "hfmode", true);
    for (int i = 0; i < 5; ++i) {
      mut = base;
      mut.m.uloc[i] += 0.125;
      snprintf(what, sizeof what, "uloc[%d]", i);
      differs(mut, what, i < b.norb);
    }
    mut = base; mut.m.ust += 0.125; differs(mut, "ust", b.norb > 1);
    mut = base; mut.m.jh += 0.125; differs(mut, "jh", b.norb > 1);
    mut = base; mut.m.jx += 0.125; differs(mut, "jx", b.norb > 1);
    mut = base; mut.m.jp += 0.125; differs(mut, "jp", b.norb > 1);
    mut = base; mut.m.xmu += 0.125; differs(mut, "xmu", true);
  }
  // every element of the three arrays, real and imaginary parts separately.  The builder reads the spin-diagonal blocks; the imaginary
  // part of a diagonal element is refused in impHloc and ignored in Hbath (bath_diag = DREAL), so those enter the key only.
  {
    const size_t nloc = base.nloc();
    auto block = [&](size_t k, bool& spin_diag, bool& orb_diag) {  // k: complex index inside one replica
      const size_t L = b.nlat, S = b.nspin, O = b.norb;
      const size_t il = k % L, jl = (k / L) % L, is = (k / (L * L)) % S, js = (k / (L * L * S)) % S, io = (k / (L * L * S * S)) % O, jo = k / (L * L * S * S * O);
      spin_diag = is == js;
      orb_diag = il == jl && io == jo;
    };
    for (size_t i = 0; i < base.h.size(); ++i) {
      Owned mut = base;
      mut.h[i] += 0.125;
      bool sd, od;
      block((i / 2) % nloc, sd, od);
      snprintf(what, sizeof what, "imphloc[%zu] (of %zu doubles)", i, base.h.size());
      differs(mut, what, sd && !(od && (i & 1)));
    }
    for (size_t i = 0; i < base.hb.size(); ++i) {
      Owned mut = base;
      mut.hb[i] += 0.125;
      bool sd, od;
      block((i / 2) % nloc, sd, od);
      snprintf(what, sizeof what, "hbath[%zu] (of %zu doubles)", i, base.hb.size());
      differs(mut, what, sd && !(od && (i & 1)));
    }
    for (size_t i = 0; i < base.vb.size(); ++i) {
      Owned mut = base;
      mut.vb[i] += 0.125;
      snprintf(what, sizeof what, "vbath[%zu] (of %zu doubles)", i, base.vb.size());
      differs(mut, what, true);
    }
  }
  // the sector, the split, the device, the exchange
  {
    const char* fn[6] = {"nup", "ndw", "rank", "nranks", "device", "exchange"};
    for (int f = 0; f < 6; ++f) {
      Sector s = sec;
      int* p[6] = {&s.nup, &s.ndw, &s.rank, &s.nranks, &s.device, &s.exchange};
      *p[f] += 1;
      const std::string k = key_of(base, s);
      check(!k.empty() && k != k0, "%s: a changed %s leaves the key unchanged", name, fn[f]);
    }
    Sector s = sec;
    std::swap(s.nup, s.ndw);
    check(s.nup == s.ndw || key_of(base, s) != k0, "%s: (ndw,nup) has the key of (nup,ndw)", name);
    s = sec;
    std::swap(s.rank, s.nranks);
    check(key_of(base, s) != k0, "%s: rank <-> nranks leaves the key unchanged", name);
  }
  // the environment hooks of the device row order: unset, set, set to something else, set but empty (atoi reads that as 0: not the default)
  {
    struct Hook {
      const char* name;
      const char* a;
      const char* b;
    };
    const Hook hooks[3] = {{"HXV_ROW_ORDER", "0", nullptr}, {"HXV_ROW_ORDER_MIN_DIMUP", "16", "32"}, {"HXV_ROW_ORDER_BITS", "8", "6"}};
    for (const Hook& hk : hooks) {
      unsetenv(hk.name);
      check(key_of(base, sec) == k0, "%s: the base key depends on something else than its inputs", name);
      setenv(hk.name, hk.a, 1);
      const std::string ka = key_of(base, sec);
      check(!ka.empty() && ka != k0, "%s: %s=%s has the key of the unset variable", name, hk.name, hk.a);
      if (hk.b) {
        setenv(hk.name, hk.b, 1);
        const std::string kb = key_of(base, sec);
        check(kb != k0 && kb != ka, "%s: %s=%s has the key of %s or of the unset variable", name, hk.name, hk.b, hk.a);
        setenv(hk.name, "", 1);
        check(key_of(base, sec) != k0, "%s: %s set but empty has the key of the unset variable", name, hk.name);
      }
      unsetenv(hk.name);
      check(key_of(base, sec) == k0, "%s: unsetting %s does not bring the base key back", name, hk.name);
    }
    // two hooks must not be able to stand in for each other
    setenv("HXV_ROW_ORDER_MIN_DIMUP", "8", 1);
    const std::string k1 = key_of(base, sec);
    unsetenv("HXV_ROW_ORDER_MIN_DIMUP");
    setenv("HXV_ROW_ORDER_BITS", "8", 1);
    const std::string k2 = key_of(base, sec);
    unsetenv("HXV_ROW_ORDER_BITS");
    check(k1 != k2, "%s: HXV_ROW_ORDER_MIN_DIMUP=8 and HXV_ROW_ORDER_BITS=8 give one key", name);
  }
  // what must NOT change the key
  {
    Owned copy = base;  // the same bytes at other addresses
    check(copy.h.data() != base.h.data(), "%s: the copy shares its arrays", name);
    check(key_of(copy, sec) == k0, "%s: the same model bytes at other addresses give another key", name);
    copy.m.reserved = 12345;
    check(key_of(copy, sec) == k0, "%s: `reserved` enters the key", name);
  }
  // every argument combination the two guards refuse
  {
    auto refused = [&](const Owned& mut, const char* why) { check(key_of(mut, sec).empty(), "%s: %s gives a key", name, why); };
    Owned mut = base;
    mut.m.nlat = 0; refused(mut, "nlat = 0");
    mut = base; mut.m.nlat = 17; refused(mut, "nlat = 17");
    mut = base; mut.m.norb = 0; refused(mut, "norb = 0");
    mut = base; mut.m.norb = 6; refused(mut, "norb = 6");
    mut = base; mut.m.nspin = 0; refused(mut, "nspin = 0");
    mut = base; mut.m.nspin = 3; refused(mut, "nspin = 3");
    mut = base; mut.m.nbath = -1; refused(mut, "nbath = -1");
    mut = base; mut.m.imphloc = nullptr; refused(mut, "imphloc = NULL");
    if (b.nbath > 0) {
      mut = base; mut.m.hbath = nullptr; refused(mut, "hbath = NULL with a bath");
      mut = base; mut.m.vbath = nullptr; refused(mut, "vbath = NULL with a bath");
    } else {
      check(b.hbath == nullptr && b.vbath == nullptr && !k0.empty(), "%s: no bath, NULL bath arrays: must be keyed", name);
    }
  }
}

void mode_key() {
  for (const char* n : {"HXV_ROW_ORDER", "HXV_ROW_ORDER_MIN_DIMUP", "HXV_ROW_ORDER_BITS", "HXV_EXCHANGE", "HXV_SECTOR_CACHE"}) unsetenv(n);
  key_one_model("real Norb 1 with a bath", make_model(2, 1, 1, 2, false), Sector{3, 2, 0, 1, 0, 0});   // Ns 6
  key_one_model("complex Nspin 2 Norb 2 with a bath", make_model(2, 2, 2, 1, true), Sector{4, 3, 0, 1, 0, 0});  // Ns 8
  key_one_model("no bath", make_model(3, 1, 1, 0, false), Sector{2, 1, 0, 1, 0, 0});                  // Ns 3
  // HXV_EXCHANGE enters through the `exchange` argument: hxv_create_from_model passes default_exchange() for a split sector
  const Owned base = make_model(2, 1, 1, 2, false);
  std::string k[3];
  const char* val[3] = {nullptr, "halo", "alltoall"};
  for (int e = 0; e < 3; ++e) {
    set_or_unset("HXV_EXCHANGE", val[e]);
    check(default_exchange() == e, "HXV_EXCHANGE=%s: default_exchange() = %d", val[e] ? val[e] : "(unset)", default_exchange());
    k[e] = sector_cache_key(base.m, 3, 2, 1, 2, 0, default_exchange());
  }
  unsetenv("HXV_EXCHANGE");
  check(!k[0].empty() && k[0] != k[1] && k[0] != k[2] && k[1] != k[2], "the three values of HXV_EXCHANGE do not give three keys");
  for (int e = 0; e < 3; ++e) {
    set_default_exchange(e);
    check(default_exchange() == e && sector_cache_key(base.m, 3, 2, 1, 2, 0, default_exchange()) == k[e], "set_default_exchange(%d) does not give the key of the variable", e);
  }
}

// ---- images without a device ------------------------------------------------------------------------------------------------------------
std::shared_ptr<SectorImage> image(const std::string& key, int64_t host_bytes) {
  auto im = std::make_shared<SectorImage>();
  im->key = key;
  im->host_bytes = host_bytes;
  im->uploaded = true;
  return im;
}

// what the cache must hold: the same policy written down again, most recently used first
struct Model {
  int64_t cap;
  std::list<std::pair<std::string, int64_t>> lru;
  int64_t hits = 0, misses = 0;
  int64_t bytes() const {
    int64_t b = 0;
    for (auto& e : lru) b += e.second;
    return b;
  }
  bool has(const std::string& k) const {
    for (auto& e : lru)
      if (e.first == k) return true;
    return false;
  }
  bool find(const std::string& k) {
    for (auto it = lru.begin(); it != lru.end(); ++it)
      if (it->first == k) {
        lru.splice(lru.begin(), lru, it);
        ++hits;
        return true;
      }
    ++misses;
    return false;
  }
  void insert(const std::string& k, int64_t b) {
    if (has(k) || b > cap) return;
    lru.emplace_front(k, b);
    while (bytes() > cap && lru.size() > 1) lru.pop_back();
  }
  void agree(const char* step) const {
    const Stats s = stats();
    check(s.entries == (int64_t)lru.size() && s.bytes == bytes() && s.hits == hits && s.misses == misses,
          "%s: the cache reports entries %" PRId64 " bytes %" PRId64 " hits %" PRId64 " misses %" PRId64 ", expected %zu %" PRId64 " %" PRId64 " %" PRId64, step,
          s.entries, s.bytes, s.hits, s.misses, lru.size(), bytes(), hits, misses);
  }
};

// ---- mode "lru" -------------------------------------------------------------------------------------------------------------------------
void mode_lru(const char* mb) {
  setenv("HXV_SECTOR_CACHE_MB", mb, 1);
  unsetenv("HXV_SECTOR_CACHE");
  const int64_t KiB = 1024;
  Model md{(int64_t)1 << 20};
  md.agree("start");
  auto a = image("A", 400 * KiB), b = image("B", 400 * KiB), d = image("D", 400 * KiB);
  b->device_bytes = 100 * KiB;  // (host + device bytes count)
  b->host_bytes = 300 * KiB;
  std::weak_ptr<SectorImage> wa = a, wb = b, wc, wd = d;
  sector_cache_insert(a); md.insert("A", 400 * KiB); md.agree("insert A");
  sector_cache_insert(b); md.insert("B", 400 * KiB); md.agree("insert B");
  check(sector_cache_find("") == nullptr, "an empty key finds something");
  md.agree("find of the empty key (counts nothing)");
  // beyond the cap: the least recently used (A) goes; nobody outside holds C
  {
    auto cc = image("C", 400 * KiB);
    wc = cc;
    sector_cache_insert(cc);
  }
  md.insert("C", 400 * KiB); md.agree("insert C beyond the cap");
  check(!md.has("A") && md.has("B") && md.has("C"), "the restated policy is wrong");
  check(!wc.expired(), "C is held by the cache and is gone");
  check(!wa.expired() && wa.use_count() == 1, "A was dropped while held outside: use count %ld, expected 1", wa.use_count());
  a.reset();
  check(wa.expired(), "A was dropped and released and is still alive");
  check(sector_cache_find("A") == nullptr, "A is found after its eviction"); md.find("A"); md.agree("find A (miss)");
  // a find refreshes: B becomes the most recent, so D pushes C out, not B
  check(sector_cache_find("B") == b, "B is not found, or is another image"); md.find("B"); md.agree("find B (hit)");
  sector_cache_insert(d); md.insert("D", 400 * KiB); md.agree("insert D");
  check(md.has("B") && md.has("D") && !md.has("C"), "the restated policy is wrong");
  check(wc.expired(), "C was dropped with no holder outside and is still alive");
  check(sector_cache_find("C") == nullptr, "C is found after its eviction"); md.find("C"); md.agree("find C (miss)");
  // a duplicate key is ignored: the first image stays
  auto b2 = image("B", 100 * KiB);
  sector_cache_insert(b2); md.insert("B", 100 * KiB); md.agree("insert a second image of key B");
  check(sector_cache_find("B") == b, "the duplicate replaced the image of key B"); md.find("B"); md.agree("find B again");
  // larger than the cap: not inserted, nothing evicted
  auto big = image("BIG", md.cap + 1);
  sector_cache_insert(big); md.insert("BIG", md.cap + 1); md.agree("insert an image larger than the cap");
  check(sector_cache_find("BIG") == nullptr, "an image larger than the cap was inserted"); md.find("BIG"); md.agree("find BIG (miss)");
  check(!wb.expired() && !wd.expired(), "the refused image evicted something");
  // not uploaded, no key, null: never stored
  auto raw = image("RAW", KiB);
  raw->uploaded = false;
  sector_cache_insert(raw);
  sector_cache_insert(image("", KiB));
  sector_cache_insert(nullptr);
  md.agree("inserts of a not-uploaded image, a keyless image and a null pointer");
  // exactly the cap: inserted, and everything else goes
  auto full = image("FULL", md.cap);
  sector_cache_insert(full); md.insert("FULL", md.cap); md.agree("insert an image of exactly the cap");
  check(md.lru.size() == 1, "the restated policy is wrong");
  check(!wb.expired() && !wd.expired(), "B and D are held outside and died with their eviction");
  b.reset();
  d.reset();
  check(wb.expired() && wd.expired(), "B and D were dropped and released and are still alive");
  // clear: entries and bytes go, the counters stay, a held image lives on
  std::weak_ptr<SectorImage> wfull = full;
  hxv_sector_cache_clear(); md.lru.clear(); md.agree("clear");
  check(!wfull.expired() && wfull.use_count() == 1, "clear killed or kept an image held outside: use count %ld", wfull.use_count());
  full.reset();
  check(wfull.expired(), "FULL outlives its last holder");
  {
    auto e = image("E", 10 * KiB);
    std::weak_ptr<SectorImage> we = e;
    sector_cache_insert(e); md.insert("E", 10 * KiB);
    e.reset();
    check(!we.expired(), "the cache does not hold E");
    hxv_sector_cache_clear(); md.lru.clear(); md.agree("clear with an image nobody else holds");
    check(we.expired(), "clear left an image alive that nobody holds");
  }
  // a seeded random walk against the restated policy: 16 keys of 50..350 KiB, the image of a key always the same size
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&] {
    rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
    return rng;
  };
  for (int step = 0; step < 4000; ++step) {
    const int k = (int)(next() % 16);
    const std::string key = "W" + std::to_string(k);
    const int64_t bytes = (50 + 20 * k) * KiB;
    const int op = (int)(next() % 100);
    if (op < 50) {
      const bool got = sector_cache_find(key) != nullptr, want = md.find(key);
      check(got == want, "walk step %d: find(%s) = %d, expected %d", step, key.c_str(), (int)got, (int)want);
    } else if (op < 99) {
      sector_cache_insert(image(key, bytes));
      md.insert(key, bytes);
    } else {
      hxv_sector_cache_clear();
      md.lru.clear();
    }
    md.agree("walk");
    if (g_failures) return;
  }
}

// ---- modes "cap" / "cap0" ---------------------------------------------------------------------------------------------------------------
void mode_cap(const char* mb, int64_t mib) {
  setenv("HXV_SECTOR_CACHE_MB", mb, 1);
  unsetenv("HXV_SECTOR_CACHE");
  const int64_t cap = mib << 20;
  Model md{cap};
  for (int64_t bytes : {(int64_t)1, (int64_t)4096, cap / 2 + 1, cap - 1, cap, cap + 1, (cap + 1) * 2, (int64_t)1 << 30}) {
    if (bytes < 1) continue;
    const std::string key = "S" + std::to_string(bytes);
    sector_cache_insert(image(key, bytes));
    md.insert(key, bytes);
    md.agree(("HXV_SECTOR_CACHE_MB=" + std::string(mb) + ", insert of " + std::to_string(bytes) + " bytes").c_str());
    const bool got = sector_cache_find(key) != nullptr, want = md.find(key);
    check(got == want && want == (bytes <= cap), "HXV_SECTOR_CACHE_MB=%s: an image of %" PRId64 " bytes is %sstored (cap %" PRId64 " MiB)", mb, bytes, got ? "" : "not ", mib);
    const Stats s = stats();
    check(s.bytes <= cap, "HXV_SECTOR_CACHE_MB=%s: %" PRId64 " bytes cached", mb, s.bytes);
    if (cap == 0) check(s.entries == 0 && s.bytes == 0 && s.hits == 0, "HXV_SECTOR_CACHE_MB=%s: something was inserted", mb);
  }
}

// ---- mode "disabled" --------------------------------------------------------------------------------------------------------------------
void mode_disabled() {
  setenv("HXV_SECTOR_CACHE", "0", 1);
  unsetenv("HXV_SECTOR_CACHE_MB");
  const Owned ms[3] = {make_model(2, 1, 1, 2, false), make_model(2, 2, 2, 1, true), make_model(3, 1, 1, 0, false)};
  for (const Owned& o : ms) {
    for (int nranks = 1; nranks <= 2; ++nranks) {
      const std::string k = sector_cache_key(o.m, 2, 1, 0, nranks, 0, 0);
      check(k.empty(), "HXV_SECTOR_CACHE=0: a key of %zu bytes", k.size());
      check(sector_cache_find(k) == nullptr, "HXV_SECTOR_CACHE=0: find returns an image");
      sector_cache_insert(image(k, 1024));
      check(sector_cache_find(k) == nullptr, "HXV_SECTOR_CACHE=0: an image was stored");
      const Stats s = stats();
      check(s.entries == 0 && s.bytes == 0 && s.hits == 0 && s.misses == 0, "HXV_SECTOR_CACHE=0: entries %" PRId64 " bytes %" PRId64 " hits %" PRId64 " misses %" PRId64,
            s.entries, s.bytes, s.hits, s.misses);
    }
  }
  hxv_sector_cache_clear();
  const Stats s = stats();
  check(s.entries == 0 && s.bytes == 0 && s.hits == 0 && s.misses == 0, "HXV_SECTOR_CACHE=0: the counters moved");
}

// ---- mode "threads" ---------------------------------------------------------------------------------------------------------------------
void mode_threads() {
  setenv("HXV_SECTOR_CACHE_MB", "1", 1);  // (small enough that inserts evict)
  unsetenv("HXV_SECTOR_CACHE");
  constexpr int NT = 8, NK = 12, ROUNDS = 3000;
  const int64_t cap = (int64_t)1 << 20;
  auto bytes_of = [](int k) { return (int64_t)(60 + 15 * k) * 1024; };
  std::atomic<long> finds{0}, found{0}, inserts{0}, clears{0}, bad{0};
  std::vector<std::thread> ths;
  for (int t = 0; t < NT; ++t)
    ths.emplace_back([&, t] {
      uint64_t rng = 0xD1B54A32D192ED03ull * (uint64_t)(t + 1);
      auto next = [&] {
        rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
        return rng;
      };
      for (int r = 0; r < ROUNDS; ++r) {
        const int k = (int)(next() % NK);
        const std::string key = "T" + std::to_string(k);
        std::shared_ptr<SectorImage> im = sector_cache_find(key);
        ++finds;
        if (im) {
          ++found;
          if (im->key != key || im->host_bytes != bytes_of(k)) ++bad;  // (an image is immutable: reading it beside the other threads is the use)
        } else {
          sector_cache_insert(image(key, bytes_of(k)));
          ++inserts;
        }
        const Stats s = stats();
        if (s.bytes < 0 || s.bytes > cap || s.entries < 0 || s.entries > NK) ++bad;
        if (next() % 700 == 0) {
          hxv_sector_cache_clear();
          ++clears;
        }
      }
    });
  for (auto& th : ths) th.join();
  check(bad == 0, "%ld reads of a wrong image or of impossible statistics", bad.load());
  const Stats s = stats();
  check(s.hits == found && s.hits + s.misses == finds, "hits %" PRId64 " misses %" PRId64 ", the threads counted %ld finds, %ld of them hits", s.hits, s.misses, finds.load(), found.load());
  // bytes = the sum over the entries: every key is probed once
  int64_t sum = 0, n = 0;
  for (int k = 0; k < NK; ++k)
    if (auto im = sector_cache_find("T" + std::to_string(k))) {
      sum += im->host_bytes + im->device_bytes;
      ++n;
    }
  check(s.entries == n && s.bytes == sum && sum <= cap, "entries %" PRId64 " bytes %" PRId64 " at the end, the probes found %" PRId64 " images of %" PRId64 " bytes", s.entries, s.bytes, n, sum);
  printf("threads: %ld finds (%ld hits), %ld inserts, %ld clears\n", finds.load(), found.load(), inserts.load(), clears.load());
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "key")
    mode_key();
  else if (mode == "lru")
    mode_lru(argc > 2 ? argv[2] : "1");
  else if (mode == "cap0")
    mode_cap("0", 0);
  else if (mode == "cap" && argc > 3)
    mode_cap(argv[2], std::atoll(argv[3]));
  else if (mode == "disabled")
    mode_disabled();
  else if (mode == "threads")
    mode_threads();
  else {
    fprintf(stderr, "usage: cache_check key | lru [MB] | cap MB MIB | cap0 | disabled | threads\n");
    return 2;
  }
  fflush(stderr);
  printf("CACHE_CHECK mode=%s checks=%ld failures=%ld %s\n", mode.c_str(), g_checks.load(), g_failures.load(), g_failures ? "FAILED" : "OK");
  return g_failures ? 1 : 0;
}
