// Stand-alone check of the option tables (csrc/hxv_options.cpp; include/hxv.h "Options").  No HIP runtime call, no device: the handles it
// constructs own no device allocation.
//
//   options_check --names                     "set NAME GROUP" for every settable row, then "get NAME" for every read-back row; nothing else
//   options_check NAME=V[,V...] ...           the values to try for the options of groups 1 and 2 (tests/test_host_options_check.py passes
//                                             the OPTIONS table of tests/test_gpu_options.py); a row of those groups without values fails
//
// Every handle under test is first filled with distinct sentinels -- every option field, every field a read-back answers from -- so that
// "unchanged" never means "still the default" and a row that reads a neighbour's field is seen.  The program walks the tables: a row
// added later is checked without an edit here (a read-back from a field that fill() does not know fails until fill() writes it).
// Every failed check prints "options_check: FAIL: ..." on stderr; stdout holds one "CASE ..." line per case and ends with OK or FAILED.
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

#include "hxv_options.hpp"

using namespace hxv;

namespace {

long g_checks = 0, g_failures = 0;

void check(bool ok, const char* f, ...) {
  ++g_checks;
  if (ok) return;
  ++g_failures;
  char buf[1024];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  fprintf(stderr, "options_check: FAIL: %s\n", buf);
}

const OptionRow* row_of(const char* name) {
  for (const OptionRow& r : option_rows())
    if (!strcmp(r.name, name)) return &r;
  return nullptr;
}
int& slot(hxv_handle& h, const OptionRow& r) { return *r.slot(&h, &h.plan.opt); }

// distinct values in every field the two tables reach; `written`: the values a read-back can answer
void fill(hxv_handle& h, std::set<int64_t>* written = nullptr) {
  int64_t next = 1000;
  for (const OptionRow& r : option_rows()) slot(h, r) = (int)next++;  // (table order: "lds_budget_kb" before its two halves, which overwrite it)
  std::set<int64_t> w;
  auto put = [&](auto& field) {
    field = (typename std::remove_reference<decltype(field)>::type)next;
    w.insert(next++);
  };
  auto put_frac = [&](double& field, double scale) {  // a double that its read-back truncates: (int64_t)(scale * field) = the sentinel
    field = ((double)next + 0.5) / scale;
    w.insert(next++);
  };
  for (double& us : h.open_us) put_frac(us, 1.0);
  put(h.open_cache_hit);
  put(h.eigh_last_full), put(h.eigh_last_local), put(h.eigh_last_search), put(h.eigh_last_check);
  put(h.eigh_last_restarts), put(h.eigh_last_fused_restarts), put(h.eigh_last_fused_first);
  put(h.last_real), put(h.plan.dw_order_last), put(h.n_allreduce), put(h.n_slab_copy), put(h.last_overlapped_us);
  for (int64_t& us : h.twin_last_us) put(us);
  put(h.plan.ncoef_up), put(h.plan.ncoef_dw);
  for (SpinTiles* t : {&h.plan.up, &h.plan.dw}) {
    put(t->lowbits), put(t->p16_bits), put(t->k_in), put(t->k_out), put(t->n_in), put(t->n_out), put(t->max_block), put(t->nblocks);
    put(t->table_classes), put(t->rs_tables), put(t->max_outer);
    put_frac(t->slots_in, 100.0), put_frac(t->slots_out, 100.0), put_frac(t->bh_per_row, 100.0), put_frac(t->rs_per_row, 100.0);
  }
  if (written) *written = w;
}

// the handle's option fields (every slot of the table) and its current plan's options, byte for byte
struct Snapshot {
  std::vector<int> slots;
  TileOptions opt;
  bool operator==(const Snapshot& b) const { return slots == b.slots && !memcmp(&opt, &b.opt, sizeof opt); }
};
Snapshot snapshot(hxv_handle& h) {
  Snapshot s;
  for (const OptionRow& r : option_rows()) {
    s.slots.push_back(slot(h, r));
    if (r.slot2) s.slots.push_back(*r.slot2(&h, &h.plan.opt));
  }
  memcpy(&s.opt, &h.plan.opt, sizeof s.opt);
  return s;
}

void experiments(const char* value) {
  if (value)
    setenv("HXV_EXPERIMENTS", value, 1);
  else
    unsetenv("HXV_EXPERIMENTS");
}

int stored_value(const OptionRow& r, int64_t v) {
  if (r.kind == OptKind::FLAG) return v ? 1 : 0;
  if (r.kind == OptKind::CLAMP) return (int)(v < r.lo ? r.lo : v > r.hi ? r.hi : v);
  return (int)v;
}

// one accepted store on a sentinel-filled handle, with everything part 2 of the contract says about it
void accepted(const OptionRow& r, int64_t v) {
  hxv_handle h;
  fill(h);
  const Snapshot before = snapshot(h);
  const int old = slot(h, r);
  TileOptions o;
  bool rebuild = !r.rebuild;
  const int rc = option_store(&h, r.name, v, &o, &rebuild);
  check(rc == HXV_OK, "%s = %" PRId64 ": refused (%d, \"%s\")", r.name, v, rc, hxv_last_error());
  check(rebuild == r.rebuild, "%s = %" PRId64 ": rebuild = %d", r.name, v, (int)rebuild);
  if (rc != HXV_OK || rebuild != r.rebuild) return;
  const int want = stored_value(r, v);
  if (r.rebuild) {
    // the handle is untouched; the options handed back are the handle's with the named field (both, for "lds_budget_kb") replaced
    check(snapshot(h) == before, "%s = %" PRId64 ": a rebuild store changed the handle", r.name, v);
    TileOptions expect = h.plan.opt;
    *r.slot(&h, &expect) = want;
    if (r.slot2) *r.slot2(&h, &expect) = want;
    check(!memcmp(&expect, &o, sizeof o), "%s = %" PRId64 ": the options handed back differ from the handle's in another field, or lack the value", r.name, v);
    check(*r.slot(&h, &o) == want && (!r.slot2 || *r.slot2(&h, &o) == want), "%s = %" PRId64 ": the options handed back lack the value", r.name, v);
    return;
  }
  check(slot(h, r) == want, "%s = %" PRId64 ": the field holds %d", r.name, v, slot(h, r));
  const int64_t got = option_read(&h, r.name);
  check(got == (r.readable ? want : -1), "%s = %" PRId64 ": read back %" PRId64, r.name, v, got);
  slot(h, r) = old;  // with the one field a direct store may change put back, the handle is what it was
  check(snapshot(h) == before, "%s = %" PRId64 ": the store changed another field", r.name, v);
}

// one refusal: the code, the exact message, nothing changed, no rebuild asked for
void refused(const char* name, int64_t v, const char* message) {
  hxv_handle h;
  fill(h);
  const Snapshot before = snapshot(h);
  TileOptions o;
  bool rebuild = true;
  const int rc = option_store(&h, name, v, &o, &rebuild);
  check(rc == HXV_ERR_ARG && !rebuild, "%s = %" PRId64 ": code %d, rebuild %d, expected the refusal \"%s\"", name, v, rc, (int)rebuild, message);
  check(!strcmp(hxv_last_error(), message), "%s = %" PRId64 ": message \"%s\", expected \"%s\"", name, v, hxv_last_error(), message);
  check(snapshot(h) == before, "%s = %" PRId64 ": the refusal changed the handle", name, v);
}

std::string gate_message(const char* name) {
  return std::string("option ") + name + " is a timing experiment that gives wrong results; set HXV_EXPERIMENTS=1 to enable it";
}

// ---- 1. store and read back -----------------------------------------------------------------------------------------------------------
void case_store(const std::map<std::string, std::vector<int64_t>>& values) {
  for (const OptionRow& r : option_rows()) {
    if (r.group == 3) {
      experiments(nullptr);
      accepted(r, !strcmp(r.name, "passes") ? 3 : 0);  // the neutral value passes the gate
      experiments("1");
      if (!strcmp(r.name, "passes"))
        for (int64_t v : {1, 2, 3}) accepted(r, v);
      else
        for (int64_t v : {1, 32, 4096 | 8192 | 5}) accepted(r, v);
      experiments(nullptr);
      continue;
    }
    const auto it = values.find(r.name);
    check(it != values.end() && !it->second.empty(), "%s: no values to try on the command line", r.name);
    if (it == values.end()) continue;
    for (int64_t v : it->second) accepted(r, v);
  }
  for (const auto& kv : values) check(row_of(kv.first.c_str()) != nullptr, "%s: values on the command line for a name the table does not hold", kv.first.c_str());
}

// ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
void case_refusals() {
  experiments(nullptr);
  // one value below and one above each range
  struct Range {
    const char* name;
    int64_t lo, hi;
    const char* message;
  };
  const Range ranges[] = {{"kernel", 0, 1, "kernel must be 0 or 1"},
                          {"lds_min_kb_up", 0, 160, "lds_min_kb must be in [0,160]"},
                          {"lds_min_kb_dw", 0, 160, "lds_min_kb must be in [0,160]"},
                          {"eigh_keep_pct", 5, 80, "eigh_keep_pct must be in [5,80]"},
                          {"pair_rows", -1, 1, "pair_rows must be -1, 0 or 1"},
                          {"block_order", -1, 2, "block_order must be -1, 0, 1 or 2"},
                          {"passes", 1, 3, "passes must be 1, 2 or 3"}};
  std::set<std::string> ranged;
  for (const Range& g : ranges) {
    ranged.insert(g.name);
    const OptionRow* r = row_of(g.name);
    check(r && r->kind == OptKind::RANGE && r->lo == g.lo && r->hi == g.hi, "%s: not a row with the range [%" PRId64 ",%" PRId64 "]", g.name, g.lo, g.hi);
    experiments(!strcmp(g.name, "passes") ? "1" : nullptr);  // (the gate comes before the range rule)
    refused(g.name, g.lo - 1, g.message);
    refused(g.name, g.hi + 1, g.message);
    refused(g.name, INT64_MIN, g.message);
    refused(g.name, INT64_MAX, g.message);
    experiments(nullptr);
  }
  for (const OptionRow& r : option_rows())
    check((r.kind == OptKind::RANGE) == (ranged.count(r.name) == 1), "%s: a range row this program does not know, or a known one that lost its range", r.name);
  // the experiment gate: unset, "0", empty -> refused before any range rule; "1" -> the range rule speaks
  const struct {
    const char* name;
    int64_t value;
  } gated[] = {{"passes", 2}, {"passes", 5}, {"passes", 0}, {"debug", 32}, {"debug", 4096}, {"debug", -1}, {"job_debug", 1}};
  for (const char* env : {(const char*)nullptr, "0", "", "yes"}) {
    experiments(env);
    for (const auto& g : gated) refused(g.name, g.value, gate_message(g.name).c_str());
  }
  experiments("1");
  refused("passes", 5, "passes must be 1, 2 or 3");
  experiments(nullptr);
  for (const OptionRow& r : option_rows()) {
    const bool gate = !strcmp(r.name, "passes") || !strcmp(r.name, "debug") || !strcmp(r.name, "job_debug");
    check((r.group == 3) == gate, "%s: group %d", r.name, r.group);
  }
  // NULL arguments
  {
    hxv_handle h;
    fill(h);
    const Snapshot before = snapshot(h);
    TileOptions o;
    bool rebuild = true;
    check(option_store(nullptr, "kernel", 1, &o, &rebuild) == HXV_ERR_ARG && !rebuild && !strcmp(hxv_last_error(), "hxv_set_option: NULL"), "set on a NULL handle: \"%s\"", hxv_last_error());
    hxv::fail(0, "");
    rebuild = true;
    check(option_store(&h, nullptr, 1, &o, &rebuild) == HXV_ERR_ARG && !rebuild && !strcmp(hxv_last_error(), "hxv_set_option: NULL"), "set of a NULL name: \"%s\"", hxv_last_error());
    check(snapshot(h) == before, "set of a NULL name changed the handle");
    check(option_read(nullptr, "kernel") == -1, "get on a NULL handle");
    check(option_read(&h, nullptr) == -1, "get of a NULL name");
  }
  // unknown names, every read-only name among them
  refused("no_such_option", 1, "unknown option no_such_option");
  refused("", 1, "unknown option ");
  refused("nblocks_up", 1, "unknown option nblocks_up");
  for (const ReadbackRow& r : readback_rows()) refused(r.name, 0, (std::string("unknown option ") + r.name).c_str());
}

// ---- 3. flag normalisation and clamping -----------------------------------------------------------------------------------------------
void case_normalise() {
  const char* flags[] = {"lanczos_fused", "real_vectors", "lanczos_graph", "lanczos_inplace", "eigh_degenerate", "eigh_fuse_restart",
                         "eigh_measure_all", "exchange_overlap", "real_dw_pairs", "wt_colmajor", "spread_banks", "fold_nd"};
  std::set<std::string> known(flags, flags + sizeof flags / sizeof flags[0]);
  for (const OptionRow& r : option_rows()) {
    check((r.kind == OptKind::FLAG) == (known.count(r.name) == 1), "%s: a flag this program does not know, or a known one that is no flag", r.name);
    if (r.kind == OptKind::FLAG)
      for (int64_t v : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)-1, INT64_MAX, INT64_MIN}) accepted(r, v);  // (accepted() expects value ? 1 : 0)
    if (r.kind == OptKind::CLAMP)
      for (int64_t v : {r.lo - 5, r.lo, r.hi, r.hi + 5, INT64_MIN, INT64_MAX}) accepted(r, v);
    check(r.kind != OptKind::CLAMP || !strcmp(r.name, "job_up"), "%s: clamps", r.name);
  }
  {
    hxv_handle h;
    fill(h);
    check(slot(h, *row_of("fold_nd")) == h.dev.nd.fold && &slot(h, *row_of("fold_nd")) == &h.dev.nd.fold, "fold_nd does not live in the handle's dev.nd.fold");
    TileOptions o;
    bool rebuild = false;
    check(option_store(&h, "job_up", -5, &o, &rebuild) == HXV_OK && rebuild && o.job_up == 0, "job_up = -5 stores %d", o.job_up);
    check(option_store(&h, "job_up", 7, &o, &rebuild) == HXV_OK && rebuild && o.job_up == 2, "job_up = 7 stores %d", o.job_up);
  }
}

// ---- 4. table hygiene -----------------------------------------------------------------------------------------------------------------
void case_hygiene() {
  std::set<std::string> names;
  for (const OptionRow& r : option_rows()) check(names.insert(r.name).second, "%s occurs twice", r.name);
  for (const ReadbackRow& r : readback_rows()) check(names.insert(r.name).second, "%s occurs twice", r.name);
  hxv_handle h;
  std::set<int64_t> written, seen;
  fill(h, &written);
  std::set<std::string> unreadable;
  for (const OptionRow& r : option_rows()) {
    const int64_t got = option_read(&h, r.name);
    if (!r.readable) {
      unreadable.insert(r.name);
      check(got == -1, "%s is not readable and answers %" PRId64, r.name, got);
    } else if (r.read) {  // answers from another field than the stored one
      check(got == r.read(&h) && got != slot(h, r) && written.count(got), "%s answers %" PRId64, r.name, got);
      check(seen.insert(got).second, "%s answers from a field another name answers from", r.name);
    } else {
      check(got == slot(h, r), "%s answers %" PRId64 ", its field holds %d", r.name, got, slot(h, r));
      check(seen.insert(got).second, "%s shares its field with another name", r.name);
    }
  }
  check(unreadable == std::set<std::string>{"lds_budget_kb", "passes", "debug", "job_debug"}, "the unreadable options are not lds_budget_kb, passes, debug and job_debug");
  check(option_read(&h, "tile_bits_up") == h.plan.up.lowbits && option_read(&h, "tile_bits_dw") == h.plan.dw.lowbits, "tile_bits_* do not answer the plan's block bits");
  check(option_read(&h, "rows_per_tile") == h.plan.opt.rows_per_tile, "rows_per_tile does not answer the plan's resolved value");
  for (const ReadbackRow& r : readback_rows()) {
    const int64_t got = option_read(&h, r.name);
    check(got == r.read(&h), "%s: the read function answers %" PRId64 ", the lookup %" PRId64, r.name, r.read(&h), got);
    if (!strcmp(r.name, "job_up_active") || !strcmp(r.name, "pool_live_blocks")) {  // computed: no jobs on this plan, no buffer handed out
      check(got == 0, "%s answers %" PRId64 " on a handle without a device", r.name, got);
      continue;
    }
    check(written.count(got) == 1, "%s answers %" PRId64 ": not the value of a field that fill() wrote", r.name, got);
    check(seen.insert(got).second, "%s answers from a field another name answers from", r.name);
  }
  // the truncations of the *_x100 read-backs and the open costs, on values of our own
  h.plan.up.slots_in = 1.239;
  h.plan.dw.rs_per_row = 0.999;
  h.open_us[3] = 17.9;
  check(option_read(&h, "slots_in_up_x100") == 123 && option_read(&h, "rs_dw_x100") == 99 && option_read(&h, "open_us_total") == 17, "the read-backs of doubles do not truncate");
  h.plan.opt.job_up = 1;
  check(option_read(&h, "job_up_active") == 0, "job_up_active on a plan without tables");
  check(option_read(&h, "no_such_option") == -1 && option_read(&h, "") == -1, "a name of neither table does not answer -1");
}

void print_names() {
  for (const OptionRow& r : option_rows()) printf("set %s %d\n", r.name, r.group);
  for (const ReadbackRow& r : readback_rows()) printf("get %s\n", r.name);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--names")) {
    print_names();
    return 0;
  }
  std::map<std::string, std::vector<int64_t>> values;
  for (int a = 1; a < argc; ++a) {
    const char* eq = strchr(argv[a], '=');
    if (!eq || eq == argv[a]) {
      fprintf(stderr, "usage: options_check --names | options_check NAME=V[,V...] ...\n");
      return 2;
    }
    std::vector<int64_t>& v = values[std::string(argv[a], (size_t)(eq - argv[a]))];
    for (const char* p = eq + 1; *p;) {
      char* end = nullptr;
      v.push_back(strtoll(p, &end, 10));
      if (end == p) return 2;
      p = *end == ',' ? end + 1 : end;
    }
  }
  struct {
    const char* name;
    void (*run)();
  } cases[] = {{"refusals", case_refusals}, {"flag normalisation and clamping", case_normalise}, {"table hygiene", case_hygiene}};
  long before = g_checks, fbefore = g_failures;
  case_store(values);
  printf("CASE store and read back: %ld checks, %ld failures\n", g_checks - before, g_failures - fbefore);
  for (const auto& c : cases) {
    before = g_checks, fbefore = g_failures;
    c.run();
    printf("CASE %s: %ld checks, %ld failures\n", c.name, g_checks - before, g_failures - fbefore);
  }
  fflush(stderr);
  printf("OPTIONS_CHECK rows=%zu+%zu checks=%ld failures=%ld\n%s\n", option_rows().n, readback_rows().n, g_checks, g_failures, g_failures ? "FAILED" : "OK");
  return g_failures ? 1 : 0;
}
