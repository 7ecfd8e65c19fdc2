// The option tables behind hxv_set_option and hxv_get_option (include/hxv.h, "Options") and the two functions that
// read them.  Host C++: no HIP runtime call, so the file links into a stand-alone checker (tests/host/options_check.cpp).  A new option
// is one row here and one line in the header.
#include "hxv_options.hpp"

#include <cstdlib>
#include <cstring>

namespace hxv {
namespace {
thread_local std::string g_err;
}
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
}  // namespace hxv

extern "C" const char* hxv_last_error(void) { return hxv::g_err.c_str(); }

namespace hxv {
namespace {

using Slot = int* (*)(hxv_handle*, TileOptions*);
template <int hxv_handle::*F>
int* in_handle(hxv_handle* h, TileOptions*) { return &(h->*F); }
template <int TileOptions::*F>
int* in_plan(hxv_handle*, TileOptions* o) { return &(o->*F); }
int* in_nd(hxv_handle* h, TileOptions*) { return &h->dev.nd.fold; }  // (the handle's copy: the host description may be shared with other handles)

constexpr OptionRow flag(const char* name, int group, Slot slot, bool rebuild = false) {
  return {name, group, OptKind::FLAG, 0, 1, nullptr, slot, rebuild, nullptr, true, nullptr};
}
constexpr OptionRow range(const char* name, int group, int64_t lo, int64_t hi, const char* refusal, Slot slot) {
  return {name, group, OptKind::RANGE, lo, hi, refusal, slot, false, nullptr, true, nullptr};
}
constexpr OptionRow any(const char* name, int group, Slot slot, bool rebuild) {
  return {name, group, OptKind::ANY, 0, 0, nullptr, slot, rebuild, nullptr, true, nullptr};
}
// a tiling knob: stored as given into a copy of the plan's options, judged by make_tile_plan alone
constexpr OptionRow knob(const char* name, Slot slot) { return any(name, 2, slot, true); }
constexpr OptionRow unreadable(OptionRow r) {
  r.readable = false;
  return r;
}
constexpr OptionRow reads(OptionRow r, int64_t (*read)(const hxv_handle*)) {
  r.read = read;
  return r;
}
constexpr OptionRow also(OptionRow r, Slot slot2) {
  r.slot2 = slot2;
  return r;
}

using H = const hxv_handle*;
using TO = TileOptions;
constexpr bool REBUILD = true, NO_REBUILD = false;
constexpr const char* LDS_MIN_REFUSAL = "lds_min_kb must be in [0,160]";

}  // namespace

Rows<OptionRow> option_rows() {
  static const OptionRow rows[] = {
      // 1. behaviour
      range("kernel", 1, 0, 1, "kernel must be 0 or 1", in_handle<&hxv_handle::kernel>),
      flag("real_vectors", 1, in_handle<&hxv_handle::real_vectors>),
      flag("lanczos_fused", 1, in_handle<&hxv_handle::lz_fused>),
      flag("lanczos_graph", 1, in_handle<&hxv_handle::lz_graph>),
      flag("lanczos_inplace", 1, in_handle<&hxv_handle::lz_inplace>),  // split sectors: Lanczos vectors in their slot of a gather buffer
      flag("eigh_degenerate", 1, in_handle<&hxv_handle::eigh_degenerate>),
      flag("eigh_measure_all", 1, in_handle<&hxv_handle::eigh_measure_all>),
      range("eigh_keep_pct", 1, 5, 80, "eigh_keep_pct must be in [5,80]", in_handle<&hxv_handle::eigh_keep_pct>),
      flag("eigh_fuse_restart", 1, in_handle<&hxv_handle::eigh_fuse_restart>),
      flag("fold_nd", 1, in_nd),  // spH0nd inside pass A (default) or as its own pass over hv
      flag("exchange_overlap", 1, in_handle<&hxv_handle::a2a_overlap>),  // exchange mode 2: diagonal + up hops on a second stream during the transposes
      // 2. tile shape and scheduling.  The knobs rebuild the plan (old tables stay allocated until hxv_destroy); the others are read from the
      //    current plan's options at launch time
      knob("cols_per_tile", in_plan<&TO::cols_per_tile>),
      knob("rows_per_tile", in_plan<&TO::rows_per_tile>),  // (reads back what the plan resolved 0 to: make_tile_plan writes it into the same field)
      unreadable(also(knob("lds_budget_kb", in_plan<&TO::lds_budget_kb_up>), in_plan<&TO::lds_budget_kb_dw>)),
      knob("lds_budget_kb_up", in_plan<&TO::lds_budget_kb_up>),
      knob("lds_budget_kb_dw", in_plan<&TO::lds_budget_kb_dw>),
      knob("threads_up", in_plan<&TO::threads_up>),
      knob("threads_dw", in_plan<&TO::threads_dw>),
      knob("sort_mode", in_plan<&TO::sort_mode>),
      knob("sort_mode_dw", in_plan<&TO::sort_mode_dw>),
      knob("wt_cols", in_plan<&TO::wt_cols>),
      reads(knob("tile_bits_up", in_plan<&TO::force_bits_up>), [](H h) -> int64_t { return h->plan.up.lowbits; }),  // the block bits of the plan in use
      reads(knob("tile_bits_dw", in_plan<&TO::force_bits_dw>), [](H h) -> int64_t { return h->plan.dw.lowbits; }),
      range("lds_min_kb_up", 2, 0, 160, LDS_MIN_REFUSAL, in_plan<&TO::lds_min_kb_up>),
      range("lds_min_kb_dw", 2, 0, 160, LDS_MIN_REFUSAL, in_plan<&TO::lds_min_kb_dw>),
      flag("spread_banks", 2, in_plan<&TO::spread_banks>, REBUILD),
      {"job_up", 2, OptKind::CLAMP, 0, 2, nullptr, in_plan<&TO::job_up>, REBUILD, nullptr, true, nullptr},
      knob("job_groups", in_plan<&TO::job_groups>),
      knob("job_cols", in_plan<&TO::job_cols>),
      knob("job_stages", in_plan<&TO::job_stages>),
      any("job_max_blocks", 2, in_plan<&TO::job_max_blocks>, NO_REBUILD),
      flag("wt_colmajor", 2, in_plan<&TO::wt_colmajor>),
      flag("real_dw_pairs", 2, in_plan<&TO::real_dw_pairs>),
      range("pair_rows", 2, -1, 1, "pair_rows must be -1, 0 or 1", in_plan<&TO::pair_rows>),
      range("block_order", 2, -1, 2, "block_order must be -1, 0, 1 or 2", in_plan<&TO::block_order>),
      // 3. timing experiments (results are wrong or partial when set): anything but the field's default only with HXV_EXPERIMENTS=1 in the environment
      unreadable(range("passes", 3, 1, 3, "passes must be 1, 2 or 3", in_plan<&TO::passes>)),
      unreadable(any("debug", 3, in_plan<&TO::debug>, NO_REBUILD)),
      unreadable(any("job_debug", 3, in_plan<&TO::job_debug>, NO_REBUILD)),
  };
  return {rows, sizeof rows / sizeof rows[0]};
}

Rows<ReadbackRow> readback_rows() {
  static const ReadbackRow rows[] = {
      // what THIS open cost, microseconds (0 for the parts a cached image saved): host description, tile plan, table upload, whole create call
      {"open_us_host", [](H h) -> int64_t { return (int64_t)h->open_us[0]; }},
      {"open_us_plan", [](H h) -> int64_t { return (int64_t)h->open_us[1]; }},
      {"open_us_upload", [](H h) -> int64_t { return (int64_t)h->open_us[2]; }},
      {"open_us_total", [](H h) -> int64_t { return (int64_t)h->open_us[3]; }},
      {"open_cache_hit", [](H h) -> int64_t { return h->open_cache_hit; }},
      // driver read-backs
      {"eigh_last_full_passes", [](H h) -> int64_t { return h->eigh_last_full; }},
      {"eigh_last_local_passes", [](H h) -> int64_t { return h->eigh_last_local; }},
      {"eigh_last_search_products", [](H h) -> int64_t { return h->eigh_last_search; }},  // *nmatvec of the last hxv_eigh_lowest = search + check
      {"eigh_last_check_products", [](H h) -> int64_t { return h->eigh_last_check; }},
      {"eigh_last_restarts", [](H h) -> int64_t { return h->eigh_last_restarts; }},              // thick restarts of the search round
      {"eigh_last_fused_restarts", [](H h) -> int64_t { return h->eigh_last_fused_restarts; }},  // ... whose rotation went through tr_rotate_dots
      {"eigh_last_fused_first_steps", [](H h) -> int64_t { return h->eigh_last_fused_first; }},  // restart cycles begun by tr_axpy_mdot
      {"lanczos_real_last", [](H h) -> int64_t { return h->last_real; }},
      {"pass_b_order_last", [](H h) -> int64_t { return h->plan.dw_order_last; }},  // phase order the last pass-B launch ran (0 / 1; -1: none yet)
      {"allreduce_count", [](H h) -> int64_t { return h->n_allreduce; }},  // sum all-reduces of a split sector since creation (the drivers' dot products)
      {"pool_live_blocks", [](H h) -> int64_t { return pool_live_blocks(h->device); }},  // buffer-cache blocks out on the handle's device (every handle's and call's)
      {"slab_copies", [](H h) -> int64_t { return h->n_slab_copy; }},  // exchanges whose vector was not at home in a gather buffer
      {"time_kernels_overlapped_us", [](H h) -> int64_t { return h->last_overlapped_us; }},
      // the last split hxv_twin_vector INTO this handle, by HIP events on its stream (-1: none yet): pack kernel, exchange, unpack kernel
      {"twin_last_pack_us", [](H h) -> int64_t { return h->twin_last_us[0]; }},
      {"twin_last_exchange_us", [](H h) -> int64_t { return h->twin_last_us[1]; }},
      {"twin_last_unpack_us", [](H h) -> int64_t { return h->twin_last_us[2]; }},
      // plan statistics
      {"p16_bits_up", [](H h) -> int64_t { return h->plan.up.p16_bits; }},
      {"p16_bits_dw", [](H h) -> int64_t { return h->plan.dw.p16_bits; }},
      {"k_in_up", [](H h) -> int64_t { return h->plan.up.k_in; }},
      {"k_out_up", [](H h) -> int64_t { return h->plan.up.k_out; }},
      {"k_in_dw", [](H h) -> int64_t { return h->plan.dw.k_in; }},
      {"k_out_dw", [](H h) -> int64_t { return h->plan.dw.k_out; }},
      {"n_in_up", [](H h) -> int64_t { return h->plan.up.n_in; }},
      {"n_out_up", [](H h) -> int64_t { return h->plan.up.n_out; }},
      {"n_in_dw", [](H h) -> int64_t { return h->plan.dw.n_in; }},
      {"n_out_dw", [](H h) -> int64_t { return h->plan.dw.n_out; }},
      {"slots_in_up_x100", [](H h) -> int64_t { return (int64_t)(100 * h->plan.up.slots_in); }},
      {"slots_out_up_x100", [](H h) -> int64_t { return (int64_t)(100 * h->plan.up.slots_out); }},
      {"slots_in_dw_x100", [](H h) -> int64_t { return (int64_t)(100 * h->plan.dw.slots_in); }},
      {"bh_up_x100", [](H h) -> int64_t { return (int64_t)(100 * h->plan.up.bh_per_row); }},
      {"rs_up_x100", [](H h) -> int64_t { return (int64_t)(100 * h->plan.up.rs_per_row); }},
      {"bh_dw_x100", [](H h) -> int64_t { return (int64_t)(100 * h->plan.dw.bh_per_row); }},
      {"rs_dw_x100", [](H h) -> int64_t { return (int64_t)(100 * h->plan.dw.rs_per_row); }},
      {"max_block_up", [](H h) -> int64_t { return h->plan.up.max_block; }},
      {"max_block_dw", [](H h) -> int64_t { return h->plan.dw.max_block; }},
      {"ncoef_up", [](H h) -> int64_t { return h->plan.ncoef_up; }},  // distinct hopping amplitudes: the kernels' coefficient tables hold 2 * ncoef + 1 words
      {"ncoef_dw", [](H h) -> int64_t { return h->plan.ncoef_dw; }},
      {"nblocks_up", [](H h) -> int64_t { return h->plan.up.nblocks; }},
      {"nblocks_dw", [](H h) -> int64_t { return h->plan.dw.nblocks; }},
      {"table_classes_up", [](H h) -> int64_t { return h->plan.up.table_classes; }},
      {"table_classes_dw", [](H h) -> int64_t { return h->plan.dw.table_classes; }},
      {"rs_tables_up", [](H h) -> int64_t { return h->plan.up.rs_tables; }},
      {"rs_tables_dw", [](H h) -> int64_t { return h->plan.dw.rs_tables; }},
      {"max_outer_up", [](H h) -> int64_t { return h->plan.up.max_outer; }},
      {"max_outer_dw", [](H h) -> int64_t { return h->plan.dw.max_outer; }},
      {"job_up_active", [](H h) -> int64_t {
         return (h->plan.opt.job_up == 1 && job_up_planned(h->dev, h->plan, false, std::max(h->plan.opt.job_cols, h->plan.opt.wt_cols))) ? 1 : 0;
       }},
  };
  return {rows, sizeof rows / sizeof rows[0]};
}

int option_store(hxv_handle* h, const char* name, int64_t value, TileOptions* rebuilt, bool* rebuild) {
  *rebuild = false;
  if (!h || !name) return fail(HXV_ERR_ARG, "hxv_set_option: NULL");
  const Rows<OptionRow> rows = option_rows();
  const OptionRow* r = std::find_if(rows.begin(), rows.end(), [&](const OptionRow& o) { return !strcmp(o.name, name); });
  if (r == rows.end()) return fail(HXV_ERR_ARG, std::string("unknown option ") + name);
  if (r->group == 3) {  // the neutral value, the field's default, is always accepted
    const char* ex = getenv("HXV_EXPERIMENTS");
    TileOptions neutral;
    if (!(ex && ex[0] == '1') && value != *r->slot(h, &neutral))
      return fail(HXV_ERR_ARG, std::string("option ") + name + " is a timing experiment that gives wrong results; set HXV_EXPERIMENTS=1 to enable it");
  }
  if (r->kind == OptKind::RANGE && (value < r->lo || value > r->hi)) return fail(HXV_ERR_ARG, r->refusal);
  const int stored = r->kind == OptKind::FLAG ? (value ? 1 : 0) : r->kind == OptKind::CLAMP ? (int)std::min(std::max(value, r->lo), r->hi) : (int)value;
  TileOptions* o = &h->plan.opt;
  if (r->rebuild) {
    *rebuilt = h->plan.opt;
    *rebuild = true;
    o = rebuilt;
  }
  *r->slot(h, o) = stored;
  if (r->slot2) *r->slot2(h, o) = stored;
  return HXV_OK;
}

int64_t option_read(const hxv_handle* h, const char* name) {
  if (!h || !name) return -1;
  for (const OptionRow& r : option_rows()) {
    if (strcmp(r.name, name)) continue;
    if (!r.readable) return -1;
    hxv_handle* hm = const_cast<hxv_handle*>(h);  // (the slots serve the store as well; nothing is written here)
    return r.read ? r.read(h) : *r.slot(hm, &hm->plan.opt);
  }
  for (const ReadbackRow& r : readback_rows())
    if (!strcmp(r.name, name)) return r.read(h);
  return -1;
}

}  // namespace hxv
