// The options of a handle, each stated once (hxv_options.cpp): what hxv_set_option accepts and stores and what hxv_get_option answers
// are both derived from the two tables below.  Host C++, no HIP runtime call.
#pragma once
#include <cstddef>
#include <cstdint>

#include "hxv_handle.hpp"

namespace hxv {

enum class OptKind {
  FLAG,   // stored as value ? 1 : 0
  RANGE,  // an integer in [lo, hi], refused with `refusal` outside
  CLAMP,  // an integer brought into [lo, hi], never refused
  ANY     // an integer stored as given
};

// One settable option.  `slot` says where it lives: a field of the handle (in_handle), of the handle's DevSector::nd (in_nd), or of a
// TileOptions (in_plan) -- the current plan's h->plan.opt, or with `rebuild` a copy of it that a new tile plan is made from.
struct OptionRow {
  const char* name;
  int group;  // of the header's option block: 1 behaviour, 2 tile shape and scheduling, 3 timing experiments (behind HXV_EXPERIMENTS=1)
  OptKind kind;
  int64_t lo, hi;
  const char* refusal;  // RANGE: the message of a refused value
  int* (*slot)(hxv_handle*, TileOptions*);
  bool rebuild;                          // storing it needs a new tile plan
  int* (*slot2)(hxv_handle*, TileOptions*);  // a second field that takes the same value ("lds_budget_kb"), or null
  bool readable;                         // false: hxv_get_option answers -1
  int64_t (*read)(const hxv_handle*);    // what hxv_get_option answers from when that is not the stored field, or null
};
// One name that hxv_get_option reports and hxv_set_option does not know: plan statistics, driver read-backs, open costs.
struct ReadbackRow {
  const char* name;
  int64_t (*read)(const hxv_handle*);
};
// The two tables, for a range-based for.  Behind functions: the engine's sources are all compiled as HIP, where a const table at namespace
// scope would be emitted for the device as well, host function pointers and all.
template <typename Row>
struct Rows {
  const Row* first;
  size_t n;
  const Row* begin() const { return first; }
  const Row* end() const { return first + n; }
};
Rows<OptionRow> option_rows();
Rows<ReadbackRow> readback_rows();

// hxv_set_option without its device half: the experiment gate, the range rule, the store.  -> HXV_OK, or HXV_ERR_ARG (a refused value,
// an unknown name, NULL) with the message recorded by hxv::fail and nothing changed.  HXV_OK with *rebuild = false: the value is in the
// handle or in its current plan's options.  HXV_OK with *rebuild = true: the handle is untouched and *rebuilt holds the current plan's
// options with the value in place; the caller makes a tile plan from them and commits it, or leaves the handle as it is.
int option_store(hxv_handle* h, const char* name, int64_t value, TileOptions* rebuilt, bool* rebuild);
// hxv_get_option: the settable table, then the read-backs, otherwise -1
int64_t option_read(const hxv_handle* h, const char* name);

}  // namespace hxv
