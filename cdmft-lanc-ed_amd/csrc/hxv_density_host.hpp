// Host side of hxv_observables_accumulate and hxv_apply_density_ops: their tables as plain vectors (hxv_observables_tables.cpp,
// hxv_density_ops_tables.cpp, pure C++, no HIP call), shared by the two entry points (hxv_observables.hip, hxv_density_ops.hip), which only
// upload them, and the stand-alone check (tests/host/density_tables_check.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "hxv_internal.hpp"

namespace hxv {

// ---- observables.  Everything in DEVICE-row numbering, the basis signs of the device row order folded into the pair's sign.
struct ObsHostTables {
  int nimp = 0, nw = 0, np = 0, gtot = 0;  // nw = 2^nimp W bins, np = nimp^2 pairs p = is + nimp*js, gtot = nw + 2*np groups of a column
  // up side (rows of one column): groups [seg_ptr[g], seg_ptr[g+1]) of (row_a, row_b, sign), g < nw: W bins (row_a == row_b), then np pair
  // groups; a pair group with is >= js is empty (R(js,is) = conj R(is,js): the host fills the lower triangle)
  std::vector<int32_t> seg_ptr, ent_a, ent_b;
  std::vector<int8_t> ent_s;
  // dw side (this rank's columns): pairs [dwp_ptr[c], dwp_ptr[c+1]) of (partner column slot, pair index, sign); a partner column owned by
  // rank o sits at slot o*cmax + (its index in o's slab) of the gathered copy, or is the column itself when the sector is not split
  std::vector<int32_t> dwp_ptr, dwp_slot, dwp_p;
  std::vector<int8_t> dwp_s;
  // this rank's columns by dw impurity bits: dwbin_cols[dwbin_ptr[g] .. dwbin_ptr[g+1])
  std::vector<int32_t> dwbin_ptr, dwbin_cols;
};
// "" or what is wrong (an "observables: ..." message of hxv_observables_accumulate)
std::string obs_build_tables(const SectorHost& s, int nimp, ObsHostTables& t);

// ---- density operators
constexpr int DOP_MAX_NIMP = 10;  // two 5-bit halves
constexpr int DOP_CHUNK = 2048;   // rows of a work item, at most
constexpr int DOP_WG_PER_CU = 8;
struct DopHostTables {
  std::vector<uint32_t> occ_up, occ_dw;  // [pitch] by device row (pad rows 0), [max(qdw,1)] by local column: the low nimp bits
  int nchunk = 1, rows = 0;              // chunks a column is cut into, rows of a chunk (a multiple of 8)
  int64_t nitems = 0;                    // qdw * nchunk
  int grid = 1;                          // workgroups of the two passes
};
// "" or what is wrong (a "density operators: ..." message of hxv_apply_density_ops); ncu: the device's compute units
std::string dop_build_tables(const SectorHost& s, int nimp, int ncu, DopHostTables& t);

}  // namespace hxv
