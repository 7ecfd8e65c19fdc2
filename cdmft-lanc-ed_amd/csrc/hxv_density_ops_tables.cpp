// Host tables of hxv_apply_density_ops (hxv_density_host.hpp): pure C++, no HIP call.  One impurity-occupation word per device row and per
// local column, and the work list of the two passes: every column cut into nchunk chunks of `rows` rows, one work item each.
#include <algorithm>

#include "hxv_density_host.hpp"

namespace hxv {

std::string dop_build_tables(const SectorHost& s, int nimp, int ncu, DopHostTables& t) {
  const uint32_t mask = (1u << nimp) - 1u;
  t = DopHostTables{};
  const std::vector<uint32_t>& mdev = s.dev_map_up();  // reference bit strings by device row
  t.occ_up.assign((size_t)s.pitch, 0u);
  t.occ_dw.assign((size_t)std::max(s.qdw, 1), 0u);
  for (int r = 0; r < s.dimup; ++r) t.occ_up[r] = mdev[r] & mask;
  for (int c = 0; c < s.qdw; ++c) t.occ_dw[c] = s.map_dw[s.dw0 + c] & mask;
  t.nchunk = std::max(1, (s.pitch + DOP_CHUNK - 1) / DOP_CHUNK);
  t.rows = (((s.pitch + t.nchunk - 1) / t.nchunk) + 7) & ~7;
  t.nitems = (int64_t)std::max(s.qdw, 0) * t.nchunk;
  if (t.nitems >= INT32_MAX) return "density operators: too many work items";
  t.grid = (int)std::max<int64_t>(1, std::min<int64_t>(t.nitems, (int64_t)DOP_WG_PER_CU * ncu));
  return std::string();
}

}  // namespace hxv
