// correction_direct.cpp — the host step of the direct build (correction_direct.h).  Host only; n_cells entries in, n_flagged out.
#include "correction_direct.h"

namespace vnr {

CorrectionDirectPlan correction_direct_plan(const int dims[3], uint32_t kind, uint32_t type_size, const CorrectionDirectStat* stats, uint64_t n_cells)
{
  CorrectionDirectPlan plan;
  for (uint64_t cl = 0; cl < n_cells; ++cl)
    if (stats[cl].max_q > 0x7fffffffu) {
      plan.refused = true;
      return plan;
    }
  uint64_t grid_group = 0;   // groups of the cells in front of cl, flagged or not
  for (uint64_t cl = 0; cl < n_cells; ++cl) {
    const uint64_t groups = correction_cell_groups(correction_cell_voxels(dims, (uint32_t)cl));
    const uint32_t m = stats[cl].max_q;
    if (m != 0) {
      const uint32_t width = kind == kCorrectionVerbatim ? type_size : (m <= 127 ? 1u : (m <= 32767 ? 2u : 4u));
      plan.cells.push_back(CorrectionCellEntry{(uint32_t)cl, width});
      plan.places.push_back(CorrectionDirectPlace{grid_group, plan.n_groups, plan.n_words});
      plan.n_groups += groups;
      plan.n_words += stats[cl].nbits;
    }
    grid_group += groups;
  }
  return plan;
}

}  // namespace vnr
