// correction_direct.h — the host step of the direct build (include/vnr_amd.h, "corrections built straight into bit planes"): from the
// per-cell pairs pass 1 folded to the entries of the flagged cells and to where each one's groups and plane words start.  Host only,
// no HIP include (like correction_packed_format.h): tests build it with the host compiler under sanitizers.
#pragma once

#include "correction_packed_format.h"

namespace vnr {

// per macrocell of the grid: max |q| saturated to 32 bits, the sum of nbits over its groups (correction.hip's RateCell)
struct CorrectionDirectStat { uint32_t max_q, nbits; };

// a flagged cell: its first group in the walk over ALL cells of the grid (where pass 1 left its groups' nbits), its first group in the
// packed group table and its first plane word -- the last two are correction_plane_index's cell_group0 and cell_word0
struct CorrectionDirectPlace { uint64_t grid_group0, group0, word0; };

struct CorrectionDirectPlan {
  bool refused = false;                        // some cell has max |q| > 2^31 - 1: nothing else is filled in
  std::vector<CorrectionCellEntry> cells;      // {cell, width}, ascending: the width rule of the build on max |q| (kind 2: type_size)
  std::vector<CorrectionDirectPlace> places;   // beside cells
  uint64_t n_groups = 0, n_words = 0;          // groups and plane words of the flagged cells
};

// stats: n_cells = correction_n_cells(dims) pairs.  A cell is flagged by max_q != 0; the nbits of an unflagged cell are not looked at
// (kind 2 records them whether or not a group differs).
CorrectionDirectPlan correction_direct_plan(const int dims[3], uint32_t kind, uint32_t type_size, const CorrectionDirectStat* stats, uint64_t n_cells);

}  // namespace vnr
