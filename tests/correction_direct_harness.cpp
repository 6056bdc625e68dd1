// Stand-alone driver of csrc/correction_direct.cpp for tests/test_correction_direct_host.py, built with the host compiler under
// sanitizers.  Each argument is a text file: "dx dy dz kind type_size n_cells" and then n_cells pairs "max_q nbits".  Prints per file
// "file i", then "refused" or "cells N groups G words W" and a line "e cell width grid_group0 group0 word0" per flagged cell.
#include "correction_direct.h"

#include <cstdio>
#include <fstream>
#include <vector>

int main(int argc, char** argv)
{
  for (int i = 1; i < argc; ++i) {
    std::ifstream in(argv[i]);
    int dims[3];
    unsigned kind, type_size;
    unsigned long long n_cells;
    if (!(in >> dims[0] >> dims[1] >> dims[2] >> kind >> type_size >> n_cells) || n_cells != vnr::correction_n_cells(dims)) {
      std::fprintf(stderr, "bad case file %s\n", argv[i]);
      return 2;
    }
    std::vector<vnr::CorrectionDirectStat> stats(n_cells);
    for (auto& s : stats)
      if (!(in >> s.max_q >> s.nbits)) {
        std::fprintf(stderr, "short case file %s\n", argv[i]);
        return 2;
      }
    const vnr::CorrectionDirectPlan plan = vnr::correction_direct_plan(dims, kind, type_size, stats.data(), n_cells);
    std::printf("file %d\n", i - 1);
    if (plan.refused) {
      if (!plan.cells.empty() || !plan.places.empty() || plan.n_groups || plan.n_words) return 3;
      std::printf("refused\n");
      continue;
    }
    if (plan.cells.size() != plan.places.size()) return 3;
    std::printf("cells %zu groups %llu words %llu\n", plan.cells.size(), (unsigned long long)plan.n_groups, (unsigned long long)plan.n_words);
    for (size_t c = 0; c < plan.cells.size(); ++c)
      std::printf("e %u %u %llu %llu %llu\n", plan.cells[c].cell, plan.cells[c].width, (unsigned long long)plan.places[c].grid_group0,
                  (unsigned long long)plan.places[c].group0, (unsigned long long)plan.places[c].word0);
  }
  return 0;
}
