// correction_budget.h — the search of a build within a byte budget (include/vnr_amd.h, "corrections to a byte budget"): the tightest
// tolerance it can find whose serialised size fits, from a callback that gives the sizes of a list of tolerances (one rate pass of
// correction.hip a call).  Host only, no HIP include (like correction_packed_format.h): tests build it with the host compiler under
// sanitizers, driven by a step function of sizes.
//
// Every step is one IEEE double operation, none contracted into an fma, so that tests/correction_rate_ref.py's budget_search gives
// the same double bit for bit:
//   round 0:  t_j = ldexp(eps_hi, -j), j = 0 .. 15, one call.  A refused entry does not fit.  t_0 does not fit: the search is refused.
//             J = the largest j with every t_i, i <= J, fitting; hi = t_J; J == 15 ends the search; otherwise lo = t_(J+1).
//   rounds 1 .. rounds:  p_i = lo + (hi - lo) * (i / 16), i = 1 .. 15, one call.  I = the smallest i with every p_i', i' >= I, fitting.
//             No I: lo = p_15.  Otherwise hi = p_I, and lo = p_(I-1) if I > 1.
// The result is hi.  Sizes do not grow with the tolerance, so this is a bisection; the prefix / suffix wording defines the outcome
// without relying on that.
#pragma once

#include <cstdint>
#include <functional>

namespace vnr {

constexpr int kCorrectionBudgetLadder = 16;      // tolerances of round 0; a later round probes one fewer
constexpr int kCorrectionBudgetMaxRounds = 8;

// sizes of n <= 16 tolerances: bytes[k] = the serialised size at eps[k], refused[k] != 0 = the build would be refused there
using CorrectionSizeFn = std::function<void(const double* eps, int n, uint64_t* bytes, int* refused)>;

struct CorrectionBudgetResult {
  double eps = 0.0;               // the chosen tolerance, hi
  uint64_t bytes = 0;             // its size
  double eps_tighter = 0.0;       // the largest tolerance probed that did not fit (NaN: there was none) and its size (0)
  uint64_t bytes_tighter = 0;
  int rate_passes = 0;            // calls of the size function
};

// throws std::runtime_error, by name: eps_hi not finite or <= 0, eps_hi * 2^-15 not a normal number, rounds outside 0 .. 8
void correction_budget_check(double eps_hi, int rounds);
// throws what correction_budget_check throws, and when eps_hi itself does not fit (the message names max_bytes, eps_hi and its size)
CorrectionBudgetResult correction_budget_search(const CorrectionSizeFn& sizes, uint64_t max_bytes, double eps_hi, int rounds);

}  // namespace vnr
