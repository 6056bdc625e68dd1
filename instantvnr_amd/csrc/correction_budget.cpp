// correction_budget.cpp — see correction_budget.h
#include "correction_budget.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>

namespace vnr {

namespace {

std::string num(double v)
{
  char b[40];
  std::snprintf(b, sizeof(b), "%.17g", v);
  return b;
}

// one call of the size function; notes the largest tolerance that did not fit
struct Prober {
  const CorrectionSizeFn& sizes;
  uint64_t max_bytes;
  CorrectionBudgetResult& r;
  uint64_t bytes[kCorrectionBudgetLadder];
  bool fits[kCorrectionBudgetLadder];

  void probe(const double* eps, int n)
  {
    int refused[kCorrectionBudgetLadder];
    for (int k = 0; k < n; ++k) { bytes[k] = 0; refused[k] = 0; }
    sizes(eps, n, bytes, refused);
    ++r.rate_passes;
    for (int k = 0; k < n; ++k) {
      fits[k] = !refused[k] && bytes[k] <= max_bytes;
      if (!fits[k] && !(eps[k] <= r.eps_tighter)) { r.eps_tighter = eps[k]; r.bytes_tighter = bytes[k]; }   // (a NaN so far: the first)
    }
  }
};

}  // namespace

void correction_budget_check(double eps_hi, int rounds)
{
  if (!std::isfinite(eps_hi) || !(eps_hi > 0.0)) throw std::runtime_error("eps_hi must be a finite tolerance > 0 in data units, got " + num(eps_hi));
  if (!std::isnormal(std::ldexp(eps_hi, -(kCorrectionBudgetLadder - 1))))
    throw std::runtime_error("eps_hi * 2^-15 must be a normal number, eps_hi is " + num(eps_hi));
  if (rounds < 0 || rounds > kCorrectionBudgetMaxRounds) throw std::runtime_error("rounds must be 0 .. 8, got " + std::to_string(rounds));
}

CorrectionBudgetResult correction_budget_search(const CorrectionSizeFn& sizes, uint64_t max_bytes, double eps_hi, int rounds)
{
  correction_budget_check(eps_hi, rounds);
  CorrectionBudgetResult r;
  r.eps_tighter = std::numeric_limits<double>::quiet_NaN();
  Prober p{sizes, max_bytes, r};

  // round 0: the ladder
  double t[kCorrectionBudgetLadder];
  for (int j = 0; j < kCorrectionBudgetLadder; ++j) t[j] = std::ldexp(eps_hi, -j);   // exact
  p.probe(t, kCorrectionBudgetLadder);
  if (!p.fits[0])
    throw std::runtime_error("the correction does not fit max_bytes " + std::to_string(max_bytes) + " at eps_hi " + num(eps_hi) + ": its size there is " +
                             std::to_string(p.bytes[0]) + " bytes" + (p.bytes[0] <= max_bytes ? " (the build is refused there)" : ""));
  int J = 0;
  while (J + 1 < kCorrectionBudgetLadder && p.fits[J + 1]) ++J;
  double hi = t[J], lo = 0.0;
  uint64_t hi_bytes = p.bytes[J];
  const bool bracket = J + 1 < kCorrectionBudgetLadder;
  if (bracket) lo = t[J + 1];

  // the refinement: 15 points inside (lo, hi)
  for (int round = 1; bracket && round <= rounds; ++round) {
    constexpr int n = kCorrectionBudgetLadder - 1;
    double pt[n];
    for (int i = 1; i <= n; ++i) {
      const volatile double d = hi - lo;              // (volatile: each step is rounded to double on its own, whatever the compiler's flags)
      const volatile double f = (double)i / 16.0;     // exact
      const volatile double m = d * f;
      pt[i - 1] = lo + m;
    }
    p.probe(pt, n);
    int I = n + 1;   // the smallest i with every p_i', i' >= I, fitting; n + 1: none
    while (I > 1 && p.fits[I - 2]) --I;
    if (I == n + 1) { lo = pt[n - 1]; continue; }
    hi = pt[I - 1]; hi_bytes = p.bytes[I - 1];
    if (I > 1) lo = pt[I - 2];
  }
  r.eps = hi;
  r.bytes = hi_bytes;
  if (r.eps_tighter != r.eps_tighter) r.bytes_tighter = 0;
  return r;
}

}  // namespace vnr
