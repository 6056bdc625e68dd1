// correction_budget_harness.cpp — csrc/correction_budget.cpp driven by a step function of sizes, for tests/test_correction_rate_host.py
// (built there with the host compiler under -fsanitize=address,undefined; a stand-alone program).
//
//   harness MAX_BYTES EPS_HI ROUNDS REFUSED_BELOW BASE_BYTES [THRESHOLD:BYTES ...]
// Doubles are given and printed as the 16 hex digits of their bit patterns.  size(eps) = BYTES of the step with the largest THRESHOLD
// <= eps, BASE_BYTES below every threshold; eps < REFUSED_BELOW is refused.  Prints
//   eps <bits> bytes <n> tighter <bits, or nan> bytes_tighter <n> passes <n>
// and then one line "probe <bits> ..." per call of the size function, or "refused: <message>".
#include "correction_budget.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

double from_bits(const char* s)
{
  const uint64_t b = std::strtoull(s, nullptr, 16);
  double d;
  std::memcpy(&d, &b, sizeof(d));
  return d;
}

uint64_t bits_of(double d)
{
  uint64_t b;
  std::memcpy(&b, &d, sizeof(b));
  return b;
}

struct Step { double threshold; uint64_t bytes; };

}  // namespace

int main(int argc, char** argv)
{
  if (argc < 6) { std::fprintf(stderr, "usage: %s MAX_BYTES EPS_HI ROUNDS REFUSED_BELOW BASE_BYTES [THRESHOLD:BYTES ...]\n", argv[0]); return 2; }
  const uint64_t max_bytes = std::strtoull(argv[1], nullptr, 10);
  const double eps_hi = from_bits(argv[2]);
  const int rounds = std::atoi(argv[3]);
  const double refused_below = from_bits(argv[4]);
  const uint64_t base = std::strtoull(argv[5], nullptr, 10);
  std::vector<Step> steps;
  for (int i = 6; i < argc; ++i) {
    const char* colon = std::strchr(argv[i], ':');
    if (!colon) { std::fprintf(stderr, "bad step %s\n", argv[i]); return 2; }
    steps.push_back(Step{from_bits(argv[i]), std::strtoull(colon + 1, nullptr, 10)});
  }
  std::string probes;
  try {
    const vnr::CorrectionBudgetResult r = vnr::correction_budget_search(
        [&](const double* eps, int n, uint64_t* bytes, int* refused) {
          probes += "probe";
          for (int k = 0; k < n; ++k) {
            char b[24];
            std::snprintf(b, sizeof(b), " %016" PRIx64, bits_of(eps[k]));
            probes += b;
            refused[k] = eps[k] < refused_below;
            uint64_t size = base;
            double best = -1.0;
            for (const Step& s : steps)
              if (s.threshold <= eps[k] && s.threshold > best) { best = s.threshold; size = s.bytes; }
            bytes[k] = refused[k] ? 0 : size;
          }
          probes += "\n";
        },
        max_bytes, eps_hi, rounds);
    char tighter[24] = "nan";
    if (r.eps_tighter == r.eps_tighter) std::snprintf(tighter, sizeof(tighter), "%016" PRIx64, bits_of(r.eps_tighter));
    std::printf("eps %016" PRIx64 " bytes %" PRIu64 " tighter %s bytes_tighter %" PRIu64 " passes %d\n", bits_of(r.eps), r.bytes, tighter, r.bytes_tighter,
                r.rate_passes);
    std::fputs(probes.c_str(), stdout);
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  return 0;
}
