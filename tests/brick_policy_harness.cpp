// Stand-alone driver of csrc/brick_policy.{h,cpp} for tests/test_brick_policy_host.py: reads a script (argv[1]) of plan cases and policy
// transitions and prints what the library answers.  Built with the address / undefined-behaviour sanitizers; no HIP, no GPU.
//
//   plan F res_cap budget_lines n_levels        then n_levels lines "resolution size offset hashed"
//     -> "plan used U mask M bytes B", then per level "  l brick pad1 lines nbx nby nbz"
//   policy env_mode after_base small_budget     a fresh policy with these process settings
//   launch n_max F outcome                      one launch; outcome of the build it may ask for: ok | empty | shortcut
//     -> "launch ask A serve S" + the state
//   params | mode M | budget | released         the other transitions -> the state
//   sync held_bytes new_bytes                   -> "sync 0|1"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "brick_policy.h"

using namespace vnr;

static BrickPolicy policy;
static int env_mode = -1;
static uint32_t after_base = 24;
static double small_budget = 0.0;

static void state()
{
  std::printf(" tier %d stable %u served %u scale %u after %u builds %" PRIu64 " small_builds %" PRIu64 " refused %d %d mode %d\n", (int)policy.tier,
              policy.stable_calls, policy.served_calls, policy.after_scale, policy.after_now(after_base), policy.builds, policy.small_builds,
              (int)policy.full_refused, (int)policy.small_refused, policy.mode);
}

int main(int argc, char** argv)
{
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string op;
    if (!(ss >> op)) continue;
    if (op == "plan") {
      uint32_t F, cap, n;
      uint64_t budget;
      ss >> F >> cap >> budget >> n;
      if (!ss || n > (uint32_t)kMaxLevels) return 3;
      LevelInfo* lv = new LevelInfo[n]();   // exactly n: reading past them is the sanitizer's to find
      for (uint32_t l = 0; l < n; ++l) {
        std::getline(in, line);
        std::istringstream ls(line);
        ls >> lv[l].resolution >> lv[l].size >> lv[l].offset >> lv[l].hashed;
        if (!ls) return 3;
        lv[l].res2 = lv[l].resolution * lv[l].resolution;
      }
      const BrickPlan p = plan_brick_image(lv, n, F, cap, budget);
      std::printf("plan used %" PRIu64 " mask %u bytes %zu empty %d epl %u\n", p.used, p.mask, p.bytes(), (int)p.empty(), p.entries_per_line);
      for (uint32_t l = 0; l < n; ++l) {
        if (p.levels[l].resolution != lv[l].resolution || p.levels[l].size != lv[l].size || p.levels[l].offset != lv[l].offset || p.levels[l].hashed != lv[l].hashed) return 4;
        std::printf("  %u %u %u %" PRIu64 " %u %u %u\n", l, p.levels[l].brick, p.levels[l].pad1, p.bricked[l].lines, p.bricked[l].lines ? p.bricked[l].nbx : 0u,
                    p.bricked[l].lines ? p.bricked[l].nby : 0u, p.bricked[l].lines ? p.bricked[l].nbz : 0u);
      }
      delete[] lv;
    } else if (op == "policy") {
      ss >> env_mode >> after_base >> small_budget;
      if (!ss) return 3;
      policy = BrickPolicy();
      std::printf("policy");
      state();
    } else if (op == "launch") {
      uint64_t n_max;
      uint32_t F;
      std::string outcome;
      ss >> n_max >> F >> outcome;
      if (!ss) return 3;
      const BrickPolicy::Tier ask = policy.before_launch(env_mode, after_base, (size_t)n_max, F, small_budget);
      if (ask != BrickPolicy::kNone) {   // what brick_cache.hip does with the answer
        if (outcome == "empty") policy.built(ask, true, false);
        else if (outcome == "shortcut") policy.built(ask, false, false);
        else { policy.build_begins(); policy.built(ask, false, true); }
      }
      const bool serve = policy.serve(env_mode);
      std::printf("launch ask %d serve %d", (int)ask, (int)serve);
      state();
    } else if (op == "params") { policy.parameters_changed(); std::printf("params"); state(); }
    else if (op == "mode") { int m; ss >> m; if (!ss) return 3; policy.mode_changed(m); std::printf("mode"); state(); }
    else if (op == "budget") { policy.budget_changed(); std::printf("budget"); state(); }
    else if (op == "released") { policy.released(); std::printf("released"); state(); }
    else if (op == "sync") {
      uint64_t held, nb;
      ss >> held >> nb;
      if (!ss) return 3;
      std::printf("sync %d\n", (int)policy.must_synchronise((size_t)held, (size_t)nb));
    } else return 3;
  }
  return 0;
}
