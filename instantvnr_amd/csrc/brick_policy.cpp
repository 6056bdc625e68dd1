// brick_policy.cpp — which levels the brick image holds, and when it is built (brick_policy.h).  Host code without HIP.
#include "brick_policy.h"

#include <algorithm>

namespace vnr {

BrickPlan plan_brick_image(const LevelInfo* levels, uint32_t n_levels, uint32_t F, uint32_t res_cap, uint64_t budget_lines)
{
  BrickPlan plan{};
  std::copy(levels, levels + n_levels, plan.levels);
  plan.entries_per_line = 64u / F;
  const BrickLog log = brick_log_shape(F);
  // Which levels first when not all fit.  F <= 2 (bricks of 32 / 64 entries): the FINEST, whose eight corners land in eight unrelated lines of the
  // table and whose big bricks are shared by the neighbouring samples of a wave (round 3's measurement on the bench model).  F >= 4 (bricks of
  // 16 / 8 entries, 2 x 2 x 2 cells for F = 8): the COARSEST.  A brick that small pays through neighbouring samples falling into the same
  // cells, which the coarser hashed levels give and a level as fine as the volume does not, and its image (gigabytes, read from HBM) replaces
  // a table of a few megabytes that lives in the caches: the reference's example model (L8 F8 T2^19, example-model.json) on the 1024^3 bench
  // volume, finest first = levels {3, 4, 6}, 17.6 GB, 181.9 frames/s; {3, 4, 5}, 2.5 GB: 185.4; no image 179.7 (round 6).
  const bool finest_first = F <= 2;
  for (int k = 0; k < (int)n_levels; ++k) {
    const int l = finest_first ? (int)n_levels - 1 - k : k;
    LevelInfo& lv = plan.levels[l];
    if (lv.hashed != 1u) continue;   // (dense levels are not bricked; a Tiled level repeats: nothing to de-hash)
    if (res_cap && lv.resolution > res_cap + 1u) continue;
    const uint64_t res = lv.resolution;
    BrickPlan::Bricked b{0, (uint32_t)(res >> log.lx) + 1u, (uint32_t)(res >> log.ly) + 1u, (uint32_t)(res >> log.lz) + 1u};
    if (F == 2) {   // the brick with a repeated column: 7 useful columns (grid_device.h gather_corners_brick)
      if (res >= 13000) continue;   // (x * 9363) >> 16 is x / 7 below 13 107
      b.nbx = (uint32_t)(res / 7 + 1);
    }
    b.lines = (uint64_t)b.nbx * b.nby * b.nbz;
    if (b.lines * plan.entries_per_line >= (1ull << 32) || plan.used + b.lines + 1 > budget_lines || plan.used + b.lines + 1 >= 0xffffffffull) continue;
    if (F == 2) lv.pad1 = b.nbx;
    lv.brick = (uint32_t)plan.used + 1u;
    plan.bricked[l] = b;
    plan.used += b.lines;
    plan.mask |= 1u << l;
  }
  return plan;
}

BrickPolicy::Tier BrickPolicy::before_launch(int env_mode, uint32_t after_base, size_t n_max, uint32_t F, double small_budget)
{
  const int m = mode >= 0 ? mode : env_mode;
  if (m == 0 || full_refused || tier == kFull) return kNone;
  if (stable_calls < 0xffffffffu) ++stable_calls;
  if (m == 1 || stable_calls > after_now(after_base)) return kFull;
  // (big bricks only: with the 2 x 2 x 2 bricks of F = 8 a per-frame image earns less than its build -- the reference's example model on the
  // bench volume: 171.0 frames/s with it, 172.9 without, round 6)
  if (tier == kNone && !small_refused && n_max >= kSmallMinLaunch && small_budget > 0.0 && F <= 2u) return kSmall;
  return kNone;
}

void BrickPolicy::built(Tier asked, bool plan_empty, bool launched)
{
  if (plan_empty) {
    (asked == kFull ? full_refused : small_refused) = true;   // (nothing fits the small tier: the full one is still tried when its time comes)
    return;
  }
  tier = asked;
  if (asked == kFull) served_calls = 0;
  if (launched) ++(asked == kFull ? builds : small_builds);
}

void BrickPolicy::parameters_changed()
{
  if (tier == kFull) after_scale = served_calls < kPaysAfter ? std::min<uint32_t>(after_scale * 2u, 1u << 16) : 1u;
  tier = kNone;
  stable_calls = 0;
  served_calls = 0;
}

void BrickPolicy::mode_changed(int m)
{
  mode = m < 0 ? -1 : (m > 0 ? 1 : 0);
  full_refused = small_refused = false;
  stable_calls = 0;
}

void BrickPolicy::budget_changed()
{
  full_refused = small_refused = false;
  stable_calls = 0;
}

}  // namespace vnr
