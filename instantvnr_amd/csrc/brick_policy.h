// brick_policy.h — the inference cache's decisions, as host code that needs no HIP: WHICH levels a brick image holds within a budget
// (plan_brick_image, a pure function) and WHEN an image is built, kept and given up (BrickPolicy, a state with a handful of transitions).
// brick_cache.hip owns the memory and the build; tests/test_brick_policy_host.py runs this file alone.
#pragma once

#include <cstddef>

#include "grid_levels.h"

namespace vnr {

struct BrickPlan {
  struct Bricked { uint64_t lines; uint32_t nbx, nby, nbz; };   // 128-byte lines = bricks = nbx * nby * nbz; lines == 0: the level stays hashed
  LevelInfo levels[kMaxLevels];   // the level table with `brick` and `pad1` filled in
  Bricked bricked[kMaxLevels];
  uint32_t entries_per_line;      // 64 / F
  uint32_t mask;                  // bit l: level l is in the image
  uint64_t used;                  // lines of all bricked levels
  bool empty() const { return used == 0; }
  size_t bytes() const { return (size_t)(used + 1) * 128u; }   // + one spare line: a pair load at the last entry reads 2 entries
};

// the hashed levels no finer than `res_cap` + 1 grid points per axis (0: no cap), while they fit `budget_lines` lines (the spare one included)
BrickPlan plan_brick_image(const LevelInfo* levels, uint32_t n_levels, uint32_t F, uint32_t res_cap, uint64_t budget_lines);

// An application that trains while it renders (apps/int_dual_volume.cpp:631-672) changes the parameters after every frame.  An image
// built between two optimizer steps costs more than it saves (6.5 ms for the C4 model against 0.1 ms saved per launch), and whether the
// base threshold is reached inside one frame depends on the frame (ray parts x iterations: 12 launches for the bench frame, 27 for a
// three-part share of it).  So the threshold backs off: an image dropped before it served `kPaysAfter` launches doubles it, an
// image that lived longer resets it.
// Two tiers (round 6).  FULL: the policy above.  SMALL: while the parameters keep changing, the first large evaluation launch after a change
// (capacity >= kSmallMinLaunch samples: a frame, not a probe) builds the levels that fit the small budget, 0.25 ms for
// the bench model's 0.7 GB, which the frame's ~12 launches earn back: the reference application's loop 190 -> 200 frames/s.  A small image
// never counts towards the backoff above, and it is replaced by the full one once the parameters have been left alone.
struct BrickPolicy {
  enum Tier : int { kNone = 0, kSmall = 1, kFull = 2 };
  static constexpr uint32_t kPaysAfter = 64;
  static constexpr size_t kSmallMinLaunch = (size_t)1 << 20;

  Tier tier = kNone;            // the image launches are served from (kNone: from the parameter blob)
  bool full_refused = false;    // no level fits the full budget: not asked for again
  bool small_refused = false;   // ... the small budget (sizes do not change with the parameters)
  uint32_t stable_calls = 0;    // launches since the parameters changed that found no full image
  uint32_t served_calls = 0;    // launches served from the image
  uint32_t after_scale = 1;     // the backoff
  uint64_t builds = 0, small_builds = 0;   // full / small images whose build kernels ran
  int mode = -1;                // -1: the environment's, 0: never, 1: build at the next launch

  // launches with unchanged parameters the next full build waits for
  uint32_t after_now(uint32_t after_base) const
  {
    const uint64_t a = (uint64_t)after_base * after_scale;
    return a > 0xffffffffull ? 0xffffffffu : (uint32_t)a;
  }
  // Asked before a launch of capacity `n_max` of a model with F features per level: what to build first (kNone: nothing).
  // `env_mode`, `after_base`, `small_budget` (bytes): the process's settings (brick_cache.hip reads the environment)
  Tier before_launch(int env_mode, uint32_t after_base, size_t n_max, uint32_t F, double small_budget);
  // ... and then whether the launch reads the image (counted) or the parameter blob
  bool serve(int env_mode)
  {
    if ((mode >= 0 ? mode : env_mode) == 0 || tier == kNone) return false;
    if (served_calls < 0xffffffffu) ++served_calls;
    return true;
  }
  // The outcome of the build before_launch asked for.  An empty plan latches that tier's refusal and leaves what is served as it is (a full
  // tier that no longer fits does not take a valid small image away); `launched` false: the small image held every level of the full plan
  // and was promoted as it stands, nothing was built.
  void built(Tier asked, bool plan_empty, bool launched);
  // whether the device must be idle before an image of `new_bytes` replaces the held buffer of `held_bytes`: when the buffer is freed for another
  // size, and when it is overwritten in place while launches (of any stream) may still read it, i.e. while it is being served
  bool must_synchronise(size_t held_bytes, size_t new_bytes) const { return held_bytes != 0 && (held_bytes != new_bytes || tier != kNone); }
  void build_begins() { tier = kNone; }   // the buffer is about to be rewritten: it serves nothing until built() says so
  void parameters_changed();              // the image is stale; the backoff rule above
  void mode_changed(int m);
  void budget_changed();
  void released() { tier = kNone; stable_calls = 0; }
};

}  // namespace vnr
