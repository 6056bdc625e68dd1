// grid_levels.h — the per-level constants of the hash grid and the shape of a brick of its inference cache: plain data, no HIP
// (network.h builds on it; brick_policy.h and its host-only test need nothing else).
#pragma once

#include <cstdint>

namespace vnr {

constexpr int kMaxLevels = 32;

struct LevelInfo {
  float scale;
  uint32_t resolution;
  uint32_t res2;    // resolution^2 (dense index stride of z)
  uint32_t size;    // entries in this level
  uint32_t offset;  // first entry of this level (entries, x F for elements)
  uint32_t hashed;  // 0: dense index, 1: prime-XOR hash (size is a power of two), 2 / 3 / 4: Tiled grid, index over 1 / 2 / 3 dimensions modulo size
  uint32_t brick;   // 0: read the parameter blob; else 1 + first 128-byte line of this level in the brick image (below)
  uint32_t pad1;    // bricked levels with F = 2: bricks per row of the image (resolution / 7 + 1); else 0.  32 bytes: one s_load_dwordx8 per level
};

// Brick image (inference only): a level whose table is hashed is ALSO kept de-hashed, as a dense array over the level's
// (res + 1)^3 grid points stored in bricks of one 128-byte line: 4x4x4 entries for F = 1, 4x2x2 for F = 4, 2x2x2 for F = 8, and
// for F = 2 8x2x2 entries of which the 8th column repeats the +x neighbour's first (grid_device.h: a cell's x-pairs never straddle).  The values are copies (image[x, y, z] = table[hash(x, y, z)]), so results are bit-identical; what changes
// is which lines a wave touches: the 8 corners of a cell fall into ~2.3 lines instead of 4-8 and neighbouring samples share
// them, where the hash scatters every (y, z) row to an unrelated line (measured on the bench frame's sample queue: 917 -> 385
// fetched bytes per sample inside a 64-sample wave).  The price is memory, 8.8 GB instead of 140 MB for the bench model,
// which is what 288 GB of HBM are for, and a rebuild (a few ms) after the parameters change, so the image is only built once
// the parameters have been left alone for a while (brick_policy.h).
// log2 of a brick's extent along x, y, z: stated here once, for the sizing (brick_policy.cpp), the build (brick_cache.hip) and the reads (grid_device.h)
struct BrickLog { uint32_t lx, ly, lz; };
constexpr BrickLog brick_log_shape(uint32_t F) { return F == 1 ? BrickLog{2, 2, 2} : F == 2 ? BrickLog{3, 1, 1} : F == 4 ? BrickLog{2, 1, 1} : BrickLog{1, 1, 1}; }
template <int F> struct BrickShape {
  static_assert(F == 1 || F == 2 || F == 4 || F == 8, "features per level");
  static constexpr uint32_t lx = brick_log_shape(F).lx, ly = brick_log_shape(F).ly, lz = brick_log_shape(F).lz;
};

}  // namespace vnr
