// correction_wave.h — what the kernels of correction_pack.hip and correction_code.hip share: a group is 64 codes and a wavefront of
// gfx950 is 64 lanes, so a wave takes a group, lane l its code l; a block is one wave and walks the groups of one flagged cell.
#pragma once

#include "correction_record.h"
#include "volume.h"

namespace vnr {

constexpr int kWave = 64;
static_assert(kWave == (int)kCorrectionGroup, "a group is one wavefront");
// (cells beyond 2^20 are reached by block stride)
inline uint32_t cell_blocks(size_t n_cells) { return (uint32_t)std::min<size_t>(n_cells, 1u << 20); }

__device__ __forceinline__ uint64_t wave_or(uint64_t v)
{
  for (int off = kWave / 2; off > 0; off >>= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, off, kWave);
  return v;
}

// exclusive prefix sum over the lanes
__device__ __forceinline__ uint32_t wave_exclusive_scan(uint32_t v, uint32_t lane)
{
  uint32_t incl = v;
  for (int off = 1; off < kWave; off <<= 1) {
    const uint32_t t = __shfl_up(incl, off, kWave);
    if (lane >= (uint32_t)off) incl += t;
  }
  return incl - v;
}

}  // namespace vnr
