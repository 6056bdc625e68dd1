// pack_rays.h — the ray lists of the streaming marcher (render.hip) and the indexing of their survivors, as a device function so that it
// can run either as the prologue of the evaluation kernel of the same iteration (network_infer.hip: both only need what march(it) wrote,
// and the prologue costs the chain march -> evaluate -> march no launch) or, where there is no such kernel, as a kernel
// of its own behind the evaluation (ray_index_kernel).  No ray is moved: march(it + 1) is told where dense ray i lives.
#pragma once
#include "common.h"

namespace vnr {

struct RayList {  // per ray payload, SoA (RayMarchingData, method_raymarching.cu:59-93)
  uint32_t* pixel_index;
  float* jitter;
  float* alpha;
  vec3f* color;
  vec3i* cell;
  vec3f* t_next;
  float* next_cell_begin;
  uint32_t* sample_base;
  uint32_t* sample_count;
};

// SINGLE_SHADE_HEURISTIC only (inter_highest_*, method_raymarching.cu:84-87): per ray, the sample that has contributed most so
// far; [b] belongs to ray list b.  A kernel argument of its own, behind the others, so that
// the instances that never touch it do not drag it through their scalar registers: as members of RayList these six pointers
// cost the unshaded march kernel 6 more spilled SGPRs (90 -> 96) and the bench 3 % of its frame rate (A/B on one box,
// tools/ab/ab.sh, n = 3 each: 195-198 against 201-204 frames/s; 199-200 against 199-201 with this layout).
struct SshLists {
  vec3f* org[2];
  vec3f* color[2];
  float* alpha[2];
};

// device counters of one ray part (render.hip)
enum { C_RAYS0 = 0, C_RAYS1 = 1, C_SAMPLES0 = 2, C_SAMPLES1 = 3, C_HIT = 4, C_STAT_SAMPLES = 6, C_STAT_REFRAYS = 8, C_COUNT = 16 };

struct PackArgs {
  uint32_t* ray_src;             // out: dense ray index of march(it + 1) -> slot of the list march(it) left its survivors in (group g: slots 64 g ..)
  const uint32_t* ray_counts;    // per 64-ray group: survivors | rays alive when the march began to emit << 8
  uint32_t n_first;              // rays of the first march (it = 0)
  uint32_t* counters;
  int parity, first, grad;
  uint32_t* host_alive;          // pinned: alive rays after this iteration
  uint32_t* host_stats;          // pinned copy of the counters
  uint32_t item_groups;          // 64-ray groups per work item of pack_rays_block (pack_item_groups)
  uint32_t n_blocks;             // work items (pack_items); 0: nothing to index
};

// Groups per work item for a part of n_rays rays.  Every item sums the counts of all groups before it, so the items of a part read
// (items x groups / 2) counts between them: at 4 groups per item, 2 048 items x 4 096 counts on average for half the bench frame, 25 us of
// every evaluation kernel that carried them (profiles/r07_ray_index_ab.txt).  A large part takes the most one wave scan covers, 64 (128
// items for that half frame); a small one, whose evaluation kernel is a few blocks per CU and short, keeps many light items.
inline uint32_t pack_item_groups(uint32_t n_rays) { return n_rays > 262144u ? 64u : 4u; }
inline uint32_t pack_items(uint32_t n_rays) { return ((n_rays + 255u) / 256u * 4u + pack_item_groups(n_rays) - 1u) / pack_item_groups(n_rays); }

#if defined(__HIPCC__)
// Numbers the survivors march_kernel left in its list (group g holds ray_counts[g] rays in slots 64 g ..) in group order: dense ray
// base(g) + l of the next march is slot 64 g + l, one 4-byte store per survivor and no copy of its 60 bytes of state
// (88 with the single-shade lists).  A work item (a.item_groups groups, a multiple of WAVES and at most 64, dealt over the waves of one
// block of 64 WAVES threads) first sums the
// counts of all groups before it (at most 64 KiB of L2-resident counts), so no second launch and no dependency between items is
// needed.  The item that holds the last group publishes the number of alive rays; item 0 also clears the sample counter the next
// march adds to.  s_part: WAVES words of LDS; every thread of the block calls this with the same `item`.
template <int WAVES>
__device__ __forceinline__ void pack_rays_block(const PackArgs& a, uint32_t item, uint32_t* s_part)
{
  constexpr uint32_t T = 64u * WAVES;
  const uint32_t G = a.item_groups;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t* counters = a.counters;
  const int parity = a.parity;
  const uint32_t n_in = a.first ? a.n_first : counters[C_RAYS0 + parity];   // rays the march that just ran consumed
  const uint32_t n_groups = ((n_in + 255u) & ~255u) >> 6;                   // groups it wrote a count for
  if (item == 0 && tid == 0) counters[C_SAMPLES0 + (parity ^ 1)] = 0;
  // the host reads the alive-ray count and the frame statistics from pinned memory the kernel writes itself: a copy
  // engine operation between two kernels of a stream costs more than either of the small kernels
  if (n_groups == 0) {  // nothing marched: the statistics are those of the previous launch
    if (item == 0 && tid == 0) { counters[C_RAYS0 + (parity ^ 1)] = 0; *a.host_alive = 0; }
    if (item == 0 && tid >= C_HIT && tid < C_COUNT) a.host_stats[tid] = counters[tid];
    return;
  }
  const uint32_t g0 = item * G;
  if (g0 >= n_groups) return;
  const uint32_t* __restrict__ ray_counts = a.ray_counts;
  // a group's count: survivors in the low byte, rays that were alive when the march began to emit above it
  uint32_t sum = 0;
  for (uint32_t g = tid; g < g0; g += T) sum += ray_counts[g] & 0xffu;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
  if (lane == 0) s_part[wave] = sum;
  __syncthreads();
  uint32_t before = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) before += s_part[w];
  // counts of this item's groups: lane l < G of every wave holds count[g0 + l]
  const uint32_t mine = (lane < G && g0 + lane < n_groups) ? ray_counts[g0 + lane] & 0xffu : 0u;
  uint32_t incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(incl, d);
    if ((int)lane >= d) incl += y;
  }
  const uint32_t block_total = __shfl(incl, 63);
  const bool last_block = g0 + G >= n_groups;  // (block-uniform) the item that holds the last group
  if (last_block && tid == 0) { counters[C_RAYS0 + (parity ^ 1)] = before + block_total; *a.host_alive = before + block_total; }
  for (uint32_t l = wave; l < G; l += (uint32_t)WAVES) {  // (block-uniform bounds) group g0 + l: one thread per slot
    const uint32_t count = __shfl(mine, (int)l), base = before + __shfl(incl, (int)l) - count;
    if (lane < count) a.ray_src[base + lane] = ((g0 + l) << 6) + lane;
  }
  // Frame statistics of the march that just ran (it used to count them with three device-scope atomics per wave), summed by
  // the last item after its stores
  if (last_block) {
    uint32_t asum = 0;
    for (uint32_t g = tid; g < n_groups; g += T) asum += ray_counts[g] >> 8;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) asum += __shfl_xor(asum, d);
    __syncthreads();  // s_part is read above
    if (lane == 0) s_part[wave] = asum;
    __syncthreads();
    if (tid == 0) {
      uint32_t alive_total = 0;
      for (int w = 0; w < WAVES; ++w) alive_total += s_part[w];
      const uint32_t records = counters[C_SAMPLES0 + parity];
      unsigned long long* c64 = (unsigned long long*)counters;
      c64[C_STAT_SAMPLES / 2] += (unsigned long long)(a.grad ? records >> 2 : records);
      c64[C_STAT_REFRAYS / 2] += (unsigned long long)alive_total;
      if (a.first) counters[C_HIT] += alive_total;
    }
    __syncthreads();
    if (tid >= C_HIT && tid < C_COUNT) a.host_stats[tid] = ((volatile uint32_t*)counters)[tid];
  }
}
#endif

}  // namespace vnr
