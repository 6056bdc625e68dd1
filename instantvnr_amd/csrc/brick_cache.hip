// brick_cache.hip — the inference cache (brick_cache.h): budget, build kernels, and the order in which an image comes to be.
#include "brick_cache.h"

#include <algorithm>
#include <cstdlib>

#include "grid_device.h"

namespace vnr {

// ------------------------------------------------------------------------------------------------ build kernels (the image: grid_levels.h)
// one thread per entry of a level's image: (brick, x-fastest position inside it) -> grid point -> the entry the reference's
// index function gives that point (level_index: hash or dense, exact `% size` semantics); points beyond the grid are zero
template <int F>
__global__ void brick_build_kernel(const LevelInfo lv, const half_t* __restrict__ table, uint8_t* __restrict__ image, uint64_t n_entries)
{
  typedef typename FeatVec<F>::type vec_t;
  constexpr uint32_t LX = BrickShape<F>::lx, LY = BrickShape<F>::ly, LZ = BrickShape<F>::lz;
  constexpr uint32_t E = 1u << (LX + LY + LZ);
  const uint32_t nbx = (lv.resolution >> LX) + 1u, nby = (lv.resolution >> LY) + 1u;
  vec_t* out = (vec_t*)(image + (size_t)(lv.brick - 1u) * 128u);
  const vec_t* src = (const vec_t*)(table + (size_t)lv.offset * F);
  if constexpr (F == 2) {   // 8 x 2 x 2 entries, column 7 = column 0 of the +x neighbour (grid_device.h gather_corners_brick)
    const uint32_t gnbx = lv.pad1, gnby = (lv.resolution >> 1) + 1u;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_entries; e += (uint64_t)gridDim.x * blockDim.x) {
      const uint32_t w = (uint32_t)(e & 31u);
      const uint64_t b = e >> 5;
      const uint32_t bx = (uint32_t)(b % gnbx), by = (uint32_t)((b / gnbx) % gnby), bz = (uint32_t)(b / ((uint64_t)gnbx * gnby));
      const uint32_t x = bx * 7u + (w & 7u), y = (by << 1) | ((w >> 3) & 1u), z = (bz << 1) | (w >> 4);
      vec_t v;
      if (x <= lv.resolution && y <= lv.resolution && z <= lv.resolution) v = src[level_index(lv, x, y, z)];
      else v = vec_t{};
      out[e] = v;
    }
    return;
  }
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_entries; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t w = (uint32_t)(e & (E - 1u));
    const uint64_t b = e >> (LX + LY + LZ);
    const uint32_t bx = (uint32_t)(b % nbx), by = (uint32_t)((b / nbx) % nby), bz = (uint32_t)(b / ((uint64_t)nbx * nby));
    const uint32_t x = (bx << LX) | (w & ((1u << LX) - 1u)), y = (by << LY) | ((w >> LX) & ((1u << LY) - 1u)), z = (bz << LZ) | (w >> (LX + LY));
    vec_t v;
    if (x <= lv.resolution && y <= lv.resolution && z <= lv.resolution) v = src[level_index(lv, x, y, z)];
    else v = vec_t{};
    out[e] = v;
  }
}

// The same image, a ROW OF BRICKS per block (round 6).  The kernel above gives every image entry a thread that de-hashes its grid point and
// gathers 2 F bytes from an unrelated line of the table: one lane address per entry, 1.3 TB/s of image (6.5 ms for the 8.8 GB of the bench
// model, 0.53 ms for the 0.7 GB an application that trains after every frame could afford per frame).  But along x the index function is
// (x ^ h(y, z)) & mask (hashed) or x + const (dense): the 64 consecutive x of a wave read ONE aligned 64-entry block of the table, permuted.
// So a block first copies its (y, z) rows -- the 2 x 2 (4 x 4 for F = 1) rows of grid points its bricks are made of, all x -- into LDS with
// those coalesced loads, and then writes its bricks entry by entry in image order: coalesced stores of whole 128-byte lines.
template <int F>
__global__ void __launch_bounds__(256) brick_build_rows_kernel(const LevelInfo lv, const half_t* __restrict__ table, uint8_t* __restrict__ image,
                                                               uint32_t nbx, uint32_t nby, uint32_t nbz)
{
  typedef typename FeatVec<F>::type vec_t;
  constexpr uint32_t LX = BrickShape<F>::lx, LY = BrickShape<F>::ly, LZ = BrickShape<F>::lz;
  constexpr uint32_t E = 1u << (LX + LY + LZ), ROWS = 1u << (LY + LZ);
  static_assert(E * F * 2 == 128, "a brick is one 128-byte line");
  extern __shared__ __attribute__((aligned(16))) uint8_t s_raw[];
  vec_t* s_rows = (vec_t*)s_raw;                       // [ROWS][res + 1]
  const uint32_t res = lv.resolution, nx = (res + 4u) & ~3u;   // row stride: whole groups of four grid points
  const vec_t* src = (const vec_t*)(table + (size_t)lv.offset * F);
  vec_t* out = (vec_t*)(image + (size_t)(lv.brick - 1u) * 128u);
  for (uint32_t row = blockIdx.x; row < nby * nbz; row += gridDim.x) {   // a row of bricks: (by, bz)
    const uint32_t by = row % nby, bz = row / nby;
    for (uint32_t r = 0; r < ROWS; ++r) {
      const uint32_t y = (by << LY) | (r & ((1u << LY) - 1u)), z = (bz << LZ) | (r >> LY);
      const bool inside = y <= res && z <= res;        // (block-uniform)
      if (F == 2 && lv.hashed == 1u && lv.size >= 4u && inside) {
        // four grid points x4 .. x4 + 3 of a hashed level are the aligned group of four entries at (x4 ^ h) & mask & ~3, permuted by the low
        // two bits of h (uniform over the row): one 16-byte load per lane
        const uint32_t h = (y * 2654435761u) ^ (z * 805459861u), mask = lv.size - 1u, hl = h & 3u;
        for (uint32_t x4 = threadIdx.x * 4u; x4 < nx; x4 += 1024u) {
          const uint4_t v = *(const uint4_t*)(src + (((x4 ^ h) & mask) & ~3u));
          uint4_t o;
          if (hl == 0u) o = v; else if (hl == 1u) o = uint4_t{v.y, v.x, v.w, v.z}; else if (hl == 2u) o = uint4_t{v.z, v.w, v.x, v.y}; else o = uint4_t{v.w, v.z, v.y, v.x};
          *(uint4_t*)(s_rows + r * nx + x4) = o;       // (grid points beyond res: read, never used)
        }
      } else {
        for (uint32_t x = threadIdx.x; x < res + 1u; x += 256u) s_rows[r * nx + x] = inside ? src[level_index(lv, x, y, z)] : vec_t{};
      }
    }
    __syncthreads();
    vec_t* dst = out + (size_t)row * nbx * E;
    if constexpr (F == 2) {   // four entries (16 bytes) per lane: columns 0..3 or 4..7 of a brick's row r
      for (uint32_t t4 = threadIdx.x; t4 < nbx * 8u; t4 += 256u) {
        const uint32_t b = t4 >> 3, r = (t4 >> 1) & 3u, x0 = b * 7u + (t4 & 1u) * 4u;   // the 8th column repeats the +x neighbour brick's first
        const uint32_t* rowp = (const uint32_t*)(s_rows + r * nx);
        uint4_t o;
        o.x = x0 <= res ? rowp[x0] : 0u;
        o.y = x0 + 1u <= res ? rowp[x0 + 1u] : 0u;
        o.z = x0 + 2u <= res ? rowp[x0 + 2u] : 0u;
        o.w = x0 + 3u <= res ? rowp[x0 + 3u] : 0u;
        *(uint4_t*)(dst + (size_t)t4 * 4u) = o;
      }
    } else {
      for (uint32_t t = threadIdx.x; t < nbx * E; t += 256u) {
        const uint32_t b = t / E, w = t % E;
        const uint32_t wx = w & ((1u << LX) - 1u), r = w >> LX;
        const uint32_t x = (b << LX) | wx;
        dst[t] = x <= res ? s_rows[r * nx + x] : vec_t{};
      }
    }
    __syncthreads();
  }
}

template <int F>
static void launch_brick_build(const LevelInfo& lv, const BrickPlan::Bricked& b, uint64_t n_entries, const uint16_t* table, uint8_t* image, hipStream_t s)
{
  const uint64_t res = lv.resolution;
  const size_t shmem = (size_t)(1u << (BrickShape<F>::ly + BrickShape<F>::lz)) * ((res + 4) & ~(uint64_t)3) * F * 2;
  if (shmem <= 64 * 1024) {
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((uint64_t)b.nby * b.nbz, 1u << 20);
    brick_build_rows_kernel<F><<<blocks, 256, shmem, s>>>(lv, (const half_t*)table, image, b.nbx, b.nby, b.nbz);
  } else {
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_entries + 255) / 256, 1u << 20);
    brick_build_kernel<F><<<blocks, 256, 0, s>>>(lv, (const half_t*)table, image, n_entries);
  }
  VNR_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ the cache
// the process's settings, read once
struct BrickEnv {
  int mode;             // VNR_AMD_BRICK: -1 auto, 0 off, 1 at once
  uint32_t after;       // VNR_AMD_BRICK_AFTER
  double small_bytes;   // VNR_AMD_BRICK_SMALL_GB (0: no small tier)
  double max_gb;        // VNR_AMD_BRICK_MAX_GB (< 0: not set)
};

static const BrickEnv& brick_env()
{
  // small tier, 0.75 GiB: swept on the bench model inside the reference application's loop (render, train one step, render ...; bench.py
  // `interactive`): none 190.1, 0.25 GiB 196.4, 0.75 GiB 200.2, 1.7 GiB 195.0 frames/s -- the build is 0.25 ms at 0.7 GB.
  static const BrickEnv env = [] {
    const char *m = std::getenv("VNR_AMD_BRICK"), *a = std::getenv("VNR_AMD_BRICK_AFTER"), *sm = std::getenv("VNR_AMD_BRICK_SMALL_GB"),
               *mx = std::getenv("VNR_AMD_BRICK_MAX_GB");
    return BrickEnv{m ? std::atoi(m) : -1, a ? (uint32_t)std::max(0, std::atoi(a)) : 24u, (sm ? std::max(0.0, std::atof(sm)) : 0.75) * 1073741824.0,
                    mx ? std::atof(mx) : -1.0};
  }();
  return env;
}

BrickCache::~BrickCache()
{
  if (t0_) { (void)hipEventDestroy(t0_); (void)hipEventDestroy(t1_); }
}

uint32_t BrickCache::after_now() const { return policy_.after_now(brick_env().after); }

void BrickCache::drop()
{
  if (Runtime::get().ready()) (void)hipDeviceSynchronize();   // nothing may still read what is freed
  image_.release();
  levels_.release();
  policy_.released();
}

void BrickCache::set_mode(int mode)
{
  policy_.mode_changed(mode);
  if (policy_.mode == 0 && in_use()) drop();   // the next launches read the parameter blob; the image's memory goes back
}

void BrickCache::set_budget(size_t bytes)
{
  budget_ = bytes;
  policy_.budget_changed();
  if (in_use()) drop();
  mask_ = 0;
}

const LevelInfo* BrickCache::levels_for_launch(const Source& source, hipStream_t s, const uint8_t** image, size_t n_max)
{
  const BrickEnv& env = brick_env();
  const BrickPolicy::Tier ask = policy_.before_launch(env.mode, env.after, n_max, source.n_features, env.small_bytes);
  if (ask != BrickPolicy::kNone) build(source, s, ask);
  const bool serve = policy_.serve(env.mode);
  *image = serve ? image_.ptr : nullptr;
  return serve ? levels_.ptr : source.levels_dev;
}

void BrickCache::build(const Source& source, hipStream_t s, BrickPolicy::Tier tier)
{
  // 1. Budget.  The image is a cache in memory nothing else of the process uses: a renderer that holds a 1024^3 fp32 volume (4.3 GB), its
  // 140 MB model and its frame buffers occupies 2 % of the 288 GB of an MI355X.  Default: 1/16 of the device's memory (18 GB), and never
  // more than a quarter of what is free when the image is built; VNR_AMD_BRICK_MAX_GB or vnrAmdNeuralVolumeSetBrickImageBudget set it.
  // What a budget buys on the bench model: profiles/r03_brick_budget_table.json.
  const BrickEnv& env = brick_env();
  size_t free_b = 0, total_b = 0;
  VNR_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  double budget = budget_ ? (double)budget_ : env.max_gb >= 0.0 ? env.max_gb * 1073741824.0 : (double)total_b / 16.0;
  // the small tier (brick_policy.h): what an application that changes the parameters after every frame can afford to rebuild per frame
  if (tier == BrickPolicy::kSmall) budget = std::min(budget, env.small_bytes);
  const uint64_t budget_lines = (uint64_t)std::min(budget, (double)(free_b + image_.bytes()) / 4.0) / 128u;
  // 2. which levels
  const BrickPlan plan = plan_brick_image(source.levels, source.n_levels, source.n_features, res_cap_, budget_lines);
  // 3. nothing to build: no level fits, or the small image of a model whose every bricked level fits the small budget IS the full image
  const bool held_as_planned = tier == BrickPolicy::kFull && in_use() && mask_ == plan.mask && image_.bytes() == plan.bytes();
  if (plan.empty() || held_as_planned) {
    policy_.built(tier, plan.empty(), false);
    return;
  }
  // 4. the buffer changes under launches that took its pointer, of this stream or another
  if (policy_.must_synchronise(image_.bytes(), plan.bytes())) VNR_HIP_CHECK(hipDeviceSynchronize());
  policy_.build_begins();
  // 5. build, on `s`
  if (!t0_) { VNR_HIP_CHECK(hipEventCreate(&t0_)); VNR_HIP_CHECK(hipEventCreate(&t1_)); }
  image_.resize(plan.bytes());
  VNR_HIP_CHECK(hipEventRecord(t0_, s));
  for (uint32_t l = 0; l < source.n_levels; ++l) {
    const BrickPlan::Bricked& b = plan.bricked[l];
    if (!b.lines) continue;
    const uint64_t n_entries = b.lines * plan.entries_per_line;
    switch (source.n_features) {
    case 1: launch_brick_build<1>(plan.levels[l], b, n_entries, source.table, image_.ptr, s); break;
    case 2: launch_brick_build<2>(plan.levels[l], b, n_entries, source.table, image_.ptr, s); break;
    case 4: launch_brick_build<4>(plan.levels[l], b, n_entries, source.table, image_.ptr, s); break;
    default: launch_brick_build<8>(plan.levels[l], b, n_entries, source.table, image_.ptr, s); break;
    }
  }
  VNR_HIP_CHECK(hipMemsetAsync(image_.ptr + plan.used * 128u, 0, 128, s));
  levels_.resize(kMaxLevels);
  // pageable host source: the copy has completed for the host when the call returns, the device side is ordered on `s`
  VNR_HIP_CHECK(hipMemcpyAsync(levels_.ptr, plan.levels, kMaxLevels * sizeof(LevelInfo), hipMemcpyHostToDevice, s));
  VNR_HIP_CHECK(hipEventRecord(t1_, s));
  VNR_HIP_CHECK(hipEventSynchronize(t1_));
  VNR_HIP_CHECK(hipEventElapsedTime(&build_ms_, t0_, t1_));
  // 6. the image serves launches from here on
  mask_ = plan.mask;
  policy_.built(tier, false, true);
}

}  // namespace vnr

