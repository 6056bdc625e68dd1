// guided_sampler.hip — error-guided training batches: a per-macrocell weight map -> a sampling table, and the weighted draw.
//
// The table is integer work from end to end so that it can be restated bit for bit (include/vnr_amd.h spells the definition out):
// a validation pass (unsigned max over the float bits, a flag for NaN / infinity / negative entries), a 24-bit quantisation in
// double, and an inclusive uint64 prefix sum in cell order.  The sum is a hierarchical device scan: every block of kScanBlock
// cells scans itself (wave shuffles, one partial per wave) and leaves its total, the totals are scanned the same way, level by
// level until one block holds them all, and the offsets are added on the way back down.  Integer addition is associative: the
// result does not depend on the block size or on the number of levels.
//
// The draw (take_samples_weighted_kernel) is one lane per sample: six draws of the sampler's pcg32 stream, an upper-bound binary
// search of the CDF, three fp32 roundings per coordinate, then the trilinear lookup of take_samples_kernel.  The search is latency
// bound (up to 21 dependent loads for 2 Mi cells); optionally a block first stages an evenly strided top of the CDF (<= 1024
// entries, 8 KiB) in LDS, searches that, and finishes the remaining <= log2(stride) steps from global memory.  Same bits either way.
#include "volume.h"

#include <algorithm>
#include <cstdlib>

#include "pcg32_device.h"
#include "sampling_device.h"

namespace vnr {

namespace {

constexpr int kScanBlock = 256;        // cells per scan block, one per lane
constexpr int kDrawBlock = 256;
constexpr uint32_t kTopEntries = 1024; // the staged top of the CDF: at most this many entries

// ---- pass 1: wmax and the invalid flag ------------------------------------------------------------------------------------------------
// out[0] = max over the float bits of the entries without a sign bit (an unsigned max orders non-negative floats), out[1] != 0 iff an
// entry is a NaN, an infinity or negative.  -0.0f counts as zero.  Both zeroed by the caller.
__global__ void __launch_bounds__(kScanBlock) weights_validate_kernel(const float* __restrict__ w, uint64_t n, uint32_t* __restrict__ out)
{
  uint32_t mx = 0, bad = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kScanBlock) {
    const uint32_t bits = __float_as_uint(w[i]);
    const uint32_t mag = bits & 0x7fffffffu;
    if (mag >= 0x7f800000u || ((bits >> 31) && mag != 0u)) bad = 1u;   // inf / NaN of either sign; a negative value
    else if (mag > mx) mx = mag;
  }
  for (int off = 32; off > 0; off >>= 1) {
    mx = max(mx, (uint32_t)__shfl_down((int)mx, off, 64));
    bad |= (uint32_t)__shfl_down((int)bad, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (mx) atomicMax(&out[0], mx);
    if (bad) atomicOr(&out[1], 1u);
  }
}

// ---- pass 2: quantise + scan -------------------------------------------------------------------------------------------------------------
// q = (uint64) rint(((double)w / (double)wmax) * 2^24), ties to even; a positive weight never quantises to 0
__device__ __forceinline__ uint64_t quantise_weight(float w, double wmax)
{
  const uint32_t mag = __float_as_uint(w) & 0x7fffffffu;
  if (mag == 0u) return 0ull;
  const uint64_t q = (uint64_t)rint(((double)w / wmax) * 16777216.0);
  return q ? q : 1ull;
}

// inclusive scan over the block's kScanBlock lanes; total = the block's sum (on every lane)
__device__ __forceinline__ uint64_t block_inclusive_scan(uint64_t v, uint64_t& total)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t t = (uint64_t)__shfl_up((unsigned long long)v, off, 64);
    if (lane >= off) v += t;
  }
  __shared__ uint64_t wave_sum[kScanBlock / 64];
  if (lane == 63) wave_sum[wave] = v;
  __syncthreads();
  uint64_t before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kScanBlock / 64; ++k) {
    const uint64_t s = wave_sum[k];
    if (k < wave) before += s;
    all += s;
  }
  total = all;
  return v + before;
}

__global__ void __launch_bounds__(kScanBlock) quantise_scan_kernel(const float* __restrict__ w, uint64_t n, double wmax, uint64_t* __restrict__ cdf,
                                                                  uint64_t* __restrict__ block_sums)
{
  const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
  uint64_t total;
  const uint64_t s = block_inclusive_scan(i < n ? quantise_weight(w[i], wmax) : 0ull, total);
  if (i < n) cdf[i] = s;
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// in place, one level up: the block sums of the level below
__global__ void __launch_bounds__(kScanBlock) scan_sums_kernel(uint64_t* __restrict__ data, uint64_t n, uint64_t* __restrict__ block_sums)
{
  const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
  uint64_t total;
  const uint64_t s = block_inclusive_scan(i < n ? data[i] : 0ull, total);
  if (i < n) data[i] = s;
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// on the way down: every block but the first adds the (final) inclusive sum of the blocks before it
__global__ void __launch_bounds__(kScanBlock) scan_add_offsets_kernel(uint64_t* __restrict__ data, uint64_t n, const uint64_t* __restrict__ scanned_sums)
{
  const uint64_t i = (uint64_t)(blockIdx.x + 1u) * kScanBlock + threadIdx.x;
  if (i < n) data[i] += scanned_sums[blockIdx.x];
}

// ---- the draw --------------------------------------------------------------------------------------------------------------------------------
struct GuidedTable {
  const uint64_t* cdf;
  uint64_t total, threshold;
  uint32_t n_cells, cells_x, cells_y;
  uint32_t top_shift, top_count;   // staged search: entry j of the top is cdf[min(((j + 1) << top_shift) - 1, n_cells - 1)]
};

// p = fminf(fl(fl((float)lo + fl(u * (float)size)) * rdim), 1 - 2^-24): three fp32 roundings, never an fma
__device__ __forceinline__ float cell_coordinate(uint32_t cell, int dim, float rdim, float u)
{
  const int lo = (int)(cell << kMacrocellSizeMip);
  const int size = min(kMacrocellSize, dim - lo);
  return fminf(__fmul_rn(__fadd_rn((float)lo, __fmul_rn(u, (float)size)), rdim), 0x1.fffffep-1f);
}

template <bool kStaged>
__global__ void __launch_bounds__(kDrawBlock) take_samples_weighted_kernel(uint64_t n, uint64_t seed, uint64_t stream, uint64_t offset, GuidedTable t,
                                                                          const float* __restrict__ vol, vec3i dims, vec3f rdims,
                                                                          float* __restrict__ coords, float* __restrict__ values)
{
  __shared__ uint64_t s_top[kStaged ? kTopEntries : 1];
  if (kStaged) {
    for (uint32_t j = threadIdx.x; j < t.top_count; j += kDrawBlock) {
      const uint64_t e = (((uint64_t)j + 1u) << t.top_shift) - 1u;
      s_top[j] = t.cdf[e < t.n_cells ? e : t.n_cells - 1u];
    }
    __syncthreads();
  }
  const uint64_t i = (uint64_t)blockIdx.x * kDrawBlock + threadIdx.x;
  if (i >= n) return;
  Pcg32Dev rng(seed, stream);
  rng.advance(offset + 6ull * i);
  const uint32_t s = rng.next_uint();
  const uint32_t r_hi = rng.next_uint(), r_lo = rng.next_uint();
  const float ux = rng.next_float(), uy = rng.next_float(), uz = rng.next_float();
  float px = ux, py = uy, pz = uz;
  if ((uint64_t)s >= t.threshold) {
    // k < total = cdf[n_cells - 1]: the first cell whose cdf exceeds k exists, and it is never a cell with q = 0
    const uint64_t k = __umul64hi(((uint64_t)r_hi << 32) | r_lo, t.total);
    uint32_t lo = 0, hi = t.n_cells - 1u;
    if (kStaged) {
      uint32_t a = 0, b = t.top_count - 1u;
      while (a < b) {
        const uint32_t m = (a + b) >> 1;
        if (s_top[m] > k) b = m; else a = m + 1u;
      }
      lo = a << t.top_shift;
      hi = min(((a + 1u) << t.top_shift) - 1u, t.n_cells - 1u);
    }
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (t.cdf[mid] > k) hi = mid; else lo = mid + 1u;
    }
    const uint32_t cx = lo % t.cells_x, cyz = lo / t.cells_x, cy = cyz % t.cells_y, cz = cyz / t.cells_y;
    px = cell_coordinate(cx, dims.x, rdims.x, ux);
    py = cell_coordinate(cy, dims.y, rdims.y, uy);
    pz = cell_coordinate(cz, dims.z, rdims.z, uz);
  }
  coords[3 * i + 0] = px; coords[3 * i + 1] = py; coords[3 * i + 2] = pz;
  values[i] = tex3d(vol, dims, px, py, pz);
}

// where the runtime knows the allocation a pointer lies in, an array that does not fit it is refused (as decode.hip does for its boxes)
void require_room(const void* p, size_t bytes, const char* what)
{
  void* base = nullptr; size_t size = 0;
  if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)p) != hipSuccess || !base || !size) {
    (void)hipGetLastError();   // not a pointer the runtime can place: taken as given
    return;
  }
  const size_t room = (size_t)((const char*)base + size - (const char*)p);
  if (bytes > room)
    throw std::runtime_error(std::string(what) + " span " + std::to_string(bytes) + " bytes from their device pointer, the allocation has " + std::to_string(room) + " left");
}

uint64_t blocks_of(uint64_t n) { return (n + kScanBlock - 1) / kScanBlock; }

bool staged_search_wanted()
{
  const char* e = std::getenv("VNR_AMD_GUIDED_LDS");
  return e ? std::atoi(e) != 0 : true;
}

}  // namespace

void device_inclusive_scan(uint64_t* d_data, uint64_t n, DeviceBuffer<uint64_t>& scratch, hipStream_t s)
{
  if (n == 0) return;
  std::vector<uint64_t> counts{n};
  while (counts.back() > 1) counts.push_back(blocks_of(counts.back()));
  size_t words = 1;   // (a one-element scan still needs a place for its block sum)
  for (size_t l = 1; l < counts.size(); ++l) words += counts[l];
  scratch.ensure(words);
  std::vector<uint64_t*> level{d_data};
  {
    uint64_t* p = scratch.ptr;
    for (size_t l = 1; l < counts.size(); ++l) { level.push_back(p); p += counts[l]; }
    if (counts.size() == 1) level.push_back(p);
  }
  for (size_t l = 0; l < std::max<size_t>(1, counts.size() - 1); ++l) {   // every level but the last one-element one scans itself
    scan_sums_kernel<<<(uint32_t)blocks_of(counts[l]), kScanBlock, 0, s>>>(level[l], counts[l], level[l + 1]);
    VNR_HIP_CHECK(hipGetLastError());
  }
  for (size_t l = counts.size(); l-- > 0;) {   // a level of one block is final as it stands
    if (counts[l] <= (uint64_t)kScanBlock) continue;
    scan_add_offsets_kernel<<<(uint32_t)(blocks_of(counts[l]) - 1), kScanBlock, 0, s>>>(level[l], counts[l], level[l + 1]);
    VNR_HIP_CHECK(hipGetLastError());
  }
}

void SimpleVolume::check_uniform_fraction(float uniform_fraction)
{
  if (!(uniform_fraction >= 0.0f && uniform_fraction <= 1.0f))
    throw std::runtime_error("uniform_fraction must lie in [0, 1], got " + std::to_string(uniform_fraction));
}

void SimpleVolume::set_sampling_weights(const float* d_weights, float uniform_fraction, hipStream_t producer)
{
  check_uniform_fraction(uniform_fraction);
  require_resident_for_ingest("set sampling weights");
  // the draws in flight that may still read the old table: on the library's stream, or on a stream a caller drew on (a stream that
  // has been destroyed since holds no work: its error is not one)
  auto wait_for_draws = [&]() {
    VNR_HIP_CHECK(hipStreamSynchronize(Runtime::get().stream));
    for (hipStream_t t : table_streams_)
      if (hipStreamSynchronize(t) != hipSuccess) (void)hipGetLastError();
    table_streams_.clear();
  };
  if (!d_weights) {
    wait_for_draws();
    table_ = SamplingTable{};
    return;
  }
  const vec3i cells = {(desc.dims.x + kMacrocellSize - 1) / kMacrocellSize, (desc.dims.y + kMacrocellSize - 1) / kMacrocellSize,
                       (desc.dims.z + kMacrocellSize - 1) / kMacrocellSize};
  const uint64_t n = (uint64_t)cells.x * cells.y * cells.z;
  if (n >= (1ull << 32)) throw std::runtime_error("set sampling weights: more than 2^32 macrocells");
  require_room(d_weights, n * sizeof(float), "set sampling weights: the weights (one float per macrocell)");
  hipStream_t s = Runtime::get().stream;
  struct EventGuard {
    hipEvent_t e = nullptr;
    ~EventGuard() { if (e) (void)hipEventDestroy(e); }
  } ev;
  if (producer) {   // the weights are complete once the producer's stream reaches this point
    VNR_HIP_CHECK(hipEventCreateWithFlags(&ev.e, hipEventDisableTiming));
    VNR_HIP_CHECK(hipEventRecord(ev.e, producer));
    VNR_HIP_CHECK(hipStreamWaitEvent(s, ev.e, 0));
  }
  // the levels of the scan: level 0 is the CDF itself, level l + 1 holds the block sums of level l, down to one element
  std::vector<uint64_t> counts{n};
  while (counts.back() > 1) counts.push_back(blocks_of(counts.back()));
  size_t scratch = 1;   // the validation pass's two words
  for (size_t l = 1; l < counts.size(); ++l) scratch += counts[l];
  table_scratch_.ensure(scratch + 1);   // (+ 1: a one-cell table still needs a place for its block sum)
  uint32_t* d_check = (uint32_t*)table_scratch_.ptr;
  VNR_HIP_CHECK(hipMemsetAsync(d_check, 0, 2 * sizeof(uint32_t), s));
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks_of(n), (uint64_t)Runtime::get().n_cus * 8));
  weights_validate_kernel<<<grid, kScanBlock, 0, s>>>(d_weights, n, d_check);
  VNR_HIP_CHECK(hipGetLastError());
  uint32_t check[2];
  VNR_HIP_CHECK(hipMemcpyAsync(check, d_check, sizeof(check), hipMemcpyDeviceToHost, s));
  VNR_HIP_CHECK(hipStreamSynchronize(s));
  if (check[1]) throw std::runtime_error("set sampling weights: the weights hold a NaN, an infinity or a negative value");
  if (check[0] == 0) throw std::runtime_error("set sampling weights: all weights are zero");
  float wmax;
  std::memcpy(&wmax, &check[0], sizeof(wmax));

  SamplingTable fresh;
  fresh.cdf.resize(n);
  std::vector<uint64_t*> level{fresh.cdf.ptr};
  {
    uint64_t* p = table_scratch_.ptr + 1;
    for (size_t l = 1; l < counts.size(); ++l) { level.push_back(p); p += counts[l]; }
    if (counts.size() == 1) level.push_back(p);
  }
  quantise_scan_kernel<<<(uint32_t)blocks_of(n), kScanBlock, 0, s>>>(d_weights, n, (double)wmax, level[0], level[1]);
  VNR_HIP_CHECK(hipGetLastError());
  for (size_t l = 1; l + 1 < counts.size(); ++l) {
    scan_sums_kernel<<<(uint32_t)blocks_of(counts[l]), kScanBlock, 0, s>>>(level[l], counts[l], level[l + 1]);
    VNR_HIP_CHECK(hipGetLastError());
  }
  for (size_t l = counts.size(); l-- > 0;) {   // a level of one block is final as it stands
    if (counts[l] <= (uint64_t)kScanBlock) continue;
    scan_add_offsets_kernel<<<(uint32_t)(blocks_of(counts[l]) - 1), kScanBlock, 0, s>>>(level[l], counts[l], level[l + 1]);
    VNR_HIP_CHECK(hipGetLastError());
  }
  VNR_HIP_CHECK(hipMemcpyAsync(&fresh.total, fresh.cdf.ptr + (n - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  VNR_HIP_CHECK(hipStreamSynchronize(s));   // the table is complete; the caller may overwrite or free the weights
  fresh.n_cells = n;
  fresh.cells = cells;
  fresh.uniform_fraction = uniform_fraction;
  fresh.threshold = (uint64_t)std::rint((double)uniform_fraction * 4294967296.0);
  fresh.staged = staged_search_wanted();
  wait_for_draws();   // draws in flight may still read the old table
  table_ = std::move(fresh);
}

void SimpleVolume::take_samples_weighted(float* d_coords, float* d_values, size_t n, hipStream_t s)
{
  if (!has_sampling_table()) throw std::runtime_error("take weighted samples: the volume has no sampling weights (vnrAmdSimpleVolumeSetSamplingWeights)");
  if (!data_.ptr) throw std::runtime_error("take weighted samples: the volume has no resident voxels");
  if (n == 0) return;
  if (!d_coords || !d_values) throw std::runtime_error("take weighted samples: null output");
  if (n > (1ull << 31)) throw std::runtime_error("take weighted samples: more than 2^31 samples in one call");
  const vec3i d = desc.dims;
  const vec3i cells = {(d.x + kMacrocellSize - 1) / kMacrocellSize, (d.y + kMacrocellSize - 1) / kMacrocellSize, (d.z + kMacrocellSize - 1) / kMacrocellSize};
  if (cells.x != table_.cells.x || cells.y != table_.cells.y || cells.z != table_.cells.z)
    throw std::runtime_error("take weighted samples: the volume's dims are not the ones the sampling weights were set for");
  GuidedTable t{};
  t.cdf = table_.cdf.ptr;
  t.total = table_.total;
  t.threshold = table_.threshold;
  t.n_cells = (uint32_t)table_.n_cells;
  t.cells_x = (uint32_t)cells.x;
  t.cells_y = (uint32_t)cells.y;
  while (((table_.n_cells + (1ull << t.top_shift) - 1) >> t.top_shift) > kTopEntries) ++t.top_shift;
  t.top_count = (uint32_t)((table_.n_cells + (1ull << t.top_shift) - 1) >> t.top_shift);
  const vec3f rdims = {1.0f / (float)d.x, 1.0f / (float)d.y, 1.0f / (float)d.z};   // in fp32 on the host, as the decode's coordinates
  const uint32_t blocks = (uint32_t)((n + kDrawBlock - 1) / kDrawBlock);
  if (table_.staged)
    take_samples_weighted_kernel<true><<<blocks, kDrawBlock, 0, s>>>(n, rng_seed_, rng_stream_, rng_offset_, t, data_.ptr, d, rdims, d_coords, d_values);
  else
    take_samples_weighted_kernel<false><<<blocks, kDrawBlock, 0, s>>>(n, rng_seed_, rng_stream_, rng_offset_, t, data_.ptr, d, rdims, d_coords, d_values);
  VNR_HIP_CHECK(hipGetLastError());
  rng_offset_ += 6ull * n;
  if (s != Runtime::get().stream && std::find(table_streams_.begin(), table_streams_.end(), s) == table_streams_.end()) table_streams_.push_back(s);
}

void NeuralVolume::guide_sampling_by_error(float uniform_fraction, DecodeError* report)
{
  SimpleVolume::check_uniform_fraction(uniform_fraction);
  if (!source_ || !source_->has_data()) throw std::runtime_error("guide sampling by error: the neural volume has no resident ground truth");
  const vec3i mcd = mc_.dims(), sd = source_->dims();
  if (sd.x != desc.dims.x || sd.y != desc.dims.y || sd.z != desc.dims.z || mcd.x != (sd.x + kMacrocellSize - 1) / kMacrocellSize ||
      mcd.y != (sd.y + kMacrocellSize - 1) / kMacrocellSize || mcd.z != (sd.z + kMacrocellSize - 1) / kMacrocellSize)
    throw std::runtime_error("guide sampling by error: the neural volume's grid is not the ground truth's");
  DeviceBuffer<float> map(MemTag::Network);
  map.resize((size_t)mcd.x * mcd.y * mcd.z);
  DecodeError r{};
  error_against_device(DeviceSource{source_->d_data(), 8, nullptr, nullptr}, nullptr, nullptr, 1.0f, 0.0f, &r, map.ptr);   // returns after the map is complete
  if (report) *report = r;
  source_->set_sampling_weights(map.ptr, uniform_fraction, nullptr);
}

}  // namespace vnr
