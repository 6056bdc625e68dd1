// ingest.hip — in-situ ground truth: typed voxels that already live in device memory -> the volume's normalised fp32 buffer.
//
// The device twin of normalise_volume / convert_chunk (volume.hip): the same two passes (min/max of the data when no range
// is given, then convert + normalise), the same IEEE operations per voxel, so the result equals the host path bit for bit.
// Both passes are pure streaming kernels over one traversal (for_each_voxel): the source is a set of contiguous runs
// (one run for a dense array, one per x-row for an array with ghost layers), every run is read in 16-byte pieces cut at the
// 16-byte boundaries of the SOURCE address, and the ragged head and tail of a run are read element by element.  An array
// with an x stride other than 1 takes a plain per-voxel gather.  All element indices are 64-bit.
#include "volume.h"

#include <algorithm>
#include <limits>

namespace vnr {

namespace {

constexpr int kIngestBlock = 256;

// how the source is walked: n_runs runs of run_len contiguous elements; run r starts at element (r % runs_y) * sy + (r / runs_y) * sz
// of the source and at element r * run_len of the (dense) destination.  sx != 1: no runs, one voxel at a time.
struct IngestLayout {
  uint64_t nx, ny, nz;
  int64_t sx, sy, sz;
  uint64_t run_len, n_runs, runs_y;
  uint64_t pieces_per_run;   // 1 (the head) + the 16-byte pieces that cover the rest of the longest run
  bool gather;
};

template <typename T> struct PieceOf { static constexpr int n = 16 / (int)sizeof(T); };

// Calls f.piece(const T (&v)[N], dst_index) for every whole 16-byte piece and f.one(T v, dst_index) for every other voxel.
template <typename T, typename F>
__device__ __forceinline__ void for_each_voxel(const T* __restrict__ src, const IngestLayout& L, F& f)
{
  constexpr int N = PieceOf<T>::n;
  if (L.gather) {
    const uint64_t n = L.nx * L.ny * L.nz;
    for (uint64_t i = (uint64_t)blockIdx.x * kIngestBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kIngestBlock) {
      const uint64_t x = i % L.nx, yz = i / L.nx, y = yz % L.ny, z = yz / L.ny;
      f.one(src[(int64_t)x * L.sx + (int64_t)y * L.sy + (int64_t)z * L.sz], i);
    }
    return;
  }
  // one work item = kIngestBlock consecutive pieces of the flattened (run, piece) space; a block strides over the items
  const uint64_t P = L.pieces_per_run;
  const uint64_t n_items = (L.n_runs * P + kIngestBlock - 1) / kIngestBlock;
  for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    const uint64_t g0 = item * kIngestBlock;      // block-uniform: the division below is done once per item
    uint64_t r = g0 / P;
    uint64_t p = g0 - r * P + threadIdx.x;
    if (P >= (uint64_t)kIngestBlock) { if (p >= P) { p -= P; ++r; } }
    else { const uint32_t dr = (uint32_t)p / (uint32_t)P; p -= (uint64_t)dr * P; r += dr; }
    if (r >= L.n_runs) continue;
    uint64_t ry, rz;
    if (L.n_runs <= 0xffffffffull) { rz = (uint32_t)r / (uint32_t)L.runs_y; ry = (uint32_t)r - (uint32_t)rz * (uint32_t)L.runs_y; }
    else { rz = r / L.runs_y; ry = r - rz * L.runs_y; }
    const T* run = src + ((int64_t)ry * L.sy + (int64_t)rz * L.sz);
    const uint64_t dst0 = r * L.run_len;
    // elements in front of the first 16-byte boundary of this run (the source is aligned to its element size)
    const uint64_t head = std::min<uint64_t>(((16u - (uint32_t)((uintptr_t)run & 15u)) & 15u) / (uint32_t)sizeof(T), L.run_len);
    if (p == 0) {
      for (uint64_t e = 0; e < head; ++e) f.one(run[e], dst0 + e);
      continue;
    }
    const uint64_t e0 = head + (p - 1) * N;
    if (e0 >= L.run_len) continue;
    if (e0 + N <= L.run_len) {
      struct alignas(16) Piece { T v[N]; };
      const Piece pc = *reinterpret_cast<const Piece*>(run + e0);
      f.piece(pc.v, dst0 + e0);
    } else {
      for (uint64_t e = e0; e < L.run_len; ++e) f.one(run[e], dst0 + e);
    }
  }
}

// ---- pass 1: min / max in the native type (exact), partials as double -------------------------------------------------------------
template <typename T>
struct MinMaxOp {
  T mn = std::numeric_limits<T>::max(), mx = std::numeric_limits<T>::lowest();
  // the host's std::min(mn, v) / std::max(mx, v): the running value stays unless v is strictly beyond it
  __device__ __forceinline__ void one(T v, uint64_t) { mn = v < mn ? v : mn; mx = mx < v ? v : mx; }
  __device__ __forceinline__ void piece(const T (&v)[PieceOf<T>::n], uint64_t)
  {
#pragma unroll
    for (int j = 0; j < PieceOf<T>::n; ++j) one(v[j], 0);
  }
};

__device__ __forceinline__ void block_reduce_minmax(double& mn, double& mx)
{
  for (int off = 32; off > 0; off >>= 1) {
    const double a = __shfl_down(mn, off, 64), b = __shfl_down(mx, off, 64);
    mn = a < mn ? a : mn; mx = mx < b ? b : mx;
  }
  __shared__ double wave_mn[kIngestBlock / 64], wave_mx[kIngestBlock / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { wave_mn[wave] = mn; wave_mx[wave] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kIngestBlock / 64; ++w) { mn = wave_mn[w] < mn ? wave_mn[w] : mn; mx = mx < wave_mx[w] ? wave_mx[w] : mx; }
  }
}

template <typename T>
__global__ void __launch_bounds__(kIngestBlock) ingest_minmax_kernel(const T* __restrict__ src, IngestLayout L, double* __restrict__ partials)
{
  MinMaxOp<T> op;
  for_each_voxel<T>(src, L, op);
  double mn = (double)op.mn, mx = (double)op.mx;
  block_reduce_minmax(mn, mx);
  if (threadIdx.x == 0) { partials[2 * (uint64_t)blockIdx.x] = mn; partials[2 * (uint64_t)blockIdx.x + 1] = mx; }
}

// second stage: one block over the block partials; out[0] = min, out[1] = max
__global__ void __launch_bounds__(kIngestBlock) ingest_minmax_final_kernel(const double* __restrict__ partials, uint32_t n, double* __restrict__ out)
{
  double mn = 1e300, mx = -1e300;   // the host's neutral elements (convert_chunk)
  for (uint32_t i = threadIdx.x; i < n; i += kIngestBlock) {
    const double a = partials[2 * (uint64_t)i], b = partials[2 * (uint64_t)i + 1];
    mn = a < mn ? a : mn; mx = mx < b ? b : mx;
  }
  block_reduce_minmax(mn, mx);
  if (threadIdx.x == 0) { out[0] = mn; out[1] = mx; }
}

// ---- pass 2: convert + normalise, the arithmetic of convert_chunk ----------------------------------------------------------------------
__device__ __forceinline__ float normalise_one(float f, float lo, float width)
{
  const float nv = (f - lo) / width;   // neural_sampler.cpp:176-210 convert_volume; a correctly rounded division (no fast-math)
  return nv < 0.0f ? 0.0f : (nv > 1.0f ? 1.0f : nv);
}

template <typename T>
struct ConvertOp {
  float* __restrict__ dst;
  float lo, width;
  __device__ __forceinline__ void one(T v, uint64_t i) { dst[i] = normalise_one((float)v, lo, width); }
  __device__ __forceinline__ void piece(const T (&v)[PieceOf<T>::n], uint64_t i)
  {
    constexpr int N = PieceOf<T>::n;
    float o[N];
#pragma unroll
    for (int j = 0; j < N; ++j) o[j] = normalise_one((float)v[j], lo, width);
    if constexpr (N >= 4) {
      if ((i & 3u) == 0) {   // the destination is a hipMalloc'ed buffer: element index % 4 == 0 is 16-byte aligned
#pragma unroll
        for (int j = 0; j < N; j += 4) *reinterpret_cast<float4*>(dst + i + j) = make_float4(o[j], o[j + 1], o[j + 2], o[j + 3]);
        return;
      }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) dst[i + j] = o[j];
  }
};

template <typename T>
__global__ void __launch_bounds__(kIngestBlock) ingest_convert_kernel(const T* __restrict__ src, IngestLayout L, float* __restrict__ dst, float lo, float width)
{
  ConvertOp<T> op{dst, lo, width};
  for_each_voxel<T>(src, L, op);
}

size_t ingest_type_size(int type)
{
  switch (type) {
  case 0: case 1: return 1;
  case 2: case 3: return 2;
  case 4: case 5: case 8: return 4;
  case 12: return 8;
  case 6: case 7: throw std::runtime_error("value type " + std::to_string(type) + " (64-bit integers) is not supported for device data");
  case 9: case 10: case 11: throw std::runtime_error("value type " + std::to_string(type) + " (a vector type) is not supported for device data");
  default: throw std::runtime_error("unknown value type " + std::to_string(type));
  }
}

template <typename F>
void dispatch_type(int type, F&& f)
{
  switch (type) {
  case 0: f((const uint8_t*)nullptr); break;
  case 1: f((const int8_t*)nullptr); break;
  case 2: f((const uint16_t*)nullptr); break;
  case 3: f((const int16_t*)nullptr); break;
  case 4: f((const uint32_t*)nullptr); break;
  case 5: f((const int32_t*)nullptr); break;
  case 8: f((const float*)nullptr); break;
  case 12: f((const double*)nullptr); break;
  default: throw std::runtime_error("unknown value type " + std::to_string(type));
  }
}

IngestLayout make_layout(vec3i dims, int type, const int64_t* strides)
{
  IngestLayout L{};
  L.nx = (uint64_t)dims.x; L.ny = (uint64_t)dims.y; L.nz = (uint64_t)dims.z;
  L.sx = strides ? strides[0] : 1;
  L.sy = strides ? strides[1] : (int64_t)L.nx;
  L.sz = strides ? strides[2] : (int64_t)(L.nx * L.ny);
  L.gather = L.sx != 1;
  if (!L.gather) {
    // contiguous runs: the whole array, whole slices, or x-rows
    if (L.sy == (int64_t)L.nx && L.sz == (int64_t)(L.nx * L.ny)) { L.run_len = L.nx * L.ny * L.nz; L.n_runs = 1; L.runs_y = 1; L.sy = 0; L.sz = 0; }
    else if (L.sy == (int64_t)L.nx) { L.run_len = L.nx * L.ny; L.n_runs = L.nz; L.runs_y = 1; L.sy = 0; }
    else { L.run_len = L.nx; L.n_runs = L.ny * L.nz; L.runs_y = L.ny; }
    const uint64_t n = (uint64_t)(16 / ingest_type_size(type));
    L.pieces_per_run = 1 + (L.run_len + n - 1) / n;
  }
  return L;
}

uint32_t ingest_grid(const IngestLayout& L)
{
  const uint64_t work = L.gather ? L.nx * L.ny * L.nz : L.n_runs * L.pieces_per_run;
  const uint64_t blocks = (work + kIngestBlock - 1) / kIngestBlock;
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)Runtime::get().n_cus * 8));   // the rest by block stride
}

// first and one-past-last byte that the strided source touches
void source_extent(const DeviceSource& src, vec3i dims, const char*& lo, const char*& hi)
{
  const size_t ts = ingest_type_size(src.type);
  const int64_t sx = src.strides ? src.strides[0] : 1, sy = src.strides ? src.strides[1] : dims.x,
                sz = src.strides ? src.strides[2] : (int64_t)dims.x * dims.y;
  const unsigned __int128 last = (unsigned __int128)(dims.x - 1) * (uint64_t)sx + (unsigned __int128)(dims.y - 1) * (uint64_t)sy +
                                 (unsigned __int128)(dims.z - 1) * (uint64_t)sz;
  if ((last + 1) * ts > (unsigned __int128)INT64_MAX) throw std::runtime_error("the strides span more than 2^63 bytes");
  lo = (const char*)src.data;
  hi = lo + (size_t)((last + 1) * ts);
}

struct EventGuard {
  hipEvent_t e = nullptr;
  ~EventGuard() { if (e) (void)hipEventDestroy(e); }
};

}  // namespace

size_t device_value_type_size(int type) { return ingest_type_size(type); }

void SimpleVolume::validate_device_source(const DeviceSource& src, vec3i dims) const
{
  if (!src.data) throw std::runtime_error("null device data");
  if (dims.x <= 0 || dims.y <= 0 || dims.z <= 0)
    throw std::runtime_error("volume dimensions must be positive: " + std::to_string(dims.x) + " x " + std::to_string(dims.y) + " x " + std::to_string(dims.z));
  const size_t ts = ingest_type_size(src.type);
  if (src.strides)
    for (int a = 0; a < 3; ++a)
      if (src.strides[a] <= 0) throw std::runtime_error("strides must be positive: stride " + std::to_string(a) + " is " + std::to_string(src.strides[a]));
  if ((uintptr_t)src.data % ts != 0) throw std::runtime_error("device data is not aligned to its value type (" + std::to_string(ts) + " bytes)");
  const char *lo, *hi;
  source_extent(src, dims, lo, hi);
  auto overlaps = [&](const DeviceBuffer<float>& b) { return b.ptr && lo < (const char*)(b.ptr + b.count) && (const char*)b.ptr < hi; };
  bool own = overlaps(data_);
  for (const DeviceBuffer<float>& b : steps_) own = own || overlaps(b);
  if (own) throw std::runtime_error("device data overlaps the volume's own voxel buffer");
}

void SimpleVolume::require_resident_for_ingest(const char* what) const
{
  if (ooc_) throw std::runtime_error(std::string(what) + ": the volume is out-of-core, it has no resident voxels to replace");
  if (!data_.ptr) throw std::runtime_error(std::string(what) + ": the volume is a shape without data (mode NOTHING)");
  if (desc.dims.x <= 0 || desc.dims.y <= 0 || desc.dims.z <= 0 || data_.count != (size_t)desc.dims.x * desc.dims.y * desc.dims.z)
    throw std::runtime_error(std::string(what) + ": the volume's dims are not the ones it was created with");
}

// typed device voxels -> dst (dims.x * dims.y * dims.z normalised floats); lo > hi: the range comes from the data and is returned
void SimpleVolume::ingest_device(const DeviceSource& src, vec3i dims, float& lo, float& hi, float* dst, hipStream_t s)
{
  const IngestLayout L = make_layout(dims, src.type, src.strides);
  const uint32_t grid = ingest_grid(L);
  EventGuard ev;
  if (src.producer) {   // the data is complete once the producer's stream reaches this point
    VNR_HIP_CHECK(hipEventCreateWithFlags(&ev.e, hipEventDisableTiming));
    VNR_HIP_CHECK(hipEventRecord(ev.e, src.producer));
    VNR_HIP_CHECK(hipStreamWaitEvent(s, ev.e, 0));
  }
  if (lo > hi) {
    ingest_partials_.ensure(2 * ((size_t)grid + 1));
    double* partials = ingest_partials_.ptr;
    double* result = partials + 2 * (size_t)grid;
    dispatch_type(src.type, [&](auto* tag) {
      using T = std::remove_cv_t<std::remove_pointer_t<decltype(tag)>>;
      ingest_minmax_kernel<T><<<grid, kIngestBlock, 0, s>>>((const T*)src.data, L, partials);
    });
    VNR_HIP_CHECK(hipGetLastError());
    ingest_minmax_final_kernel<<<1, kIngestBlock, 0, s>>>(partials, grid, result);
    VNR_HIP_CHECK(hipGetLastError());
    double mm[2];
    VNR_HIP_CHECK(hipMemcpyAsync(mm, result, sizeof(mm), hipMemcpyDeviceToHost, s));
    VNR_HIP_CHECK(hipStreamSynchronize(s));
    lo = (float)mm[0]; hi = (float)mm[1];   // the host path's rounding: (float) of the double min / max
  }
  dispatch_type(src.type, [&](auto* tag) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(tag)>>;
    ingest_convert_kernel<T><<<grid, kIngestBlock, 0, s>>>((const T*)src.data, L, dst, lo, hi - lo);
  });
  VNR_HIP_CHECK(hipGetLastError());
  VNR_HIP_CHECK(hipStreamSynchronize(s));   // the caller may overwrite or free the source on return
}

void SimpleVolume::create_from_device(const DeviceSource& src, vec3i dims, float range_lo, float range_hi, float used_range[2])
{
  validate_device_source(src, dims);
  if (!Runtime::get().ready()) Runtime::get().init(-1);
  hipStream_t s = Runtime::get().stream;
  ooc_.reset();
  steps_.clear();
  current_step_ = 0;
  data_.resize((size_t)dims.x * dims.y * dims.z);
  ingest_device(src, dims, range_lo, range_hi, data_.ptr, s);
  unnormalized_lo = range_lo; unnormalized_hi = range_hi;
  desc.dims = dims; desc.type = 8; desc.range_lo = 0.0f; desc.range_hi = 1.0f;
  finish_load(s);
  if (used_range) { used_range[0] = range_lo; used_range[1] = range_hi; }
}

void SimpleVolume::update_from_device(const DeviceSource& src, float range_lo, float range_hi, float used_range[2])
{
  require_resident_for_ingest("update from device");
  validate_device_source(src, desc.dims);
  hipStream_t s = Runtime::get().stream;
  ingest_device(src, desc.dims, range_lo, range_hi, data_.ptr, s);
  if (num_timesteps() == 1) { unnormalized_lo = range_lo; unnormalized_hi = range_hi; }
  else { unnormalized_lo = std::min(unnormalized_lo, range_lo); unnormalized_hi = std::max(unnormalized_hi, range_hi); }
  // what set_current_timestep does after the switch, from a clean slate: the cells bound the new voxels only, as in a fresh volume
  if (!mc_.is_external()) { mc_.reset_value_range(s); mc_.compute_everything(data_.ptr, s); }
  if (!tfn_.empty()) mc_.update_max_opacity(tfn_.view(), s);
  VNR_HIP_CHECK(hipStreamSynchronize(s));
  if (used_range) { used_range[0] = range_lo; used_range[1] = range_hi; }
}

int SimpleVolume::append_from_device(const DeviceSource& src, float range_lo, float range_hi, float used_range[2])
{
  require_resident_for_ingest("append time step from device");
  validate_device_source(src, desc.dims);
  hipStream_t s = Runtime::get().stream;
  DeviceBuffer<float> step;
  step.resize(data_.count);
  ingest_device(src, desc.dims, range_lo, range_hi, step.ptr, s);
  if (steps_.empty()) steps_.resize(1);   // entry current_step_ stands for data_
  steps_.push_back(std::move(step));
  unnormalized_lo = std::min(unnormalized_lo, range_lo);   // like load_scene's further steps
  unnormalized_hi = std::max(unnormalized_hi, range_hi);
  if (used_range) { used_range[0] = range_lo; used_range[1] = range_hi; }
  return (int)steps_.size() - 1;
}

}  // namespace vnr
