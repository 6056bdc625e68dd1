// decode.hip — in-situ round trip: a trained neural volume -> typed voxels in the application's own device array, and the error of
// exactly those voxels against a field in device memory.  The mirror of ingest.hip.
//
// Both calls walk a box of a voxel grid in chunks of linear box indices (x fastest): a coordinate kernel writes the voxel centres of
// the chunk (the arithmetic of generate_coords_kernel, volume.hip), Network::inference evaluates them into the volume's scratch, and
// one streaming kernel consumes the chunk: decode_store_kernel converts and stores it, decode_error_kernel converts it, reads the
// reference and reduces the difference -- the decoded box never exists.  The user's array is a set of contiguous runs (one for a
// dense box, one per x-row for an array with ghost layers); the part of a run inside the chunk is accessed in 16-byte pieces cut at
// the 16-byte boundaries of the ARRAY's address, its ragged head and tail element by element, so a store never touches a byte
// outside the box and the result does not depend on where the chunks end.  An x stride other than 1 goes voxel by voxel.  All
// element indices are 64-bit.
#include "volume.h"

#include <algorithm>
#include <cstdlib>
#include <limits>
#include <type_traits>

namespace vnr {

namespace {

constexpr int kDecodeBlock = 256;
// samples per chunk (VNR_AMD_DECODE_CHUNK): 4 Mi samples = 64 MiB of scratch (12 B of coordinates + 4 B of values each); at 512^3 the
// 32 chunks cost 3 launches each, and a launch of this size fills every CU some hundred times over
constexpr uint64_t kDefaultChunk = 1ull << 22, kMaxChunk = 1ull << 28;

// how the user's array is walked: runs of run_len contiguous elements; run r starts at element (r % runs_y) * sy + (r / runs_y) * sz and
// holds the box's linear indices [r * run_len, (r + 1) * run_len).  sx != 1: no runs, one voxel at a time.
struct BoxLayout {
  uint64_t bx, by, bz;
  int64_t sx, sy, sz;
  uint64_t run_len, runs_y;
  bool gather;
};

template <typename T> struct PieceOf { static constexpr int n = 16 / (int)sizeof(T); };

// For the linear box indices [b, e): f.piece(T* p, i) for every whole 16-byte piece (p 16-byte aligned, N voxels from index i on)
// and f.one(T* p, i) for every other voxel.  T is const-qualified for a source.
template <typename T, typename F>
__device__ __forceinline__ void for_each_chunk_voxel(T* base, const BoxLayout& L, uint64_t b, uint64_t e, F& f)
{
  constexpr int N = PieceOf<std::remove_const_t<T>>::n;
  if (L.gather) {
    for (uint64_t i = b + (uint64_t)blockIdx.x * kDecodeBlock + threadIdx.x; i < e; i += (uint64_t)gridDim.x * kDecodeBlock) {
      const uint64_t x = i % L.bx, yz = i / L.bx, y = yz % L.by, z = yz / L.by;
      f.one(base + ((int64_t)x * L.sx + (int64_t)y * L.sy + (int64_t)z * L.sz), i);
    }
    return;
  }
  const uint64_t r0 = b / L.run_len, r1 = (e - 1) / L.run_len;   // the runs this chunk touches
  // per run: 1 (the head) + the 16-byte pieces that cover the longest part a run can have inside this chunk
  const uint64_t P = 1 + (std::min(L.run_len, e - b) + N - 1) / N, work = (r1 - r0 + 1) * P;
  for (uint64_t g = (uint64_t)blockIdx.x * kDecodeBlock + threadIdx.x; g < work; g += (uint64_t)gridDim.x * kDecodeBlock) {
    uint64_t r, p;
    if (work <= 0xffffffffull) { const uint32_t q = (uint32_t)g / (uint32_t)P; r = r0 + q; p = (uint32_t)g - q * (uint32_t)P; }
    else { const uint64_t q = g / P; r = r0 + q; p = g - q * P; }
    const uint64_t run_first = r * L.run_len;
    const uint64_t lo = std::max(b, run_first), hi = std::min(e, run_first + L.run_len);   // the run's part inside the chunk
    const uint64_t len = hi - lo;
    uint64_t ry, rz;
    if (r <= 0xffffffffull) { rz = (uint32_t)r / (uint32_t)L.runs_y; ry = (uint32_t)r - (uint32_t)rz * (uint32_t)L.runs_y; }
    else { rz = r / L.runs_y; ry = r - rz * L.runs_y; }
    T* part = base + ((int64_t)ry * L.sy + (int64_t)rz * L.sz + (int64_t)(lo - run_first));
    // elements in front of the first 16-byte boundary of this part (the array is aligned to its element size)
    const uint64_t head = std::min<uint64_t>(((16u - (uint32_t)((uintptr_t)part & 15u)) & 15u) / (uint32_t)sizeof(T), len);
    if (p == 0) {
      for (uint64_t k = 0; k < head; ++k) f.one(part + k, lo + k);
      continue;
    }
    const uint64_t e0 = head + (p - 1) * N;
    if (e0 >= len) continue;
    if (e0 + N <= len) f.piece(part + e0, lo + e0);
    else for (uint64_t k = e0; k < len; ++k) f.one(part + k, lo + k);
  }
}

// ---- the conversion: network output -> the typed voxel.  Every step is one IEEE operation (include/vnr_amd.h spells them out) --------
struct Conversion {
  float lo, width;   // d = v * width + lo, two roundings
  bool scale;        // false: d = v
};

template <typename T>
__device__ __forceinline__ T convert_value(float v, const Conversion& c)
{
  const float d = c.scale ? __fadd_rn(__fmul_rn(v, c.width), c.lo) : v;
  if constexpr (std::is_same_v<T, float>) return d;
  else if constexpr (std::is_same_v<T, double>) return (double)d;
  else {
    const double r = rint((double)d);   // ties to even
    constexpr double tmin = (double)std::numeric_limits<T>::lowest(), tmax = (double)std::numeric_limits<T>::max();
    if (r != r) return (T)0;
    return r <= tmin ? std::numeric_limits<T>::lowest() : (r >= tmax ? std::numeric_limits<T>::max() : (T)r);
  }
}

// voxel centres of the box's linear indices [b, b + n): generate_coords_kernel's arithmetic with a 64-bit index
__global__ void __launch_bounds__(kDecodeBlock) decode_coords_kernel(uint64_t b, uint32_t n, uint64_t bx, uint64_t by, vec3i lower, vec3f rdims,
                                                                     float* __restrict__ coords)
{
  const uint32_t t = blockIdx.x * kDecodeBlock + threadIdx.x;
  if (t >= n) return;
  const uint64_t i = b + t, yz = i / bx;
  const int x = lower.x + (int)(i - yz * bx), y = lower.y + (int)(yz % by), z = lower.z + (int)(yz / by);
  coords[3 * (size_t)t + 0] = ((float)x + 0.5f) * rdims.x;
  coords[3 * (size_t)t + 1] = ((float)y + 0.5f) * rdims.y;
  coords[3 * (size_t)t + 2] = ((float)z + 0.5f) * rdims.z;
}

// ---- decode: convert + store ------------------------------------------------------------------------------------------------------------
template <typename T>
struct StoreOp {
  const float* __restrict__ values;   // values[i - b]
  uint64_t b;
  Conversion c;
  __device__ __forceinline__ void one(T* p, uint64_t i) { *p = convert_value<T>(values[i - b], c); }
  __device__ __forceinline__ void piece(T* p, uint64_t i)
  {
    constexpr int N = PieceOf<T>::n;
    struct alignas(16) Piece { T v[N]; } pc;
    const float* v = values + (i - b);
#pragma unroll
    for (int j = 0; j < N; ++j) pc.v[j] = convert_value<T>(v[j], c);
    *reinterpret_cast<Piece*>(p) = pc;   // one 16-byte vector store
  }
};

template <typename T>
__global__ void __launch_bounds__(kDecodeBlock) decode_store_kernel(T* __restrict__ dst, BoxLayout L, uint64_t b, uint64_t e, const float* __restrict__ values,
                                                                    Conversion c)
{
  StoreOp<T> op{values, b, c};
  for_each_chunk_voxel<T>(dst, L, b, e, op);
}

// ---- error report: convert, compare, reduce -----------------------------------------------------------------------------------------------
struct ErrorPartial {
  double max_abs;      // -1: no voxel yet (every |e| is >= 0)
  uint64_t worst;      // linear box index of max_abs, the lowest one among equals
  double sum_abs, sum_sq;
};

struct BlockMap {
  uint32_t* cells;     // float bit patterns: the order of non-negative floats is the order of their bits
  vec3i lower;         // box_lo in grid indices
  int mcx, mcy;
};

template <typename T>
struct ErrorOp {
  const float* __restrict__ values;
  uint64_t b;
  Conversion c;
  uint64_t bx, by;
  BlockMap map;
  double mx = -1.0, sum_abs = 0.0, sum_sq = 0.0;
  uint64_t mi = ~0ull;
  uint32_t cell = 0xffffffffu;   // the cell whose maximum is pending in cell_bits
  uint32_t cell_bits = 0;

  __device__ __forceinline__ void flush()
  {
    // the map only ever grows, so a stale read can only be too small: the atomic is skipped when it could not raise the cell
    if (cell != 0xffffffffu && cell_bits > map.cells[cell]) atomicMax(map.cells + cell, cell_bits);
    cell_bits = 0;
  }
  __device__ __forceinline__ void voxel(T ref, uint64_t i, uint32_t x, uint32_t y, uint32_t z)
  {
    const double err = (double)convert_value<T>(values[i - b], c) - (double)ref;
    const double a = fabs(err);
    sum_abs += a;
    sum_sq += err * err;
    if (a > mx) { mx = a; mi = i; }   // (i only grows inside a lane: the first of equals stays; a NaN never wins)
    if (map.cells && a == a) {
      const uint32_t cl = (uint32_t)((map.lower.x + (int)x) >> 4) +
                          (uint32_t)map.mcx * ((uint32_t)((map.lower.y + (int)y) >> 4) + (uint32_t)map.mcy * (uint32_t)((map.lower.z + (int)z) >> 4));
      if (cl != cell) { flush(); cell = cl; }
      float af = (float)a;   // round to nearest
      cell_bits = std::max(cell_bits, __float_as_uint(af));
    }
  }
  __device__ __forceinline__ void split(uint64_t i, uint32_t& x, uint32_t& y, uint32_t& z) const
  {
    const uint64_t yz = i / bx;
    x = (uint32_t)(i - yz * bx); y = (uint32_t)(yz % by); z = (uint32_t)(yz / by);
  }
  __device__ __forceinline__ void one(const T* p, uint64_t i)
  {
    uint32_t x, y, z;
    split(i, x, y, z);
    voxel(*p, i, x, y, z);
  }
  __device__ __forceinline__ void piece(const T* p, uint64_t i)
  {
    constexpr int N = PieceOf<T>::n;
    struct alignas(16) Piece { T v[N]; };
    const Piece pc = *reinterpret_cast<const Piece*>(p);   // one 16-byte vector load
    uint32_t x, y, z;
    split(i, x, y, z);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      voxel(pc.v[j], i + j, x, y, z);
      if (++x == (uint32_t)bx) { x = 0; if (++y == (uint32_t)by) { y = 0; ++z; } }   // (a dense box: a piece may run over the end of a row)
    }
  }
};

// (max, lowest index) and the two sums over the block: inside the wave by shuffles, then one value per wave through the LDS
__device__ __forceinline__ void block_reduce_error(double& mx, uint64_t& mi, double& sa, double& sq)
{
  for (int off = 32; off > 0; off >>= 1) {
    const double omx = __shfl_down(mx, off, 64);
    const uint64_t omi = (uint64_t)__shfl_down((unsigned long long)mi, off, 64);
    sa += __shfl_down(sa, off, 64);
    sq += __shfl_down(sq, off, 64);
    if (omx > mx || (omx == mx && omi < mi)) { mx = omx; mi = omi; }
  }
  __shared__ double w_mx[kDecodeBlock / 64], w_sa[kDecodeBlock / 64], w_sq[kDecodeBlock / 64];
  __shared__ uint64_t w_mi[kDecodeBlock / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { w_mx[wave] = mx; w_mi[wave] = mi; w_sa[wave] = sa; w_sq[wave] = sq; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kDecodeBlock / 64; ++w) {
      if (w_mx[w] > mx || (w_mx[w] == mx && w_mi[w] < mi)) { mx = w_mx[w]; mi = w_mi[w]; }
      sa += w_sa[w]; sq += w_sq[w];
    }
  }
}

__global__ void __launch_bounds__(kDecodeBlock) decode_error_init_kernel(ErrorPartial* __restrict__ partials, uint32_t n)
{
  const uint32_t i = blockIdx.x * kDecodeBlock + threadIdx.x;
  if (i < n) partials[i] = ErrorPartial{-1.0, ~0ull, 0.0, 0.0};
}

// one partial per block; the launches of one report run one behind the other on one stream, so block k owns partials[k] throughout
template <typename T>
__global__ void __launch_bounds__(kDecodeBlock) decode_error_kernel(const T* __restrict__ ref, BoxLayout L, uint64_t b, uint64_t e,
                                                                    const float* __restrict__ values, Conversion c, BlockMap map,
                                                                    ErrorPartial* __restrict__ partials)
{
  ErrorOp<T> op{values, b, c, L.bx, L.by, map};
  for_each_chunk_voxel<const T>(ref, L, b, e, op);
  if (map.cells) op.flush();
  block_reduce_error(op.mx, op.mi, op.sum_abs, op.sum_sq);
  if (threadIdx.x == 0) {
    ErrorPartial p = partials[blockIdx.x];
    if (op.mx > p.max_abs || (op.mx == p.max_abs && op.mi < p.worst)) { p.max_abs = op.mx; p.worst = op.mi; }
    p.sum_abs += op.sum_abs; p.sum_sq += op.sum_sq;
    partials[blockIdx.x] = p;
  }
}

// second stage: one block over the block partials
__global__ void __launch_bounds__(kDecodeBlock) decode_error_final_kernel(const ErrorPartial* __restrict__ partials, uint32_t n, ErrorPartial* __restrict__ out)
{
  double mx = -1.0, sa = 0.0, sq = 0.0;
  uint64_t mi = ~0ull;
  for (uint32_t i = threadIdx.x; i < n; i += kDecodeBlock) {
    const ErrorPartial p = partials[i];
    if (p.max_abs > mx || (p.max_abs == mx && p.worst < mi)) { mx = p.max_abs; mi = p.worst; }
    sa += p.sum_abs; sq += p.sum_sq;
  }
  block_reduce_error(mx, mi, sa, sq);
  if (threadIdx.x == 0) *out = ErrorPartial{mx, mi, sa, sq};
}

template <typename F>
void dispatch_type(int type, F&& f)
{
  switch (type) {
  case 0: f((uint8_t*)nullptr); break;
  case 1: f((int8_t*)nullptr); break;
  case 2: f((uint16_t*)nullptr); break;
  case 3: f((int16_t*)nullptr); break;
  case 4: f((uint32_t*)nullptr); break;
  case 5: f((int32_t*)nullptr); break;
  case 8: f((float*)nullptr); break;
  case 12: f((double*)nullptr); break;
  default: throw std::runtime_error("unknown value type " + std::to_string(type));
  }
}

std::string str3(const int v[3]) { return std::to_string(v[0]) + " x " + std::to_string(v[1]) + " x " + std::to_string(v[2]); }

// where the runtime knows the allocation a pointer lies in, what the call will touch must fit into it
void require_room(const void* p, size_t bytes, const char* what)
{
  void* base = nullptr; size_t size = 0;
  if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)p) != hipSuccess || !base || !size) {
    (void)hipGetLastError();   // not a pointer the runtime can place: taken as given
    return;
  }
  const size_t room = (size_t)((const char*)base + size - (const char*)p);
  if (bytes > room)
    throw std::runtime_error(std::string(what) + " spans " + std::to_string(bytes) + " bytes from its device pointer, the allocation has " + std::to_string(room) + " left");
}

// everything a call is refused for, before the first kernel; returns the layout of the box in the user's array
BoxLayout validate_box_array(const void* data, int type, const int64_t* strides, const int box_lo[3], const int box_size[3], vec3i grid, vec3i& lower, vec3i& size,
                             float range_lo, float range_hi)
{
  if (!data) throw std::runtime_error("null device data");
  const size_t ts = device_value_type_size(type);   // refuses the 64-bit integer and the vector types like the ingest
  if (grid.x <= 0 || grid.y <= 0 || grid.z <= 0)
    throw std::runtime_error("grid dimensions must be positive: " + std::to_string(grid.x) + " x " + std::to_string(grid.y) + " x " + std::to_string(grid.z));
  if ((box_lo == nullptr) != (box_size == nullptr)) throw std::runtime_error("box_lo and box_size go together: both or neither");
  lower = box_lo ? vec3i{box_lo[0], box_lo[1], box_lo[2]} : vec3i{0, 0, 0};
  size = box_size ? vec3i{box_size[0], box_size[1], box_size[2]} : grid;
  if (size.x <= 0 || size.y <= 0 || size.z <= 0) throw std::runtime_error("box sizes must be positive: " + str3(box_size));
  if (lower.x < 0 || lower.y < 0 || lower.z < 0 || (int64_t)lower.x + size.x > grid.x || (int64_t)lower.y + size.y > grid.y || (int64_t)lower.z + size.z > grid.z)
    throw std::runtime_error("the box (lower " + str3(box_lo) + ", size " + str3(box_size) + ") is outside the grid " + std::to_string(grid.x) + " x " +
                             std::to_string(grid.y) + " x " + std::to_string(grid.z));
  const bool integer = type != 8 && type != 12;
  if (!(range_lo < range_hi) && !(range_lo > range_hi)) throw std::runtime_error("range_lo == range_hi (or a NaN): an empty value range");
  if (integer && range_lo > range_hi) throw std::runtime_error("an integer value type needs a value range (range_lo < range_hi)");

  BoxLayout L{};
  L.bx = (uint64_t)size.x; L.by = (uint64_t)size.y; L.bz = (uint64_t)size.z;
  L.sx = strides ? strides[0] : 1;
  L.sy = strides ? strides[1] : (int64_t)L.bx;
  L.sz = strides ? strides[2] : (int64_t)(L.bx * L.by);
  const int64_t s[3] = {L.sx, L.sy, L.sz};
  const uint64_t n[3] = {L.bx, L.by, L.bz};
  for (int a = 0; a < 3; ++a)
    if (s[a] <= 0) throw std::runtime_error("strides must be positive: stride " + std::to_string(a) + " is " + std::to_string(s[a]));
  // no two voxels of the box at one address: the axes longer than one voxel, ordered by stride, must nest (each stride at least the
  // extent of the axis below it).  This refuses a few exotic layouts that do not overlap; it accepts every array with ghost layers,
  // every sub-box and every transposition of them.
  int order[3] = {0, 1, 2};
  std::sort(order, order + 3, [&](int a, int b) { return s[a] < s[b]; });
  unsigned __int128 extent = 1, last = 0;   // elements the axes so far span; offset of the last voxel
  for (int k = 0; k < 3; ++k) {
    const int a = order[k];
    if (n[a] == 1) continue;
    if ((unsigned __int128)s[a] < extent)
      throw std::runtime_error("the strides (" + std::to_string(L.sx) + ", " + std::to_string(L.sy) + ", " + std::to_string(L.sz) +
                               ") overlap: two voxels of the box would share an address");
    extent = (unsigned __int128)s[a] * (n[a] - 1) + extent;
  }
  for (int a = 0; a < 3; ++a) last += (unsigned __int128)s[a] * (n[a] - 1);
  if ((last + 1) * ts > (unsigned __int128)INT64_MAX) throw std::runtime_error("the strides span more than 2^63 bytes");
  if ((uintptr_t)data % ts != 0) throw std::runtime_error("device data is not aligned to its value type (" + std::to_string(ts) + " bytes)");
  require_room(data, (size_t)((last + 1) * ts), "the box");

  L.gather = L.sx != 1;
  if (!L.gather) {
    // contiguous runs: the whole box, whole slices, or x-rows
    if (L.sy == (int64_t)L.bx && L.sz == (int64_t)(L.bx * L.by)) { L.run_len = L.bx * L.by * L.bz; L.runs_y = 1; L.sy = 0; L.sz = 0; }
    else if (L.sy == (int64_t)L.bx) { L.run_len = L.bx * L.by; L.runs_y = 1; L.sy = 0; }
    else { L.run_len = L.bx; L.runs_y = L.by; }
  }
  return L;
}

// launch width for the chunk [b, e): its pieces of work (for_each_chunk_voxel), the rest by block stride
uint32_t chunk_grid(const BoxLayout& L, int type, uint64_t b, uint64_t e)
{
  uint64_t work = e - b;
  if (!L.gather) {
    const uint64_t per = 16 / device_value_type_size(type);
    work = ((e - 1) / L.run_len - b / L.run_len + 1) * (1 + (std::min(L.run_len, e - b) + per - 1) / per);
  }
  const uint64_t blocks = (work + kDecodeBlock - 1) / kDecodeBlock;
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)Runtime::get().n_cus * 8));
}

uint64_t chunk_samples()
{
  uint64_t c = kDefaultChunk;
  if (const char* e = std::getenv("VNR_AMD_DECODE_CHUNK")) {
    char* end = nullptr;
    const unsigned long long v = std::strtoull(e, &end, 10);
    if (end == e || *end != '\0' || v == 0) throw std::runtime_error(std::string("VNR_AMD_DECODE_CHUNK must be a positive sample count, got '") + e + "'");
    c = std::min<uint64_t>(v, kMaxChunk);
  }
  return c;
}

struct EventGuard {
  hipEvent_t e = nullptr;
  ~EventGuard() { if (e) (void)hipEventDestroy(e); }
};

// the library's stream waits for what the caller's stream holds at this point; the caller's stream is not touched otherwise
void wait_for(hipStream_t theirs, hipStream_t ours, EventGuard& ev)
{
  if (!theirs) return;
  VNR_HIP_CHECK(hipEventCreateWithFlags(&ev.e, hipEventDisableTiming));
  VNR_HIP_CHECK(hipEventRecord(ev.e, theirs));
  VNR_HIP_CHECK(hipStreamWaitEvent(ours, ev.e, 0));
}

}  // namespace

void NeuralVolume::decode_chunk(uint64_t b, uint32_t n, uint64_t bx, uint64_t by, vec3i lower, vec3f rdims, float* d_values)
{
  decode_coords_kernel<<<div_round_up(n, kDecodeBlock), kDecodeBlock, 0, stream>>>(b, n, bx, by, lower, rdims, dd_coords_.ptr);
  VNR_HIP_CHECK(hipGetLastError());
  net_.inference(dd_coords_.ptr, d_values, n, nullptr, n, stream);
}

void NeuralVolume::decode_to_device(const DeviceTarget& out, const int box_lo[3], const int box_size[3], const int grid_dims[3], float range_lo, float range_hi)
{
  if (!net_.valid()) throw std::runtime_error("neural volume has no valid network");
  const vec3i grid = grid_dims ? vec3i{grid_dims[0], grid_dims[1], grid_dims[2]} : desc.dims;
  vec3i lower, size;
  const BoxLayout L = validate_box_array(out.data, out.type, out.strides, box_lo, box_size, grid, lower, size, range_lo, range_hi);
  const uint64_t total = L.bx * L.by * L.bz, chunk = std::min(chunk_samples(), total);
  const vec3f rdims = {1.0f / (float)grid.x, 1.0f / (float)grid.y, 1.0f / (float)grid.z};
  const Conversion c{range_lo, range_hi - range_lo, range_lo < range_hi};
  // a dense float32 box without a range is the network's output as it stands: the inference writes into the destination
  const bool direct = out.type == 8 && !c.scale && !L.gather && L.run_len == total;
  dd_coords_.ensure(3 * chunk);
  if (!direct) dd_values_.ensure(chunk);
  EventGuard ev;
  wait_for(out.consumer, stream, ev);   // what the destination held may still be being read
  for (uint64_t b = 0; b < total; b += chunk) {
    const uint64_t e = std::min(total, b + chunk);
    decode_chunk(b, (uint32_t)(e - b), L.bx, L.by, lower, rdims, direct ? (float*)out.data + b : dd_values_.ptr);
    if (direct) continue;
    const uint32_t blocks = chunk_grid(L, out.type, b, e);
    dispatch_type(out.type, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      decode_store_kernel<T><<<blocks, kDecodeBlock, 0, stream>>>((T*)out.data, L, b, e, dd_values_.ptr, c);
    });
    VNR_HIP_CHECK(hipGetLastError());
  }
  VNR_HIP_CHECK(hipStreamSynchronize(stream));   // on return the box is there
}

void NeuralVolume::error_against_device(const DeviceSource& ref, const int box_lo[3], const int box_size[3], float range_lo, float range_hi, DecodeError* result,
                                        float* d_block_max)
{
  if (!result) throw std::runtime_error("null result");
  if (!net_.valid()) throw std::runtime_error("neural volume has no valid network");
  const vec3i grid = desc.dims;
  vec3i lower, size;
  const BoxLayout L = validate_box_array(ref.data, ref.type, ref.strides, box_lo, box_size, grid, lower, size, range_lo, range_hi);
  const uint64_t total = L.bx * L.by * L.bz, chunk = std::min(chunk_samples(), total);
  const vec3f rdims = {1.0f / (float)grid.x, 1.0f / (float)grid.y, 1.0f / (float)grid.z};
  const Conversion c{range_lo, range_hi - range_lo, range_lo < range_hi};
  const vec3i mcd = mc_.dims();
  if (d_block_max) require_room(d_block_max, (size_t)mcd.x * mcd.y * mcd.z * sizeof(float), "the block map");
  const BlockMap map{(uint32_t*)d_block_max, lower, mcd.x, mcd.y};
  const uint32_t max_blocks = (uint32_t)Runtime::get().n_cus * 8;
  dd_coords_.ensure(3 * chunk);
  dd_values_.ensure(chunk);
  dd_partials_.ensure((size_t)(max_blocks + 1) * (sizeof(ErrorPartial) / sizeof(double)));
  ErrorPartial* partials = (ErrorPartial*)dd_partials_.ptr;
  ErrorPartial* d_result = partials + max_blocks;
  EventGuard ev;
  wait_for(ref.producer, stream, ev);   // the reference is complete once the caller's stream reaches this point
  decode_error_init_kernel<<<div_round_up(max_blocks, kDecodeBlock), kDecodeBlock, 0, stream>>>(partials, max_blocks);
  VNR_HIP_CHECK(hipGetLastError());
  if (d_block_max) VNR_HIP_CHECK(hipMemsetAsync(d_block_max, 0, (size_t)mcd.x * mcd.y * mcd.z * sizeof(float), stream));
  for (uint64_t b = 0; b < total; b += chunk) {
    const uint64_t e = std::min(total, b + chunk);
    decode_chunk(b, (uint32_t)(e - b), L.bx, L.by, lower, rdims, dd_values_.ptr);
    const uint32_t blocks = chunk_grid(L, ref.type, b, e);
    dispatch_type(ref.type, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      decode_error_kernel<T><<<blocks, kDecodeBlock, 0, stream>>>((const T*)ref.data, L, b, e, dd_values_.ptr, c, map, partials);
    });
    VNR_HIP_CHECK(hipGetLastError());
  }
  decode_error_final_kernel<<<1, kDecodeBlock, 0, stream>>>(partials, max_blocks, d_result);
  VNR_HIP_CHECK(hipGetLastError());
  ErrorPartial r;
  VNR_HIP_CHECK(hipMemcpyAsync(&r, d_result, sizeof(r), hipMemcpyDeviceToHost, stream));
  VNR_HIP_CHECK(hipStreamSynchronize(stream));
  result->n_voxels = total;
  result->sum_abs = r.sum_abs;
  result->sum_sq = r.sum_sq;
  if (r.max_abs < 0.0) {   // every voxel's error is a NaN
    result->max_abs = std::numeric_limits<double>::quiet_NaN();
    result->worst[0] = result->worst[1] = result->worst[2] = -1;
  } else {
    result->max_abs = r.max_abs;
    const uint64_t yz = r.worst / L.bx;
    result->worst[0] = lower.x + (int)(r.worst - yz * L.bx);
    result->worst[1] = lower.y + (int)(yz % L.by);
    result->worst[2] = lower.z + (int)(yz / L.by);
  }
  const double width = c.scale ? (double)range_hi - (double)range_lo : 1.0;
  result->psnr_db = 10.0 * std::log10(width * width * (double)total / r.sum_sq);
}

}  // namespace vnr
