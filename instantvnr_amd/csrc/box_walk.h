// box_walk.h — what decode.hip and correction.hip share: the walk of a box of a voxel grid in the caller's device array, the conversion
// of the network's output to the typed voxel, the reduction to the worst voxel, and everything a call is refused for before its first
// kernel.  The kernels that walk stay in the two files; the only kernels here are the reduction's init and final stage.
//
// The caller's array is a set of contiguous runs (one for a dense box, one per x-row for an array with ghost layers); the part of a run
// inside a chunk of linear box indices is accessed in 16-byte pieces cut at the 16-byte boundaries of the ARRAY's address, its ragged
// head and tail element by element, so a store never touches a byte outside the box and the result does not depend on where the chunks
// end.  An x stride other than 1 goes voxel by voxel.  All element indices are 64-bit.  Everything here has internal linkage: each
// translation unit that includes this file gets its own copy, and its kernels inline the device functions.
#pragma once

#include "volume.h"

#include <algorithm>
#include <cstdlib>
#include <limits>
#include <type_traits>

namespace vnr {

namespace {

constexpr int kBlock = 256;
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
    for (uint64_t i = b + (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < e; i += (uint64_t)gridDim.x * kBlock) {
      const uint64_t x = i % L.bx, yz = i / L.bx, y = yz % L.by, z = yz / L.by;
      f.one(base + ((int64_t)x * L.sx + (int64_t)y * L.sy + (int64_t)z * L.sz), i);
    }
    return;
  }
  const uint64_t r0 = b / L.run_len, r1 = (e - 1) / L.run_len;   // the runs this chunk touches
  // per run: 1 (the head) + the 16-byte pieces that cover the longest part a run can have inside this chunk
  const uint64_t P = 1 + (std::min(L.run_len, e - b) + N - 1) / N, work = (r1 - r0 + 1) * P;
  for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < work; g += (uint64_t)gridDim.x * kBlock) {
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

// ---- the piece cursor: where in the box a piece starts, and from a voxel to the next ---------------------------------------------------
template <typename T> struct alignas(16) Piece { T v[PieceOf<T>::n]; };   // moved with one 16-byte vector load or store

__device__ __forceinline__ void split_index(uint64_t i, uint64_t bx, uint64_t by, uint32_t& x, uint32_t& y, uint32_t& z)
{
  const uint64_t yz = i / bx;
  x = (uint32_t)(i - yz * bx); y = (uint32_t)(yz % by); z = (uint32_t)(yz / by);
}

// the next voxel of the box, x fastest (a dense box: a piece may run over the end of a row)
__device__ __forceinline__ void next_voxel(uint64_t bx, uint64_t by, uint32_t& x, uint32_t& y, uint32_t& z)
{
  if (++x == (uint32_t)bx) { x = 0; if (++y == (uint32_t)by) { y = 0; ++z; } }
}

// ---- the worst voxel: (max |e|, lowest index) and two side accumulators of type A, summed --------------------------------------------
// A = double: the error report's sums of |e| and e^2; A = uint64_t: the corrections' counts.  A lane's candidates come with growing
// indices, so it keeps its first of equals with a plain `a > mx`; wherever two lanes, waves or blocks meet, VNR_TAKE_WORST decides.
template <typename A>
struct WorstPartial {
  double max_abs;      // -1: no voxel yet (every |e| is >= 0)
  uint64_t worst;      // linear box index of max_abs, the lowest one among equals
  A a, b;
};
static_assert(sizeof(WorstPartial<double>) == 4 * sizeof(double) && sizeof(WorstPartial<uint64_t>) == 4 * sizeof(double), "a WorstPartial is laid over dd_partials_");

// greater, or equal with the lower index (a NaN never wins).  A macro of this section alone (undefined at its end) and not a function:
// the compiler simplifies a function before it inlines it, which reads the candidate's index from the LDS ahead of the test and
// orders the kernels' instructions differently; as text the comparison compiles to what it was when each place spelled it out.
#define VNR_TAKE_WORST(mx, mi, omx, omi) \
  do { if ((omx) > (mx) || ((omx) == (mx) && (omi) < (mi))) { (mx) = (omx); (mi) = (omi); } } while (0)

// over the block, into thread 0: inside the wave by shuffles (offsets 32 down to 1), then one value per wave through the LDS, waves
// 1.. folded in that order -- the order of the additions is part of the error report's result
template <typename A>
__device__ __forceinline__ void block_reduce(double& mx, uint64_t& mi, A& a, A& b)
{
  for (int off = 32; off > 0; off >>= 1) {
    const double omx = __shfl_down(mx, off, 64);
    const uint64_t omi = __shfl_down(mi, off, 64);
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
    VNR_TAKE_WORST(mx, mi, omx, omi);
  }
  __shared__ double w_mx[kBlock / 64];
  __shared__ uint64_t w_mi[kBlock / 64];
  __shared__ A w_sa[kBlock / 64], w_sb[kBlock / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { w_mx[wave] = mx; w_mi[wave] = mi; w_sa[wave] = a; w_sb[wave] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / 64; ++w) {
      VNR_TAKE_WORST(mx, mi, w_mx[w], w_mi[w]);
      a += w_sa[w]; b += w_sb[w];
    }
  }
}

// one partial per block; the launches of one pass run one behind the other on one stream, so block k owns partials[k] throughout
template <typename A>
__device__ __forceinline__ void merge_partial(WorstPartial<A>* __restrict__ partials, double mx, uint64_t mi, A a, A b)
{
  WorstPartial<A> p = partials[blockIdx.x];
  VNR_TAKE_WORST(p.max_abs, p.worst, mx, mi);
  p.a += a; p.b += b;
  partials[blockIdx.x] = p;
}

template <typename A>
__global__ void __launch_bounds__(kBlock) worst_init_kernel(WorstPartial<A>* __restrict__ partials, uint32_t n)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) partials[i] = WorstPartial<A>{-1.0, ~0ull, A(0), A(0)};
}

// second stage: one block over the block partials, by block stride
template <typename A>
__global__ void __launch_bounds__(kBlock) worst_final_kernel(const WorstPartial<A>* __restrict__ partials, uint32_t n, WorstPartial<A>* __restrict__ out)
{
  double mx = -1.0;
  uint64_t mi = ~0ull;
  A a = A(0), b = A(0);
  for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
    const WorstPartial<A> p = partials[i];
    VNR_TAKE_WORST(mx, mi, p.max_abs, p.worst);
    a += p.a; b += p.b;
  }
  block_reduce(mx, mi, a, b);
  if (threadIdx.x == 0) *out = WorstPartial<A>{mx, mi, a, b};
}

#undef VNR_TAKE_WORST

// ---- host side: dispatch, validation and chunking -------------------------------------------------------------------------------------
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

// everything a call is refused for, before the first kernel (box_lo = box_size = null: the whole grid); returns the layout of the box
// in the user's array and its lower corner
BoxLayout validate_box_array(const void* data, int type, const int64_t* strides, const int box_lo[3], const int box_size[3], vec3i grid, vec3i& lower, float range_lo,
                             float range_hi)
{
  if (!data) throw std::runtime_error("null device data");
  const size_t ts = device_value_type_size(type);   // refuses the 64-bit integer and the vector types like the ingest
  if (grid.x <= 0 || grid.y <= 0 || grid.z <= 0)
    throw std::runtime_error("grid dimensions must be positive: " + std::to_string(grid.x) + " x " + std::to_string(grid.y) + " x " + std::to_string(grid.z));
  if ((box_lo == nullptr) != (box_size == nullptr)) throw std::runtime_error("box_lo and box_size go together: both or neither");
  lower = box_lo ? vec3i{box_lo[0], box_lo[1], box_lo[2]} : vec3i{0, 0, 0};
  const vec3i size = box_size ? vec3i{box_size[0], box_size[1], box_size[2]} : grid;
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
  const uint64_t blocks = (work + kBlock - 1) / kBlock;
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

}  // namespace vnr
