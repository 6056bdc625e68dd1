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
// element indices are 64-bit.  The walk, the conversion, the validation and the worst-voxel reduction live in box_walk.h, which
// correction.hip includes as well.
#include "box_walk.h"

namespace vnr {

namespace {

// voxel centres of the box's linear indices [b, b + n): generate_coords_kernel's arithmetic with a 64-bit index
__global__ void __launch_bounds__(kBlock) decode_coords_kernel(uint64_t b, uint32_t n, uint64_t bx, uint64_t by, vec3i lower, vec3f rdims,
                                                               float* __restrict__ coords)
{
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
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
    Piece<T> pc;
    const float* v = values + (i - b);
#pragma unroll
    for (int j = 0; j < PieceOf<T>::n; ++j) pc.v[j] = convert_value<T>(v[j], c);
    *reinterpret_cast<Piece<T>*>(p) = pc;   // one 16-byte vector store
  }
};

template <typename T>
__global__ void __launch_bounds__(kBlock) decode_store_kernel(T* __restrict__ dst, BoxLayout L, uint64_t b, uint64_t e, const float* __restrict__ values,
                                                              Conversion c)
{
  StoreOp<T> op{values, b, c};
  for_each_chunk_voxel<T>(dst, L, b, e, op);
}

// ---- error report: convert, compare, reduce -----------------------------------------------------------------------------------------------
using ErrorPartial = WorstPartial<double>;   // a: the sum of |e|, b: of e^2

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
  __device__ __forceinline__ void one(const T* p, uint64_t i)
  {
    uint32_t x, y, z;
    split_index(i, bx, by, x, y, z);
    voxel(*p, i, x, y, z);
  }
  __device__ __forceinline__ void piece(const T* p, uint64_t i)
  {
    const Piece<T> pc = *reinterpret_cast<const Piece<T>*>(p);   // one 16-byte vector load
    uint32_t x, y, z;
    split_index(i, bx, by, x, y, z);
#pragma unroll
    for (int j = 0; j < PieceOf<T>::n; ++j) {
      voxel(pc.v[j], i + j, x, y, z);
      next_voxel(bx, by, x, y, z);
    }
  }
};

// the block's (max, lowest index) and sums go into its own partial; worst_final_kernel<double> reduces the partials
template <typename T>
__global__ void __launch_bounds__(kBlock) decode_error_kernel(const T* __restrict__ ref, BoxLayout L, uint64_t b, uint64_t e, const float* __restrict__ values,
                                                              Conversion c, BlockMap map, ErrorPartial* __restrict__ partials)
{
  ErrorOp<T> op{values, b, c, L.bx, L.by, map};
  for_each_chunk_voxel<const T>(ref, L, b, e, op);
  if (map.cells) op.flush();
  block_reduce(op.mx, op.mi, op.sum_abs, op.sum_sq);
  if (threadIdx.x == 0) merge_partial(partials, op.mx, op.mi, op.sum_abs, op.sum_sq);
}

}  // namespace

void NeuralVolume::decode_chunk(uint64_t b, uint32_t n, uint64_t bx, uint64_t by, vec3i lower, vec3f rdims, float* d_values)
{
  decode_coords_kernel<<<div_round_up(n, kBlock), kBlock, 0, stream>>>(b, n, bx, by, lower, rdims, dd_coords_.ptr);
  VNR_HIP_CHECK(hipGetLastError());
  net_.inference(dd_coords_.ptr, d_values, n, nullptr, n, stream);
}

void NeuralVolume::decode_to_device(const DeviceTarget& out, const int box_lo[3], const int box_size[3], const int grid_dims[3], float range_lo, float range_hi)
{
  if (!net_.valid()) throw std::runtime_error("neural volume has no valid network");
  const vec3i grid = grid_dims ? vec3i{grid_dims[0], grid_dims[1], grid_dims[2]} : desc.dims;
  vec3i lower;
  const BoxLayout L = validate_box_array(out.data, out.type, out.strides, box_lo, box_size, grid, lower, range_lo, range_hi);
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
      decode_store_kernel<T><<<blocks, kBlock, 0, stream>>>((T*)out.data, L, b, e, dd_values_.ptr, c);
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
  vec3i lower;
  const BoxLayout L = validate_box_array(ref.data, ref.type, ref.strides, box_lo, box_size, grid, lower, range_lo, range_hi);
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
  worst_init_kernel<<<div_round_up(max_blocks, kBlock), kBlock, 0, stream>>>(partials, max_blocks);
  VNR_HIP_CHECK(hipGetLastError());
  if (d_block_max) VNR_HIP_CHECK(hipMemsetAsync(d_block_max, 0, (size_t)mcd.x * mcd.y * mcd.z * sizeof(float), stream));
  for (uint64_t b = 0; b < total; b += chunk) {
    const uint64_t e = std::min(total, b + chunk);
    decode_chunk(b, (uint32_t)(e - b), L.bx, L.by, lower, rdims, dd_values_.ptr);
    const uint32_t blocks = chunk_grid(L, ref.type, b, e);
    dispatch_type(ref.type, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      decode_error_kernel<T><<<blocks, kBlock, 0, stream>>>((const T*)ref.data, L, b, e, dd_values_.ptr, c, map, partials);
    });
    VNR_HIP_CHECK(hipGetLastError());
  }
  worst_final_kernel<<<1, kBlock, 0, stream>>>(partials, max_blocks, d_result);
  VNR_HIP_CHECK(hipGetLastError());
  ErrorPartial r;
  VNR_HIP_CHECK(hipMemcpyAsync(&r, d_result, sizeof(r), hipMemcpyDeviceToHost, stream));
  VNR_HIP_CHECK(hipStreamSynchronize(stream));
  result->n_voxels = total;
  result->sum_abs = r.a;
  result->sum_sq = r.b;
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
  result->psnr_db = 10.0 * std::log10(width * width * (double)total / r.b);
}

}  // namespace vnr
