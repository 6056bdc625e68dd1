// correction.hip — error-bounded round trip: residual corrections for the macrocells where the decode misses a tolerance, and the
// decode with a correction applied.  The last step of the in-situ loop of ingest.hip / decode.hip / guided_sampler.hip.
//
// build_correction walks the whole grid twice in chunks of linear voxel indices, exactly as decode.hip's error report does (the same
// VNR_AMD_DECODE_CHUNK, scratch and decode_chunk; the walker, the conversion, the validation and the worst-voxel reduction are
// box_walk.h's, the very ones decode.hip uses): pass 1 reduces max |q| per macrocell (one atomicMax per cell change of a lane) and
// the error before; the host turns the cell map into per-cell {payload offset, code width}; pass 2 evaluates the network again,
// stores every voxel's code of the flagged cells with one plain store each and reduces the error after.  The apply kernel decodes,
// looks the voxel's cell up and stores the corrected value in the decode's 16-byte pieces.  The arithmetic is integer or single IEEE
// double operations (include/vnr_amd.h spells it out); tests/error_bound_ref.py restates it in numpy and is matched bit for bit.
//
// correction_rates ("corrections to a byte budget") answers what many tolerances would cost without building any: one chunked
// evaluation in the packed form's order, a wave per group of 64 codes, the build's quantise per tolerance, wave reductions and
// integer atomics per cell; tests/correction_rate_ref.py restates it.  The search on top of it is correction_budget.cpp, host only.
// correction_rates_coded ("byte budgets in the coded form") is the same pass with the coded instantiation of both kernels, which adds
// the exact size of the coded form per tolerance; tests/correction_coded_rate_ref.py restates that.
//
// gather_voxels_corrected and sample_corrected ("random access to the corrected field") take a list instead of a box, one lane a query:
// the gather stores what the apply stores at the listed voxels (the box kernels' own voxel()), the sampler adds the trilinear blend of
// the stored residuals of the eight voxel centres around a position to the network's value there; tests/correction_sample_ref.py.
//
// build_correction_packed ("corrections built straight into bit planes", at the end of this file) gives build_correction's correction
// in the packed resident form without the fixed-width codes in between: the rate pass's walk for one tolerance with the error reports
// taken from it, n_cells pairs through the host (correction_direct.cpp), an index kernel, and the planes of the groups that store any
// from a second evaluation of those groups alone.  What a correction holds afterwards and every conversion of it: correction_store.hip.
#include "box_walk.h"
#include "correction_direct.h"
#include "correction_record.h"

#include <cstdio>
#include <cstring>

namespace vnr {

namespace {

// ---- the quantiser (include/vnr_amd.h, "error-bounded round trip") ----------------------------------------------------------------------
struct Quantiser {
  uint32_t kind;
  int64_t E, s;      // kind 0: floor(eps), 2 E + 1
  int64_t qmax;      // kind 0: 2^34 / s + 1; a code beyond it saturates every type, so q is clamped to it before q * s (no overflow)
  double sd;         // kind 1: 2 eps
};

template <typename T> struct BitsOf { using type = std::conditional_t<sizeof(T) == 8, uint64_t, uint32_t>; };

template <typename T>
__device__ __forceinline__ typename BitsOf<T>::type bits_of(T v)
{
  typename BitsOf<T>::type b;
  __builtin_memcpy(&b, &v, sizeof(T));
  return b;
}

// one voxel's code.  q: the signed code of kinds 0 and 1 (kind 2: 1 where the bit patterns differ); aq: |q| saturated to 32 bits;
// nan: the difference is a NaN (a NaN in ref or dec, two infinities of one sign): q = 0, the voxel stays as decoded
template <typename T>
__device__ __forceinline__ void quantise(T dec, T ref, const Quantiser& k, int64_t& q, uint32_t& aq, bool& nan)
{
  nan = false;
  if constexpr (std::is_floating_point_v<T>) {
    const double r = __dsub_rn((double)ref, (double)dec);
    nan = r != r;
    if (k.kind == kCorrectionVerbatim) { q = bits_of(dec) != bits_of(ref) ? 1 : 0; aq = (uint32_t)q; return; }
    const double qd = nan ? 0.0 : rint(__ddiv_rn(r, k.sd));   // one division, ties to even
    const double a = fabs(qd);
    if (a >= 4294967295.0) { aq = 0xffffffffu; q = qd < 0.0 ? -4294967295ll : 4294967295ll; }   // (the build is refused)
    else { q = (int64_t)qd; aq = (uint32_t)a; }
  } else {
    const int64_t r = (int64_t)ref - (int64_t)dec, t = r + k.E;
    if ((uint64_t)t <= (uint64_t)(2 * k.E)) { q = 0; aq = 0; return; }   // |r| <= E: the common case, no division
    q = t / k.s;
    if (t < 0 && q * k.s != t) --q;   // floor
    const uint64_t a = (uint64_t)(q < 0 ? -q : q);
    aq = a >= 0xffffffffull ? 0xffffffffu : (uint32_t)a;
  }
}

// what the apply stores for a voxel of a flagged cell, from the decoded value and its code
template <typename T>
__device__ __forceinline__ T corrected_value(T dec, int64_t q, const Quantiser& k)
{
  if (q == 0) return dec;   // (dec + 0 * s, spelled as what it is: -0.0 and a NaN's payload stay)
  if constexpr (std::is_floating_point_v<T>) {
    return (T)__dadd_rn((double)dec, __dmul_rn((double)q, k.sd));   // never an fma
  } else {
    const int64_t v = (int64_t)dec + std::max(-k.qmax, std::min(k.qmax, q)) * k.s;
    constexpr int64_t tmin = (int64_t)std::numeric_limits<T>::lowest(), tmax = (int64_t)std::numeric_limits<T>::max();
    return (T)std::max(tmin, std::min(tmax, v));
  }
}

// the macrocells of the grid and a voxel's place in its cell
struct CellGrid {
  uint32_t dx, dy, dz, mcx, mcy;
  __device__ __forceinline__ uint32_t cell(uint32_t x, uint32_t y, uint32_t z) const { return (x >> 4) + mcx * ((y >> 4) + mcy * (z >> 4)); }
  __device__ __forceinline__ uint32_t local(uint32_t x, uint32_t y, uint32_t z) const
  {
    const uint32_t cx = std::min(16u, dx - (x & ~15u)), cy = std::min(16u, dy - (y & ~15u));
    return (x & 15u) + cx * ((y & 15u) + cy * (z & 15u));
  }
};

using Partial = WorstPartial<uint64_t>;   // pass 1: a = voxels over the tolerance, b = NaN voxels; pass 2: both 0

// ---- pass 1: max |q| per cell, the error before ----------------------------------------------------------------------------------------------
template <typename T>
struct MeasureOp {
  const float* __restrict__ values;   // values[i - b]
  uint64_t b;
  Conversion c;
  Quantiser k;
  uint64_t bx, by;
  CellGrid g;
  uint32_t* cells;
  double mx = -1.0;
  uint64_t mi = ~0ull, n_over = 0, n_nan = 0;
  uint32_t cell = 0xffffffffu, cell_max = 0;   // the cell whose maximum is pending in cell_max

  __device__ __forceinline__ void flush()
  {
    // the map only ever grows, so a stale read can only be too small: the atomic is skipped when it could not raise the cell
    if (cell != 0xffffffffu && cell_max > cells[cell]) atomicMax(cells + cell, cell_max);
    cell_max = 0;
  }
  __device__ __forceinline__ void voxel(T ref, uint64_t i, uint32_t x, uint32_t y, uint32_t z)
  {
    const T dec = convert_value<T>(values[i - b], c);
    const double a = fabs((double)dec - (double)ref);
    if (a > mx) { mx = a; mi = i; }   // (i only grows inside a lane: the first of equals stays; a NaN never wins)
    int64_t q; uint32_t aq; bool nan;
    quantise<T>(dec, ref, k, q, aq, nan);
    n_nan += nan ? 1 : 0;
    if (aq) {
      ++n_over;
      const uint32_t cl = g.cell(x, y, z);
      if (cl != cell) { flush(); cell = cl; }
      cell_max = std::max(cell_max, aq);
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

template <typename T>
__global__ void __launch_bounds__(kBlock) correction_measure_kernel(const T* __restrict__ ref, BoxLayout L, uint64_t b, uint64_t e, const float* __restrict__ values,
                                                                    Conversion c, Quantiser k, CellGrid g, uint32_t* __restrict__ cells,
                                                                    Partial* __restrict__ partials)
{
  MeasureOp<T> op{values, b, c, k, L.bx, L.by, g, cells};
  for_each_chunk_voxel<const T>(ref, L, b, e, op);
  op.flush();
  block_reduce(op.mx, op.mi, op.n_over, op.n_nan);
  if (threadIdx.x == 0) merge_partial(partials, op.mx, op.mi, op.n_over, op.n_nan);
}

// ---- the cell table, read with the entry cached while a lane stays in one cell -----------------------------------------------------------
struct TableReader {
  const CorrectionTableEntry* __restrict__ table;
  uint32_t cell = 0xffffffffu;
  CorrectionTableEntry entry{~0ull, 0, 0};
  __device__ __forceinline__ const CorrectionTableEntry& at(uint32_t cl)
  {
    if (cl != cell) { entry = table[cl]; cell = cl; }
    return entry;
  }
};

template <typename C>
__device__ __forceinline__ void store_code(uint8_t* payload, uint64_t offset, uint32_t li, int64_t q)
{
  reinterpret_cast<C*>(payload + offset)[li] = (C)q;
}

// code li of a cell of the fixed-width payload (kinds 0 and 1), sign-extended; codes: the cell's first byte
__device__ __forceinline__ int64_t load_code(const uint8_t* __restrict__ codes, uint32_t width, uint32_t li)
{
  return width == 1 ? (int64_t)reinterpret_cast<const int8_t*>(codes)[li]
                    : (width == 2 ? (int64_t)reinterpret_cast<const int16_t*>(codes)[li] : (int64_t)reinterpret_cast<const int32_t*>(codes)[li]);
}

// the signed code of kinds 0 and 1 from its z of the packed form
__device__ __forceinline__ int64_t unzigzag(uint64_t z) { return (int64_t)(z >> 1) ^ -(int64_t)(z & 1); }

// ---- pass 2: the codes of the flagged cells, the error after --------------------------------------------------------------------------------
template <typename T>
struct EncodeOp {
  const float* __restrict__ values;
  uint64_t b;
  Conversion c;
  Quantiser k;
  uint64_t bx, by;
  CellGrid g;
  TableReader table;
  uint8_t* __restrict__ payload;
  double mx = -1.0;
  uint64_t mi = ~0ull;

  __device__ __forceinline__ void voxel(T ref, uint64_t i, uint32_t x, uint32_t y, uint32_t z)
  {
    const T dec = convert_value<T>(values[i - b], c);
    const CorrectionTableEntry& en = table.at(g.cell(x, y, z));
    T out = dec;
    if (en.offset != ~0ull) {
      const uint32_t li = g.local(x, y, z);
      if constexpr (std::is_floating_point_v<T>) {
        if (k.kind == kCorrectionVerbatim) {   // the code is ref's bit pattern, for every voxel of the cell
          reinterpret_cast<typename BitsOf<T>::type*>(payload + en.offset)[li] = bits_of(ref);
          out = ref;
        }
      }
      if (k.kind != kCorrectionVerbatim) {
        int64_t q; uint32_t aq; bool nan;
        quantise<T>(dec, ref, k, q, aq, nan);
        // every code byte is written exactly once: the voxel owns bytes [li * width, (li + 1) * width) of its cell
        if (en.width == 1) store_code<int8_t>(payload, en.offset, li, q);
        else if (en.width == 2) store_code<int16_t>(payload, en.offset, li, q);
        else store_code<int32_t>(payload, en.offset, li, q);
        out = corrected_value<T>(dec, q, k);
      }
    }
    const double a = fabs((double)out - (double)ref);
    if (a > mx) { mx = a; mi = i; }
  }
  __device__ __forceinline__ void one(const T* p, uint64_t i)
  {
    uint32_t x, y, z;
    split_index(i, bx, by, x, y, z);
    voxel(*p, i, x, y, z);
  }
  __device__ __forceinline__ void piece(const T* p, uint64_t i)
  {
    const Piece<T> pc = *reinterpret_cast<const Piece<T>*>(p);
    uint32_t x, y, z;
    split_index(i, bx, by, x, y, z);
#pragma unroll
    for (int j = 0; j < PieceOf<T>::n; ++j) {
      voxel(pc.v[j], i + j, x, y, z);
      next_voxel(bx, by, x, y, z);
    }
  }
};

template <typename T>
__global__ void __launch_bounds__(kBlock) correction_encode_kernel(const T* __restrict__ ref, BoxLayout L, uint64_t b, uint64_t e, const float* __restrict__ values,
                                                                   Conversion c, Quantiser k, CellGrid g, const CorrectionTableEntry* __restrict__ table,
                                                                   uint8_t* __restrict__ payload, Partial* __restrict__ partials)
{
  EncodeOp<T> op{values, b, c, k, L.bx, L.by, g, TableReader{table}, payload};
  for_each_chunk_voxel<const T>(ref, L, b, e, op);
  uint64_t na = 0, nb = 0;
  block_reduce(op.mx, op.mi, na, nb);
  if (threadIdx.x == 0) merge_partial<uint64_t>(partials, op.mx, op.mi, 0, 0);
}

// ---- the apply: decode, look up, correct, store ------------------------------------------------------------------------------------------------
template <typename T>
struct ApplyOp {
  const float* __restrict__ values;
  uint64_t b;
  Conversion c;
  Quantiser k;
  uint64_t bx, by;
  CellGrid g;
  uint32_t ox, oy, oz;   // the box's lower corner: cell and local index are those of the grid coordinate
  TableReader table;
  const uint8_t* __restrict__ payload;

  // x, y, z: the voxel in the box
  __device__ __forceinline__ T voxel(uint64_t i, uint32_t x, uint32_t y, uint32_t z)
  {
    x += ox; y += oy; z += oz;
    const T dec = convert_value<T>(values[i - b], c);
    const CorrectionTableEntry& en = table.at(g.cell(x, y, z));
    if (en.offset == ~0ull) return dec;
    const uint32_t li = g.local(x, y, z);
    const uint8_t* codes = payload + en.offset;
    if constexpr (std::is_floating_point_v<T>) {
      if (k.kind == kCorrectionVerbatim) {
        const typename BitsOf<T>::type bits = reinterpret_cast<const typename BitsOf<T>::type*>(codes)[li];
        T v;
        __builtin_memcpy(&v, &bits, sizeof(T));
        return v;
      }
    }
    return corrected_value<T>(dec, load_code(codes, en.width, li), k);
  }
  __device__ __forceinline__ void one(T* p, uint64_t i)
  {
    uint32_t x, y, z;
    split_index(i, bx, by, x, y, z);
    *p = voxel(i, x, y, z);
  }
  __device__ __forceinline__ void piece(T* p, uint64_t i)
  {
    Piece<T> pc;
    uint32_t x, y, z;
    split_index(i, bx, by, x, y, z);
#pragma unroll
    for (int j = 0; j < PieceOf<T>::n; ++j) {
      pc.v[j] = voxel(i + j, x, y, z);
      next_voxel(bx, by, x, y, z);
    }
    *reinterpret_cast<Piece<T>*>(p) = pc;   // one 16-byte vector store
  }
};

template <typename T>
__global__ void __launch_bounds__(kBlock) correction_apply_kernel(T* __restrict__ dst, BoxLayout L, uint64_t b, uint64_t e, const float* __restrict__ values,
                                                                  Conversion c, Quantiser k, CellGrid g, uint32_t ox, uint32_t oy, uint32_t oz,
                                                                  const CorrectionTableEntry* __restrict__ table, const uint8_t* __restrict__ payload)
{
  ApplyOp<T> op{values, b, c, k, L.bx, L.by, g, ox, oy, oz, TableReader{table}, payload};
  for_each_chunk_voxel<T>(dst, L, b, e, op);
}

// ---- the apply that reads the bit planes (correction_packed_format.h): the same walk, a voxel's code gathered from its group's planes ----
// The index of correction_plane_index on the device: cells[cell] = {the cell's first plane word, its first group} (word0 = ~0: not
// flagged), groups[group] = the group's first word inside its cell | nbits << 16.  Code li of a cell is lane li % 64 of its group
// li / 64, and bit b of its z is bit `lane` of the group's plane word b: nbits loads of 8 bytes, none for a group of zeros.  The M
// codes [li, li + M) of ONE group come out of one pass over its planes, which is what a 16-byte piece inside an x-row of a cell
// needs (cx == 16: always; a ragged cell, a box that starts between pieces: voxel by voxel where the piece straddles).
template <typename T>
struct PlanesApplyOp {
  using Z = typename BitsOf<T>::type;   // kinds 0 and 1: the z of a code of at most 4 bytes has at most 32 bits; kind 2: sizeof(T) bytes
  const float* __restrict__ values;
  uint64_t b;
  Conversion c;
  Quantiser k;
  uint64_t bx, by;
  CellGrid g;
  uint32_t ox, oy, oz;
  const Correction::PlaneCell* __restrict__ cells;
  const uint32_t* __restrict__ groups;
  const uint64_t* __restrict__ planes;
  uint32_t cell = 0xffffffffu;   // the entry cached while a lane stays in one cell, as TableReader does
  Correction::PlaneCell entry{~0ull, 0, 0};

  __device__ __forceinline__ const Correction::PlaneCell& at(uint32_t cl)
  {
    if (cl != cell) { entry = cells[cl]; cell = cl; }
    return entry;
  }
  // z of the codes [li, li + M) of a flagged cell; they lie in one group
  template <int M>
  __device__ __forceinline__ void read_codes(const Correction::PlaneCell& en, uint32_t li, Z (&z)[M]) const
  {
    const uint32_t gi = groups[en.group0 + (li >> 6)], nbits = gi >> 16, lane = li & 63u;
    const uint64_t* __restrict__ w = planes + (en.word0 + (gi & 0xffffu));
#pragma unroll
    for (int j = 0; j < M; ++j) z[j] = 0;
    for (uint32_t p = 0; p < nbits; ++p) {
      const uint32_t bits = (uint32_t)(w[p] >> lane);   // (M <= 16 lanes from `lane` on)
#pragma unroll
      for (int j = 0; j < M; ++j) z[j] |= (Z)((bits >> j) & 1u) << p;
    }
  }
  __device__ __forceinline__ T corrected(T dec, Z z) const
  {
    if constexpr (std::is_floating_point_v<T>) {
      if (k.kind == kCorrectionVerbatim) {
        T v;
        __builtin_memcpy(&v, &z, sizeof(T));
        return v;
      }
    }
    return corrected_value<T>(dec, unzigzag(z), k);
  }
  // x, y, z: the voxel in the grid
  __device__ __forceinline__ T voxel(uint64_t i, uint32_t x, uint32_t y, uint32_t z)
  {
    const T dec = convert_value<T>(values[i - b], c);
    const Correction::PlaneCell& en = at(g.cell(x, y, z));
    if (en.word0 == ~0ull) return dec;
    Z code[1];
    read_codes<1>(en, g.local(x, y, z), code);
    return corrected(dec, code[0]);
  }
  __device__ __forceinline__ void one(T* p, uint64_t i)
  {
    uint32_t x, y, z;
    split_index(i, bx, by, x, y, z);
    *p = voxel(i, ox + x, oy + y, oz + z);
  }
  __device__ __forceinline__ void piece(T* p, uint64_t i)
  {
    constexpr int N = PieceOf<T>::n;
    Piece<T> pc;
    uint32_t x, y, z;
    split_index(i, bx, by, x, y, z);
    const uint32_t gx = ox + x, gy = oy + y, gz = oz + z;
    const uint32_t li = g.local(gx, gy, gz);
    // the piece stays in its row of the box, in one cell and in one group of it: its codes are consecutive lanes of that group
    if (x + N <= (uint32_t)bx && (gx >> 4) == ((gx + N - 1) >> 4) && (li >> 6) == ((li + N - 1) >> 6)) {
      const float* v = values + (i - b);
#pragma unroll
      for (int j = 0; j < N; ++j) pc.v[j] = convert_value<T>(v[j], c);
      const Correction::PlaneCell& en = at(g.cell(gx, gy, gz));
      if (en.word0 != ~0ull) {
        Z code[N];
        read_codes<N>(en, li, code);
#pragma unroll
        for (int j = 0; j < N; ++j) pc.v[j] = corrected(pc.v[j], code[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        pc.v[j] = voxel(i + j, ox + x, oy + y, oz + z);
        next_voxel(bx, by, x, y, z);
      }
    }
    *reinterpret_cast<Piece<T>*>(p) = pc;   // one 16-byte vector store
  }
};

template <typename T>
__global__ void __launch_bounds__(kBlock) correction_apply_planes_kernel(T* __restrict__ dst, BoxLayout L, uint64_t b, uint64_t e, const float* __restrict__ values,
                                                                         Conversion c, Quantiser k, CellGrid g, uint32_t ox, uint32_t oy, uint32_t oz,
                                                                         const Correction::PlaneCell* __restrict__ cells, const uint32_t* __restrict__ groups,
                                                                         const uint64_t* __restrict__ planes)
{
  PlanesApplyOp<T> op{values, b, c, k, L.bx, L.by, g, ox, oy, oz, cells, groups, planes};
  for_each_chunk_voxel<T>(dst, L, b, e, op);
}

// ---- random access (include/vnr_amd.h, "random access to the corrected field"): a list instead of a box, one lane a query ---------------------
// What the list calls read of a correction: kFormFixed and kFormPacked are the resident forms; kFormNone: no cell is flagged.
constexpr int kFormFixed = 0, kFormPacked = 1, kFormNone = 2;

struct CorrectionView {
  const CorrectionTableEntry* __restrict__ table;
  const uint8_t* __restrict__ payload;
  const Correction::PlaneCell* __restrict__ cells;
  const uint32_t* __restrict__ groups;
  const uint64_t* __restrict__ planes;
};

// position j of the lowest voxel of the list outside the grid into *first_bad (the caller sets it to ~0): one ballot a wave, one
// atomicMin a wave that holds such a voxel.  A negative component is a large unsigned one.
__global__ void __launch_bounds__(kBlock) correction_voxels_check_kernel(const int32_t* __restrict__ voxels, uint64_t n, CellGrid g,
                                                                         unsigned long long* __restrict__ first_bad)
{
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock + (threadIdx.x & ~63u); base < n; base += (uint64_t)gridDim.x * kBlock) {   // (wave-uniform)
    const uint64_t j = base + lane;
    bool bad = false;
    if (j < n) bad = (uint32_t)voxels[3 * j + 0] >= g.dx || (uint32_t)voxels[3 * j + 1] >= g.dy || (uint32_t)voxels[3 * j + 2] >= g.dz;
    const uint64_t mask = __ballot(bad);
    if (mask && lane == 0) atomicMin(first_bad, (unsigned long long)(base + (uint32_t)__ffsll((long long)mask) - 1u));
  }
}

// the centres of the listed voxels: decode_coords_kernel's arithmetic
__global__ void __launch_bounds__(kBlock) correction_voxel_coords_kernel(const int32_t* __restrict__ voxels, uint32_t n, vec3f rdims, float* __restrict__ coords)
{
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  coords[3 * (size_t)t + 0] = ((float)voxels[3 * (size_t)t + 0] + 0.5f) * rdims.x;
  coords[3 * (size_t)t + 1] = ((float)voxels[3 * (size_t)t + 1] + 0.5f) * rdims.y;
  coords[3 * (size_t)t + 2] = ((float)voxels[3 * (size_t)t + 2] + 0.5f) * rdims.z;
}

// out[t] = what the apply of this form stores at voxel t of the list: the very voxel() of the box kernels, the box at the origin
template <typename T, int Form>
__global__ void __launch_bounds__(kBlock) correction_gather_kernel(const int32_t* __restrict__ voxels, uint32_t n, const float* __restrict__ values, Conversion c,
                                                                   Quantiser k, CellGrid g, CorrectionView v, T* __restrict__ out)
{
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  const uint32_t x = (uint32_t)voxels[3 * (size_t)t + 0], y = (uint32_t)voxels[3 * (size_t)t + 1], z = (uint32_t)voxels[3 * (size_t)t + 2];
  if constexpr (Form == kFormFixed) {
    ApplyOp<T> op{values, 0, c, k, 0, 0, g, 0, 0, 0, TableReader{v.table}, v.payload};
    out[t] = op.voxel(t, x, y, z);
  } else if constexpr (Form == kFormPacked) {
    PlanesApplyOp<T> op{values, 0, c, k, 0, 0, g, 0, 0, 0, v.cells, v.groups, v.planes};
    out[t] = op.voxel(t, x, y, z);
  } else {
    out[t] = convert_value<T>(values[t], c);
  }
}

// where a coordinate lies between the voxel centres of its axis, in fp32: t = p dim - 0.5 clamped to [0, dim - 1] (a NaN: 0)
struct AxisPlace { uint32_t i0, i1; float w; };

__device__ __forceinline__ AxisPlace axis_place(float p, uint32_t dim)
{
  float t = __fsub_rn(__fmul_rn(p, (float)dim), 0.5f);
  if (!(t >= 0.0f)) t = 0.0f;
  const float top = (float)(dim - 1u);
  if (t > top) t = top;
  const float f = floorf(t);
  const uint32_t i0 = (uint32_t)f;
  return AxisPlace{i0, std::min(i0 + 1u, dim - 1u), __fsub_rn(t, f)};   // (the difference is exact)
}

// the codes of the two x-neighbours x0 <= x1 <= x0 + 1 of a row; a voxel of a cell that is not flagged has the code 0
struct FixedRows {
  CellGrid g;
  TableReader table;
  const uint8_t* __restrict__ payload;
  __device__ __forceinline__ int64_t code(uint32_t x, uint32_t y, uint32_t z)
  {
    const CorrectionTableEntry& en = table.at(g.cell(x, y, z));
    return en.offset == ~0ull ? 0 : load_code(payload + en.offset, en.width, g.local(x, y, z));
  }
  __device__ __forceinline__ void row(uint32_t x0, uint32_t x1, uint32_t y, uint32_t z, int64_t (&q)[2])
  {
    q[0] = code(x0, y, z);
    q[1] = x1 == x0 ? q[0] : code(x1, y, z);
  }
};

// in the packed form both come out of one pass over their group's planes wherever they are adjacent lanes of one group
struct PlaneRows {
  PlanesApplyOp<float> op;   // for its cached cell entry and its read_codes: a z of kinds 0 and 1 has at most 32 bits
  __device__ __forceinline__ int64_t code(uint32_t x, uint32_t y, uint32_t z)
  {
    const Correction::PlaneCell& en = op.at(op.g.cell(x, y, z));
    if (en.word0 == ~0ull) return 0;
    uint32_t zc[1];
    op.read_codes<1>(en, op.g.local(x, y, z), zc);
    return unzigzag(zc[0]);
  }
  __device__ __forceinline__ void row(uint32_t x0, uint32_t x1, uint32_t y, uint32_t z, int64_t (&q)[2])
  {
    const uint32_t li = op.g.local(x0, y, z);
    if (x1 != x0 && (x0 >> 4) == (x1 >> 4) && (li >> 6) == ((li + 1u) >> 6)) {
      q[0] = q[1] = 0;
      const Correction::PlaneCell& en = op.at(op.g.cell(x0, y, z));
      if (en.word0 == ~0ull) return;
      uint32_t zc[2];
      op.read_codes<2>(en, li, zc);
      q[0] = unzigzag(zc[0]); q[1] = unzigzag(zc[1]);
    } else {   // the clamped upper face, a cell boundary, a row of a ragged cell that wraps a group: one by one
      q[0] = code(x0, y, z);
      q[1] = x1 == x0 ? q[0] : code(x1, y, z);
    }
  }
};

// the stored residual of a voxel as a double (kinds 0 and 1)
__device__ __forceinline__ double code_residual(int64_t q, const Quantiser& k)
{
  if (k.kind == kCorrectionInteger) return (double)(std::max(-k.qmax, std::min(k.qmax, q)) * k.s);
  return __dmul_rn((double)q, k.sd);
}

__device__ __forceinline__ double lerp_rn(double a, double b, double w)   // three roundings, never an fma; w = 0 or 1 gives an endpoint exactly
{
  return __dadd_rn(__dmul_rn(a, __dsub_rn(1.0, w)), __dmul_rn(b, w));
}

// values[t]: the network's value at coords[t] -> the corrected field there, in place: the converted value plus the trilinear blend of
// the residuals of the eight surrounding voxel centres, x first, then y, then z.  All eight codes 0: the converted value as it is.
template <int Form>
__global__ void __launch_bounds__(kBlock) correction_sample_kernel(const float* __restrict__ coords, float* __restrict__ values, uint32_t n, Conversion c, Quantiser k,
                                                                   CellGrid g, CorrectionView v)
{
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  const float d = convert_value<float>(values[t], c);
  if constexpr (Form == kFormNone) {
    values[t] = d;
  } else {
    const AxisPlace ax = axis_place(coords[3 * (size_t)t + 0], g.dx), ay = axis_place(coords[3 * (size_t)t + 1], g.dy), az = axis_place(coords[3 * (size_t)t + 2], g.dz);
    int64_t q[4][2];   // the rows (y0, z0), (y1, z0), (y0, z1), (y1, z1)
    if constexpr (Form == kFormFixed) {
      FixedRows rows{g, TableReader{v.table}, v.payload};
      rows.row(ax.i0, ax.i1, ay.i0, az.i0, q[0]); rows.row(ax.i0, ax.i1, ay.i1, az.i0, q[1]);
      rows.row(ax.i0, ax.i1, ay.i0, az.i1, q[2]); rows.row(ax.i0, ax.i1, ay.i1, az.i1, q[3]);
    } else {
      PlaneRows rows{PlanesApplyOp<float>{nullptr, 0, c, k, 0, 0, g, 0, 0, 0, v.cells, v.groups, v.planes}};
      rows.row(ax.i0, ax.i1, ay.i0, az.i0, q[0]); rows.row(ax.i0, ax.i1, ay.i1, az.i0, q[1]);
      rows.row(ax.i0, ax.i1, ay.i0, az.i1, q[2]); rows.row(ax.i0, ax.i1, ay.i1, az.i1, q[3]);
    }
    int64_t any = 0;
    double r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      any |= q[i][0] | q[i][1];
      r[i] = lerp_rn(code_residual(q[i][0], k), code_residual(q[i][1], k), (double)ax.w);
    }
    const double blend = lerp_rn(lerp_rn(r[0], r[1], (double)ay.w), lerp_rn(r[2], r[3], (double)ay.w), (double)az.w);
    values[t] = any == 0 ? d : (float)__dadd_rn((double)d, blend);   // (-0.0 and a NaN's payload stay where nothing is stored)
  }
}

// ---- the rate pass: the sizes many tolerances would build, from one evaluation of the network ----------------------------------------------
// (include/vnr_amd.h, "corrections to a byte budget").  The walk is the packed form's: a chunk is a run of consecutive groups of 64
// codes over ALL cells of the grid, cell index ascending, a cell's codes in lx + cx (ly + cy lz); one wave takes one group, lane l its
// code l, exactly as correction_pack.hip does for the flagged cells.  A group's place follows in closed form from the grid's dims: the
// cells along an axis are 16 wide but the last, so a cell has one of 8 group counts, an x-row of cells one of 4, a z-layer one of 2.
constexpr int kRateBatch = 16;   // tolerances a launch takes; more are further launches over the same chunk's values

struct GroupWalk {
  uint32_t dx, dy, dz, mcx, mcy, mcz;
  uint32_t cell_groups[2][2][2];   // groups of a cell, [last in z][last in y][last in x]
  uint64_t row_groups[2][2];       // of an x-row of cells, [last in z][last in y]
  uint64_t layer_groups[2];        // of a z-layer of cells, [last in z]
  uint64_t n_groups;               // of the grid
  bool narrow;                     // every count above fits 32 bits: the divisions are 32-bit

  struct Place {
    uint32_t cell, voxels, cx, cy;   // the cell, its voxels and its extents
    uint32_t x0, y0, z0;             // its lower corner
    uint32_t group;                  // the group inside the cell
  };
  __device__ __forceinline__ Place place(uint64_t gid) const
  {
    uint32_t ix, iy, iz, rem;
    if (narrow) {
      const uint32_t g = (uint32_t)gid;
      iz = std::min(g / (uint32_t)layer_groups[0], mcz - 1);
      const uint32_t lz = iz == mcz - 1, in_layer = g - iz * (uint32_t)layer_groups[0];
      iy = std::min(in_layer / (uint32_t)row_groups[lz][0], mcy - 1);
      const uint32_t ly = iy == mcy - 1, in_row = in_layer - iy * (uint32_t)row_groups[lz][0];
      ix = std::min(in_row / cell_groups[lz][ly][0], mcx - 1);
      rem = in_row - ix * cell_groups[lz][ly][0];
    } else {
      iz = (uint32_t)std::min<uint64_t>(gid / layer_groups[0], mcz - 1);
      const uint32_t lz = iz == mcz - 1;
      const uint64_t in_layer = gid - iz * layer_groups[0];
      iy = (uint32_t)std::min<uint64_t>(in_layer / row_groups[lz][0], mcy - 1);
      const uint32_t ly = iy == mcy - 1;
      const uint64_t in_row = in_layer - iy * row_groups[lz][0];
      ix = (uint32_t)std::min<uint64_t>(in_row / cell_groups[lz][ly][0], mcx - 1);
      rem = (uint32_t)(in_row - (uint64_t)ix * cell_groups[lz][ly][0]);
    }
    Place p;
    p.x0 = ix * 16u; p.y0 = iy * 16u; p.z0 = iz * 16u;
    p.cx = std::min(16u, dx - p.x0); p.cy = std::min(16u, dy - p.y0);
    p.voxels = p.cx * p.cy * std::min(16u, dz - p.z0);
    p.cell = ix + mcx * (iy + mcy * iz);
    p.group = rem;
    return p;
  }
};

// the voxel centres of the groups [g0, g0 + n / 64) in that order: decode_coords_kernel's arithmetic.  A lane beyond its cell's voxels
// (the last group of a ragged cell) gets the cell's last voxel: its value is evaluated and never read.
__device__ __forceinline__ void group_lane_coords(const GroupWalk& w, uint64_t gid, uint32_t t, vec3f rdims, float* __restrict__ coords)
{
  const GroupWalk::Place p = w.place(gid);
  const uint32_t li = std::min(p.group * 64u + (t & 63u), p.voxels - 1u);
  const uint32_t row = li / p.cx, lx = li - row * p.cx, lz = row / p.cy, ly = row - lz * p.cy;
  coords[3 * (size_t)t + 0] = ((float)(int)(p.x0 + lx) + 0.5f) * rdims.x;
  coords[3 * (size_t)t + 1] = ((float)(int)(p.y0 + ly) + 0.5f) * rdims.y;
  coords[3 * (size_t)t + 2] = ((float)(int)(p.z0 + lz) + 0.5f) * rdims.z;
}

__global__ void __launch_bounds__(kBlock) correction_rate_coords_kernel(GroupWalk w, uint64_t g0, uint32_t n, vec3f rdims, float* __restrict__ coords)
{
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  group_lane_coords(w, g0 + (t >> 6), t, rdims, coords);
}

// the same for a list of groups (the direct build's pass 2): group t / 64 of the chunk is list[t / 64] of the walk
__global__ void __launch_bounds__(kBlock) correction_list_coords_kernel(GroupWalk w, const uint64_t* __restrict__ list, uint32_t n, vec3f rdims, float* __restrict__ coords)
{
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  group_lane_coords(w, list[t >> 6], t, rdims, coords);
}

struct RateBatch {
  Quantiser k[kRateBatch];
  int n;
};
struct RateCell { uint32_t max_q, nbits; };   // per (tolerance, macrocell): max |q| saturated, the sum of its groups' nbits

__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
  for (int off = 32; off > 0; off >>= 1) v = std::max(v, (uint32_t)__shfl_xor(v, off, 64));
  return v;
}

// the arguments a kernel takes only in its coded instantiation, by place
template <typename A, typename... R> __device__ __forceinline__ A first_of(A a, R...) { return a; }
template <typename A, typename B, typename... R> __device__ __forceinline__ B second_of(A, B b, R...) { return b; }

// what a plane of the coded form costs: a list of its c <= 9 set lanes, or one bit and the plane (correction_coded_format.h)
__device__ __forceinline__ uint32_t coded_plane_bits(uint64_t plane)
{
  const uint32_t count = (uint32_t)__popcll(plane);
  return count <= kCodedListMax ? 5u + 6u * count : 65u;
}

// groups [g0, g0 + n_groups) of the walk, their values in values[64 * (group - g0) + lane].  A lane reads its voxel of ref through the
// strides, converts its value and forms the code of every tolerance of the batch with the build's quantise; per tolerance the wave
// reduces max |q| and the bit length of the largest z (the group's nbits) and counts the codes != 0 with a ballot.  Lane 0 folds the
// two maxima into the cell's pair (a cell has up to 64 groups, which may lie in several blocks and chunks) and the count into the
// block's; all three are integers, so the result is exact whatever the order.  stats[j * n_cells + cell], nonzero[j]: of tolerance j.
//
// Coded (the coded rate call alone; the plain call's kernel is the instantiation without it and takes no argument for it): the length
// of the group's record of the coded form (correction_coded_format.h) in closed form, as correction_code_measure_kernel finds it from
// the resident codes.  The magnitude of a lane is |q| (kind 2: ref's bit pattern), mbits the bit length of the wave's largest; a plane
// is one ballot and one popcount and costs 5 + 6 c bits as a list of c <= 9 lanes, 65 dense; kinds 0 and 1 add a sign bit per lane
// with q != 0, the ballot that is there already.  All of it is wave-uniform, the plane loop a scalar loop.  Lane 0 adds the sum to
// coded_bits[j * n_cells + cell]: one integer atomic, exact in any order.  The 7 bits of mbits are not in it: EVERY group of a
// flagged cell has them, the groups of zeros that leave above included, and correction_rate_final_kernel adds them per cell.  A cell
// has at most 64 groups of at most 64 planes and 64 signs, so its sum stays below 2^19.  A magnitude is read from aq, which
// saturates at 2^32 - 1: such an entry is refused and its sizes are never reported.
template <typename T, typename... Coded>
__global__ void __launch_bounds__(kBlock) correction_rate_kernel(const T* __restrict__ ref, int64_t sx, int64_t sy, int64_t sz, GroupWalk w, uint64_t g0, uint32_t n_groups,
                                                                 const float* __restrict__ values, Conversion c, RateBatch batch, uint64_t n_cells,
                                                                 RateCell* __restrict__ stats, unsigned long long* __restrict__ nonzero, Coded... coded)
{
  constexpr bool kCoded = sizeof...(Coded) != 0;   // coded: (uint32_t* coded_bits), beside stats and zeroed by the caller
  __shared__ uint32_t block_nonzero[kRateBatch];   // (a chunk holds at most 2^28 samples)
  if (threadIdx.x < kRateBatch) block_nonzero[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u, waves = kBlock / 64;
  for (uint32_t g = blockIdx.x * waves + (threadIdx.x >> 6); g < n_groups; g += gridDim.x * waves) {
    const GroupWalk::Place p = w.place(g0 + g);
    const uint32_t li = p.group * 64u + lane;
    const bool has = li < p.voxels;   // the pack fills the other lanes with codes of value 0
    T rv = T(0), dec = T(0);
    if (has) {
      const uint32_t row = li / p.cx, lx = li - row * p.cx, lz = row / p.cy, ly = row - lz * p.cy;
      rv = ref[(int64_t)(p.x0 + lx) * sx + (int64_t)(p.y0 + ly) * sy + (int64_t)(p.z0 + lz) * sz];
      dec = convert_value<T>(values[(size_t)g * 64 + lane], c);
    }
    for (int j = 0; j < batch.n; ++j) {
      const Quantiser& k = batch.k[j];
      int64_t q = 0; uint32_t aq = 0; bool nan;
      uint64_t z = 0;
      if (has) {
        quantise<T>(dec, rv, k, q, aq, nan);
        if constexpr (std::is_floating_point_v<T>) z = k.kind == kCorrectionVerbatim ? (uint64_t)bits_of(rv) : ((uint64_t)q << 1) ^ (uint64_t)(q >> 63);
        else z = ((uint64_t)q << 1) ^ (uint64_t)(q >> 63);
      }
      const uint64_t differ = __ballot(q != 0);
      if (differ == 0 && k.kind != kCorrectionVerbatim) continue;   // a group of zeros: nothing to fold (verbatim: its planes are ref's bits)
      const uint32_t m = wave_max(aq), nbits = wave_max(z ? 64u - (uint32_t)__clzll((long long)z) : 0u);
      if (lane == 0) {
        RateCell* s = stats + ((uint64_t)j * n_cells + p.cell);
        if (m) atomicMax(&s->max_q, m);
        if (nbits) atomicAdd(&s->nbits, nbits);
        if (differ) atomicAdd(&block_nonzero[j], (uint32_t)__popcll(differ));
      }
      if constexpr (kCoded) {
        uint32_t* __restrict__ coded_bits = first_of(coded...);
        uint32_t mbits, bits;
        bool verbatim = false;
        if constexpr (std::is_floating_point_v<T>) verbatim = k.kind == kCorrectionVerbatim;
        if (verbatim) {   // the planes of the patterns are the planes of z; no signs
          mbits = (uint32_t)__builtin_amdgcn_readfirstlane((int)nbits);
          bits = 0;
          for (uint32_t b = 0; b < mbits; ++b) bits += coded_plane_bits(__ballot((int)((z >> b) & 1)));
        } else {
          mbits = (uint32_t)__builtin_amdgcn_readfirstlane((int)(m ? 32u - (uint32_t)__clz((int)m) : 0u));
          bits = (uint32_t)__popcll(differ);
          for (uint32_t b = 0; b < mbits; ++b) bits += coded_plane_bits(__ballot((int)((aq >> b) & 1u)));
        }
        if (lane == 0 && bits) atomicAdd(coded_bits + ((uint64_t)j * n_cells + p.cell), bits);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < (uint32_t)batch.n && block_nonzero[threadIdx.x]) atomicAdd(nonzero + threadIdx.x, (unsigned long long)block_nonzero[threadIdx.x]);
}

struct RateSums { uint64_t n_flagged, n_groups, payload_bytes, sum_nbits, n_voxels_flagged, refused; };
struct RateWidths { uint8_t verbatim[64]; };   // per tolerance: sizeof(T) for kind 2, 0 for the width rule on max |q|

__device__ __forceinline__ uint64_t block_sum(uint64_t v)
{
  for (int off = 32; off > 0; off >>= 1) v += (uint64_t)__shfl_down((unsigned long long)v, off, 64);
  __shared__ uint64_t w_sum[kBlock / 64];
  if ((threadIdx.x & 63) == 0) w_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t r = 0;
  for (int i = 0; i < kBlock / 64; ++i) r += w_sum[i];
  __syncthreads();
  return r;
}

// block j: the per-cell pairs of tolerance j -> its sums, with the header's width rule and the paddings of both serialised forms.
// Coded: a flagged cell's stream is its records' bits, 7 for every group's mbits plus what the rate kernel summed, filled up to whole
// 64-bit words; coded_words[j] gets the sum over the flagged cells.
template <typename... Coded>
__global__ void __launch_bounds__(kBlock) correction_rate_final_kernel(const RateCell* __restrict__ stats, uint64_t n_cells, CellGrid g, RateWidths widths,
                                                                       const unsigned long long* __restrict__ nonzero, RateSums* __restrict__ out, Coded... coded)
{
  constexpr bool kCoded = sizeof...(Coded) != 0;   // coded: (const uint32_t* coded_bits, uint64_t* coded_words)
  const uint32_t j = blockIdx.x;
  const uint32_t verbatim = widths.verbatim[j];
  uint64_t n_flagged = 0, n_groups = 0, payload = 0, nbits = 0, refused = 0;
  [[maybe_unused]] uint64_t words = 0;
  for (uint64_t cl = threadIdx.x; cl < n_cells; cl += kBlock) {
    const RateCell s = stats[(uint64_t)j * n_cells + cl];
    if (s.max_q == 0) continue;
    if (s.max_q > 0x7fffffffu) refused = 1;
    const uint32_t ix = (uint32_t)(cl % g.mcx), iy = (uint32_t)(cl / g.mcx % g.mcy), iz = (uint32_t)(cl / ((uint64_t)g.mcx * g.mcy));
    const uint64_t voxels = (uint64_t)std::min(16u, g.dx - 16u * ix) * std::min(16u, g.dy - 16u * iy) * std::min(16u, g.dz - 16u * iz);
    const uint32_t width = verbatim ? verbatim : (s.max_q <= 127u ? 1u : (s.max_q <= 32767u ? 2u : 4u));
    ++n_flagged;
    n_groups += (voxels + 63) / 64;
    payload += (voxels * width + 15) / 16 * 16;
    nbits += s.nbits;
    if constexpr (kCoded) words += ((uint64_t)first_of(coded...)[(uint64_t)j * n_cells + cl] + 7 * ((voxels + 63) / 64) + 63) / 64;
  }
  n_flagged = block_sum(n_flagged); n_groups = block_sum(n_groups); payload = block_sum(payload); nbits = block_sum(nbits); refused = block_sum(refused);
  if (threadIdx.x == 0) out[j] = RateSums{n_flagged, n_groups, payload, nbits, nonzero[j], refused};
  if constexpr (kCoded) {
    words = block_sum(words);
    if (threadIdx.x == 0) second_of(coded...)[j] = words;
  }
}

Quantiser make_quantiser(uint32_t kind, double eps)
{
  Quantiser k{kind, 0, 1, 1, 1.0};
  if (kind == kCorrectionInteger) {
    k.E = (int64_t)std::floor(std::min(eps, kCorrectionMaxIntegerEps));
    k.s = 2 * k.E + 1;
    k.qmax = (1ll << 34) / k.s + 1;
  } else if (kind == kCorrectionFloat) {
    k.sd = 2.0 * eps;
  }
  return k;
}

CellGrid make_cell_grid(vec3i d)
{
  return CellGrid{(uint32_t)d.x, (uint32_t)d.y, (uint32_t)d.z, (uint32_t)((d.x + 15) / 16), (uint32_t)((d.y + 15) / 16)};
}

void index_to_voxel(uint64_t i, const BoxLayout& L, int out[3])
{
  const uint64_t yz = i / L.bx;
  out[0] = (int)(i - yz * L.bx); out[1] = (int)(yz % L.by); out[2] = (int)(yz / L.by);
}

// what a build reports: the counts and the error before, the error after and where it is (a negative maximum: every error is a NaN)
void set_report(Correction& corr, const Partial& before, const Partial& after, const BoxLayout& L)
{
  const double nan = std::numeric_limits<double>::quiet_NaN();
  corr.n_voxels_flagged = before.a;
  corr.n_nan = before.b;
  corr.max_abs_before = before.max_abs < 0.0 ? nan : before.max_abs;
  corr.data.h.max_abs_after = after.max_abs < 0.0 ? nan : after.max_abs;
  if (!(after.max_abs < 0.0)) index_to_voxel(after.worst, L, corr.worst_after);
}

}  // namespace

uint64_t NeuralVolume::params_hash()
{
  std::vector<uint16_t> p(net_.n_params());
  net_.get_params_f16(p.data(), p.size(), stream);
  return fnv1a64(p.data(), p.size() * sizeof(uint16_t));
}

std::shared_ptr<Correction> NeuralVolume::build_correction(const DeviceSource& ref, float range_lo, float range_hi, double eps)
{
  if (!net_.valid()) throw std::runtime_error("neural volume has no valid network");
  if (!(eps >= 0.0) || !std::isfinite(eps)) throw std::runtime_error("eps must be a finite tolerance >= 0 in data units, got " + std::to_string(eps));
  const vec3i grid = desc.dims;
  vec3i lower;
  const BoxLayout L = validate_box_array(ref.data, ref.type, ref.strides, nullptr, nullptr, grid, lower, range_lo, range_hi);
  const uint64_t total = L.bx * L.by * L.bz, chunk = std::min(chunk_samples(), total);
  const vec3f rdims = {1.0f / (float)grid.x, 1.0f / (float)grid.y, 1.0f / (float)grid.z};
  const Conversion c{range_lo, range_hi - range_lo, range_lo < range_hi};
  const bool is_float = correction_type_is_float(ref.type);
  const uint32_t kind = !is_float ? kCorrectionInteger : (eps > 0.0 ? kCorrectionFloat : kCorrectionVerbatim);
  const Quantiser k = make_quantiser(kind, eps);
  const CellGrid g = make_cell_grid(grid);
  const int dims[3] = {grid.x, grid.y, grid.z};
  const uint64_t n_cells = correction_n_cells(dims);

  auto corr = std::make_shared<Correction>(CorrectionOrigin::Built);
  CorrectionHeader& h = corr->data.h;
  h.value_type = ref.type;
  for (int a = 0; a < 3; ++a) h.dims[a] = dims[a];
  h.eps = eps; h.range_lo = range_lo; h.range_hi = range_hi; h.kind = kind;
  h.step = correction_step(kind, eps);
  h.n_params = net_.n_params();
  h.params_hash = params_hash();

  const uint32_t max_blocks = (uint32_t)Runtime::get().n_cus * 8;
  dd_coords_.ensure(3 * chunk);
  dd_values_.ensure(chunk);
  dd_partials_.ensure((size_t)(max_blocks + 1) * (sizeof(Partial) / sizeof(double)));
  Partial* partials = (Partial*)dd_partials_.ptr;
  Partial* d_result = partials + max_blocks;
  DeviceBuffer<uint32_t> cell_max(MemTag::Network);
  cell_max.resize(n_cells);
  EventGuard ev;
  wait_for(ref.producer, stream, ev);   // the reference is complete once the caller's stream reaches this point

  // pass 1
  worst_init_kernel<<<div_round_up(max_blocks, kBlock), kBlock, 0, stream>>>(partials, max_blocks);
  VNR_HIP_CHECK(hipGetLastError());
  cell_max.zero(stream);
  for (uint64_t b = 0; b < total; b += chunk) {
    const uint64_t e = std::min(total, b + chunk);
    decode_chunk(b, (uint32_t)(e - b), L.bx, L.by, lower, rdims, dd_values_.ptr);
    const uint32_t blocks = chunk_grid(L, ref.type, b, e);
    dispatch_type(ref.type, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      correction_measure_kernel<T><<<blocks, kBlock, 0, stream>>>((const T*)ref.data, L, b, e, dd_values_.ptr, c, k, g, cell_max.ptr, partials);
    });
    VNR_HIP_CHECK(hipGetLastError());
  }
  worst_final_kernel<<<1, kBlock, 0, stream>>>(partials, max_blocks, d_result);
  VNR_HIP_CHECK(hipGetLastError());
  Partial before;
  std::vector<uint32_t> cells(n_cells);
  VNR_HIP_CHECK(hipMemcpyAsync(&before, d_result, sizeof(before), hipMemcpyDeviceToHost, stream));
  cell_max.download(cells.data(), n_cells, stream);   // (synchronises)

  // the table
  const uint32_t ts = (uint32_t)device_value_type_size(ref.type);
  for (uint64_t cl = 0; cl < n_cells; ++cl) {
    const uint32_t m = cells[cl];
    if (m == 0) continue;
    if (m > 0x7fffffffu) throw std::runtime_error("the tolerance needs codes wider than 32 bits: eps " + std::to_string(eps) + " against a maximum error of " + std::to_string(before.max_abs));
    const uint32_t width = kind == kCorrectionVerbatim ? ts : (m <= 127 ? 1u : (m <= 32767 ? 2u : 4u));
    corr->data.cells.push_back(CorrectionCellEntry{(uint32_t)cl, width});
  }
  const uint64_t payload_bytes = correction_fixed_payload_bytes(h, corr->data.cells);
  Partial after = before;   // without a flagged cell every voxel stays as decoded
  if (!corr->data.cells.empty()) {
    const std::vector<CorrectionTableEntry> table = correction_make_table(h, corr->data.cells);
    corr->d_table.upload(table.data(), table.size(), stream);
    corr->d_payload.resize(payload_bytes);
    corr->d_payload.zero(stream);   // (the padding, and what no voxel owns, stays zero)
    // pass 2: the network a second time
    worst_init_kernel<<<div_round_up(max_blocks, kBlock), kBlock, 0, stream>>>(partials, max_blocks);
    VNR_HIP_CHECK(hipGetLastError());
    for (uint64_t b = 0; b < total; b += chunk) {
      const uint64_t e = std::min(total, b + chunk);
      decode_chunk(b, (uint32_t)(e - b), L.bx, L.by, lower, rdims, dd_values_.ptr);
      const uint32_t blocks = chunk_grid(L, ref.type, b, e);
      dispatch_type(ref.type, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        correction_encode_kernel<T><<<blocks, kBlock, 0, stream>>>((const T*)ref.data, L, b, e, dd_values_.ptr, c, k, g, corr->d_table.ptr, corr->d_payload.ptr,
                                                                   partials);
      });
      VNR_HIP_CHECK(hipGetLastError());
    }
    worst_final_kernel<<<1, kBlock, 0, stream>>>(partials, max_blocks, d_result);
    VNR_HIP_CHECK(hipGetLastError());
    VNR_HIP_CHECK(hipMemcpyAsync(&after, d_result, sizeof(after), hipMemcpyDeviceToHost, stream));
    corr->data.payload.resize(payload_bytes);
    corr->d_payload.download(corr->data.payload.data(), payload_bytes, stream);   // (synchronises: `table` and `after` are done with)
  }
  set_report(*corr, before, after, L);
  return corr;
}

namespace {

GroupWalk make_group_walk(vec3i d)
{
  GroupWalk w{};
  w.dx = (uint32_t)d.x; w.dy = (uint32_t)d.y; w.dz = (uint32_t)d.z;
  w.mcx = (w.dx + 15) / 16; w.mcy = (w.dy + 15) / 16; w.mcz = (w.dz + 15) / 16;
  const uint32_t ex[2] = {16, w.dx - 16 * (w.mcx - 1)}, ey[2] = {16, w.dy - 16 * (w.mcy - 1)}, ez[2] = {16, w.dz - 16 * (w.mcz - 1)};
  for (int z = 0; z < 2; ++z) {
    for (int y = 0; y < 2; ++y) {
      for (int x = 0; x < 2; ++x) w.cell_groups[z][y][x] = (ex[x] * ey[y] * ez[z] + 63) / 64;
      w.row_groups[z][y] = (uint64_t)(w.mcx - 1) * w.cell_groups[z][y][0] + w.cell_groups[z][y][1];
    }
    w.layer_groups[z] = (uint64_t)(w.mcy - 1) * w.row_groups[z][0] + w.row_groups[z][1];
  }
  w.n_groups = (uint64_t)(w.mcz - 1) * w.layer_groups[0] + w.layer_groups[1];
  w.narrow = std::max({w.n_groups, w.layer_groups[0], w.row_groups[0][0], w.row_groups[1][0]}) <= 0xffffffffull;
  return w;
}

std::string str_g(double v)
{
  char b[40];
  std::snprintf(b, sizeof(b), "%.17g", v);
  return b;
}

}  // namespace

void NeuralVolume::correction_rates(const DeviceSource& ref, float range_lo, float range_hi, const double* eps, int n_eps, CorrectionRate* out)
{
  if (!net_.valid()) throw std::runtime_error("neural volume has no valid network");
  correction_rates_check(eps, n_eps, out);
  rate_pass(ref, range_lo, range_hi, eps, n_eps, out, nullptr);
}

void NeuralVolume::correction_rates_coded(const DeviceSource& ref, float range_lo, float range_hi, const double* eps, int n_eps, CorrectionRateCoded* out)
{
  if (!net_.valid()) throw std::runtime_error("neural volume has no valid network");
  correction_rates_check(eps, n_eps, out ? &out->rate : nullptr);
  CorrectionRate rates[kCorrectionMaxRates];
  uint64_t words[kCorrectionMaxRates];
  rate_pass(ref, range_lo, range_hi, eps, n_eps, rates, words);
  for (int j = 0; j < n_eps; ++j) {
    CorrectionRateCoded r{rates[j], 0, 0, 0};
    if (!r.rate.refused) {
      r.coded_stream_words = words[j];
      r.coded_payload_bytes = correction_coded_table_bytes(r.rate.n_flagged) + 8 * words[j];
      r.coded_serialized_bytes = kCorrectionHeaderBytes + 8 * r.rate.n_flagged + r.coded_payload_bytes;
    }
    out[j] = r;
  }
}

// the rate pass of both calls.  coded_words null: the plain call, with the kernels, the scratch and the launches it always had;
// otherwise the coded variants of both kernels, 4 more bytes of scratch per macrocell and tolerance, and coded_words[j] = the
// 64-bit words of all streams of tolerance j (whatever it is where the entry is refused)
void NeuralVolume::rate_pass(const DeviceSource& ref, float range_lo, float range_hi, const double* eps, int n_eps, CorrectionRate* out, uint64_t* coded_words)
{
  const vec3i grid = desc.dims;
  vec3i lower;
  const BoxLayout L = validate_box_array(ref.data, ref.type, ref.strides, nullptr, nullptr, grid, lower, range_lo, range_hi);
  const int64_t sx = ref.strides ? ref.strides[0] : 1, sy = ref.strides ? ref.strides[1] : (int64_t)L.bx, sz = ref.strides ? ref.strides[2] : (int64_t)(L.bx * L.by);
  const vec3f rdims = {1.0f / (float)grid.x, 1.0f / (float)grid.y, 1.0f / (float)grid.z};
  const Conversion c{range_lo, range_hi - range_lo, range_lo < range_hi};
  const bool is_float = correction_type_is_float(ref.type);
  const uint32_t ts = (uint32_t)device_value_type_size(ref.type);
  const CellGrid g = make_cell_grid(grid);
  const GroupWalk w = make_group_walk(grid);
  const int dims[3] = {grid.x, grid.y, grid.z};
  const uint64_t n_cells = correction_n_cells(dims);
  // a chunk: whole groups, as many as VNR_AMD_DECODE_CHUNK samples hold (at least one)
  const uint64_t chunk_groups = std::min(std::max<uint64_t>(1, chunk_samples() / 64), w.n_groups);

  std::vector<Quantiser> quantisers(n_eps);
  RateWidths widths{};
  for (int j = 0; j < n_eps; ++j) {
    const uint32_t kind = !is_float ? kCorrectionInteger : (eps[j] > 0.0 ? kCorrectionFloat : kCorrectionVerbatim);
    quantisers[j] = make_quantiser(kind, eps[j]);
    widths.verbatim[j] = kind == kCorrectionVerbatim ? (uint8_t)ts : (uint8_t)0;
  }

  dd_coords_.ensure(3 * 64 * chunk_groups);
  dd_values_.ensure(64 * chunk_groups);
  DeviceBuffer<RateCell> stats(MemTag::Network);
  DeviceBuffer<unsigned long long> nonzero(MemTag::Network);
  DeviceBuffer<RateSums> sums(MemTag::Network);
  stats.resize(n_cells * (uint64_t)n_eps);
  nonzero.resize(n_eps);
  sums.resize(n_eps);
  DeviceBuffer<uint32_t> coded_bits(MemTag::Network);   // the coded call alone: a cell's record bits beyond the 7 of every group
  DeviceBuffer<uint64_t> d_coded_words(MemTag::Network);
  if (coded_words) {
    coded_bits.resize(n_cells * (uint64_t)n_eps);
    d_coded_words.resize(n_eps);
  }
  EventGuard ev;
  wait_for(ref.producer, stream, ev);
  stats.zero(stream);
  nonzero.zero(stream);
  if (coded_words) coded_bits.zero(stream);
  const uint32_t max_blocks = (uint32_t)Runtime::get().n_cus * 8;
  for (uint64_t g0 = 0; g0 < w.n_groups; g0 += chunk_groups) {
    const uint32_t n_groups = (uint32_t)std::min(chunk_groups, w.n_groups - g0), n = 64 * n_groups;
    correction_rate_coords_kernel<<<div_round_up(n, kBlock), kBlock, 0, stream>>>(w, g0, n, rdims, dd_coords_.ptr);
    VNR_HIP_CHECK(hipGetLastError());
    net_.inference(dd_coords_.ptr, dd_values_.ptr, n, nullptr, n, stream);   // the one evaluation of these voxels, whatever n_eps is
    const uint32_t blocks = std::max(1u, std::min(div_round_up(n_groups, kBlock / 64), max_blocks));
    for (int j0 = 0; j0 < n_eps; j0 += kRateBatch) {
      RateBatch batch{};
      batch.n = std::min(kRateBatch, n_eps - j0);
      for (int j = 0; j < batch.n; ++j) batch.k[j] = quantisers[j0 + j];
      dispatch_type(ref.type, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        if (coded_words)
          correction_rate_kernel<T, uint32_t*><<<blocks, kBlock, 0, stream>>>((const T*)ref.data, sx, sy, sz, w, g0, n_groups, dd_values_.ptr, c, batch, n_cells,
                                                                              stats.ptr + (uint64_t)j0 * n_cells, nonzero.ptr + j0,
                                                                              coded_bits.ptr + (uint64_t)j0 * n_cells);
        else
          correction_rate_kernel<T><<<blocks, kBlock, 0, stream>>>((const T*)ref.data, sx, sy, sz, w, g0, n_groups, dd_values_.ptr, c, batch, n_cells,
                                                                   stats.ptr + (uint64_t)j0 * n_cells, nonzero.ptr + j0);
      });
      VNR_HIP_CHECK(hipGetLastError());
    }
  }
  if (coded_words) {
    correction_rate_final_kernel<const uint32_t*, uint64_t*><<<n_eps, kBlock, 0, stream>>>(stats.ptr, n_cells, g, widths, nonzero.ptr, sums.ptr, coded_bits.ptr,
                                                                                             d_coded_words.ptr);
    VNR_HIP_CHECK(hipGetLastError());
    VNR_HIP_CHECK(hipMemcpyAsync(coded_words, d_coded_words.ptr, n_eps * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  } else {
    correction_rate_final_kernel<><<<n_eps, kBlock, 0, stream>>>(stats.ptr, n_cells, g, widths, nonzero.ptr, sums.ptr);
    VNR_HIP_CHECK(hipGetLastError());
  }
  std::vector<RateSums> host(n_eps);
  sums.download(host.data(), n_eps, stream);   // (synchronises)
  for (int j = 0; j < n_eps; ++j) {
    const RateSums& s = host[j];
    CorrectionRate r{};
    r.eps = eps[j];
    r.kind = (int)quantisers[j].kind;
    r.refused = s.refused ? 1 : 0;
    if (!r.refused) {
      r.n_flagged = s.n_flagged; r.n_voxels_flagged = s.n_voxels_flagged; r.n_groups = s.n_groups;
      r.payload_bytes = s.payload_bytes;
      r.serialized_bytes = kCorrectionHeaderBytes + 8 * s.n_flagged + s.payload_bytes;
      r.packed_payload_bytes = correction_group_table_bytes(s.n_groups) + 8 * s.sum_nbits;
      r.packed_serialized_bytes = kCorrectionHeaderBytes + 8 * s.n_flagged + r.packed_payload_bytes;
    }
    out[j] = r;
  }
}

void correction_rates_check(const double* eps, int n_eps, const CorrectionRate* out)
{
  if (!eps) throw std::runtime_error("null eps: the tolerances are missing");
  if (!out) throw std::runtime_error("null result");
  if (n_eps < 1 || n_eps > kCorrectionMaxRates) throw std::runtime_error("n_eps must be 1 .. 64, got " + std::to_string(n_eps));
  for (int k = 0; k < n_eps; ++k)
    if (!(eps[k] >= 0.0) || !std::isfinite(eps[k]))
      throw std::runtime_error("eps[" + std::to_string(k) + "] must be a finite tolerance >= 0 in data units, got " + str_g(eps[k]));
}

void NeuralVolume::decode_to_device_corrected(Correction& corr, const DeviceTarget& out, const int box_lo[3], const int box_size[3], bool verify_params)
{
  if (!net_.valid()) throw std::runtime_error("neural volume has no valid network");
  const CorrectionHeader& h = corr.data.h;
  const vec3i grid = desc.dims;
  if (h.dims[0] != grid.x || h.dims[1] != grid.y || h.dims[2] != grid.z)
    throw std::runtime_error("the correction's dims (" + std::to_string(h.dims[0]) + " x " + std::to_string(h.dims[1]) + " x " + std::to_string(h.dims[2]) +
                             ") differ from the volume's (" + std::to_string(grid.x) + " x " + std::to_string(grid.y) + " x " + std::to_string(grid.z) + ")");
  vec3i lower;
  const BoxLayout L = validate_box_array(out.data, h.value_type, out.strides, box_lo, box_size, grid, lower, h.range_lo, h.range_hi);
  const uint64_t chunk_limit = chunk_samples();
  if (verify_params) verify_correction_params(h);
  if (corr.data.cells.empty()) {   // nothing to apply: the plain decode
    decode_to_device(DeviceTarget{out.data, h.value_type, out.strides, out.consumer}, box_lo, box_size, nullptr, h.range_lo, h.range_hi);
    return;
  }
  correction_make_resident(corr, corr.resident_form, stream);
  const uint64_t total = L.bx * L.by * L.bz, chunk = std::min(chunk_limit, total);
  const vec3f rdims = {1.0f / (float)grid.x, 1.0f / (float)grid.y, 1.0f / (float)grid.z};
  const uint32_t ox = (uint32_t)lower.x, oy = (uint32_t)lower.y, oz = (uint32_t)lower.z;
  const Conversion c{h.range_lo, h.range_hi - h.range_lo, h.range_lo < h.range_hi};
  const Quantiser k = make_quantiser(h.kind, h.eps);
  const CellGrid g = make_cell_grid(grid);
  dd_coords_.ensure(3 * chunk);
  dd_values_.ensure(chunk);
  EventGuard ev;
  wait_for(out.consumer, stream, ev);   // what the destination held may still be being read
  for (uint64_t b = 0; b < total; b += chunk) {
    const uint64_t e = std::min(total, b + chunk);
    decode_chunk(b, (uint32_t)(e - b), L.bx, L.by, lower, rdims, dd_values_.ptr);
    const uint32_t blocks = chunk_grid(L, h.value_type, b, e);
    dispatch_type(h.value_type, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      if (corr.resident_form == 0)
        correction_apply_kernel<T><<<blocks, kBlock, 0, stream>>>((T*)out.data, L, b, e, dd_values_.ptr, c, k, g, ox, oy, oz, corr.d_table.ptr, corr.d_payload.ptr);
      else
        correction_apply_planes_kernel<T><<<blocks, kBlock, 0, stream>>>((T*)out.data, L, b, e, dd_values_.ptr, c, k, g, ox, oy, oz, corr.d_plane_cells.ptr,
                                                                         corr.d_plane_groups.ptr, corr.d_planes());
    });
    VNR_HIP_CHECK(hipGetLastError());
  }
  VNR_HIP_CHECK(hipStreamSynchronize(stream));   // on return the box is there
}

// ---- random access: the two list calls.  Their handles, pointers and alignments have been looked at by the entry points ----------------------
namespace {

// what both refuse before anything runs on a device; returns the chunk limit
uint64_t list_call_check(const CorrectionHeader& h, vec3i grid)
{
  if (h.dims[0] != grid.x || h.dims[1] != grid.y || h.dims[2] != grid.z)
    throw std::runtime_error("the correction's dims (" + std::to_string(h.dims[0]) + " x " + std::to_string(h.dims[1]) + " x " + std::to_string(h.dims[2]) +
                             ") differ from the volume's (" + std::to_string(grid.x) + " x " + std::to_string(grid.y) + " x " + std::to_string(grid.z) + ")");
  return chunk_samples();
}

// the form the kernels read and its pointers; a correction with a flagged cell has been made resident
CorrectionView list_call_view(const Correction& corr, int& form)
{
  form = corr.empty() ? kFormNone : (corr.resident_form == 0 ? kFormFixed : kFormPacked);
  if (form == kFormFixed) return CorrectionView{corr.d_table.ptr, corr.d_payload.ptr, nullptr, nullptr, nullptr};
  if (form == kFormPacked) return CorrectionView{nullptr, nullptr, corr.d_plane_cells.ptr, corr.d_plane_groups.ptr, corr.d_planes()};
  return CorrectionView{nullptr, nullptr, nullptr, nullptr, nullptr};
}

template <typename F>
void dispatch_form(int form, F&& f)
{
  if (form == kFormFixed) f(std::integral_constant<int, kFormFixed>{});
  else if (form == kFormPacked) f(std::integral_constant<int, kFormPacked>{});
  else f(std::integral_constant<int, kFormNone>{});
}

}  // namespace

void NeuralVolume::verify_correction_params(const CorrectionHeader& h)
{
  if (h.n_params != (uint64_t)net_.n_params())
    throw std::runtime_error("the correction was built on " + std::to_string(h.n_params) + " parameters, the volume has " + std::to_string(net_.n_params()));
  if (h.params_hash != params_hash()) throw std::runtime_error("the volume's parameters are not the ones the correction was built on (their hash differs)");
}

void NeuralVolume::gather_voxels_corrected(Correction& corr, size_t n, const int32_t* d_voxels, void* d_out, hipStream_t theirs, bool verify_params)
{
  const CorrectionHeader& h = corr.data.h;
  const vec3i grid = desc.dims;
  const uint64_t chunk = std::min<uint64_t>(list_call_check(h, grid), n);
  if (n == 0) return;
  if (!net_.valid()) throw std::runtime_error("neural volume has no valid network");
  if (verify_params) verify_correction_params(h);
  const size_t ts = device_value_type_size(h.value_type);
  require_room(d_voxels, n * 3 * sizeof(int32_t), "the voxel list");
  require_room(d_out, n * ts, "the result");
  const CellGrid g = make_cell_grid(grid);
  EventGuard ev;
  wait_for(theirs, stream, ev);   // the list is complete, and what the destination held has been read, once the caller's stream reaches this point

  // the whole list is looked at before a voxel is evaluated
  dd_partials_.ensure(1);
  unsigned long long* d_first_bad = (unsigned long long*)dd_partials_.ptr;
  unsigned long long first_bad = ~0ull;
  VNR_HIP_CHECK(hipMemsetAsync(d_first_bad, 0xff, sizeof(first_bad), stream));
  const uint32_t check_blocks = (uint32_t)std::min<uint64_t>((n + kBlock - 1) / kBlock, (uint64_t)Runtime::get().n_cus * 8);
  correction_voxels_check_kernel<<<check_blocks, kBlock, 0, stream>>>(d_voxels, n, g, d_first_bad);
  VNR_HIP_CHECK(hipGetLastError());
  VNR_HIP_CHECK(hipMemcpyAsync(&first_bad, d_first_bad, sizeof(first_bad), hipMemcpyDeviceToHost, stream));
  VNR_HIP_CHECK(hipStreamSynchronize(stream));
  if (first_bad != ~0ull) {
    int32_t v[3];
    VNR_HIP_CHECK(hipMemcpyAsync(v, d_voxels + 3 * first_bad, sizeof(v), hipMemcpyDeviceToHost, stream));
    VNR_HIP_CHECK(hipStreamSynchronize(stream));
    throw std::runtime_error("voxel " + std::to_string(first_bad) + " of the list (" + std::to_string(v[0]) + ", " + std::to_string(v[1]) + ", " + std::to_string(v[2]) +
                             ") is outside the grid " + std::to_string(grid.x) + " x " + std::to_string(grid.y) + " x " + std::to_string(grid.z));
  }

  if (!corr.empty()) correction_make_resident(corr, corr.resident_form, stream);
  int form;
  const CorrectionView view = list_call_view(corr, form);
  const vec3f rdims = {1.0f / (float)grid.x, 1.0f / (float)grid.y, 1.0f / (float)grid.z};
  const Conversion c{h.range_lo, h.range_hi - h.range_lo, h.range_lo < h.range_hi};
  const Quantiser k = make_quantiser(h.kind, h.eps);
  dd_coords_.ensure(3 * chunk);
  dd_values_.ensure(chunk);
  for (uint64_t b = 0; b < n; b += chunk) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - b), blocks = div_round_up(m, kBlock);
    const int32_t* voxels = d_voxels + 3 * b;
    correction_voxel_coords_kernel<<<blocks, kBlock, 0, stream>>>(voxels, m, rdims, dd_coords_.ptr);
    VNR_HIP_CHECK(hipGetLastError());
    net_.inference(dd_coords_.ptr, dd_values_.ptr, m, nullptr, m, stream);
    dispatch_type(h.value_type, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      dispatch_form(form, [&](auto f) {
        correction_gather_kernel<T, decltype(f)::value><<<blocks, kBlock, 0, stream>>>(voxels, m, dd_values_.ptr, c, k, g, view, (T*)d_out + b);
      });
    });
    VNR_HIP_CHECK(hipGetLastError());
  }
  VNR_HIP_CHECK(hipStreamSynchronize(stream));   // on return the values are there
}

void NeuralVolume::sample_corrected(Correction& corr, size_t n, const float* d_coords, float* d_values, hipStream_t theirs, bool verify_params)
{
  const CorrectionHeader& h = corr.data.h;
  const vec3i grid = desc.dims;
  const uint64_t chunk = std::min<uint64_t>(list_call_check(h, grid), n);
  if (n == 0) return;
  if (!net_.valid()) throw std::runtime_error("neural volume has no valid network");
  if (verify_params) verify_correction_params(h);
  require_room(d_coords, n * 3 * sizeof(float), "the coordinates");
  require_room(d_values, n * sizeof(float), "the result");
  if (!corr.empty()) correction_make_resident(corr, corr.resident_form, stream);
  int form;
  const CorrectionView view = list_call_view(corr, form);
  const Conversion c{h.range_lo, h.range_hi - h.range_lo, h.range_lo < h.range_hi};
  const Quantiser k = make_quantiser(h.kind, h.eps);
  const CellGrid g = make_cell_grid(grid);
  EventGuard ev;
  wait_for(theirs, stream, ev);
  for (uint64_t b = 0; b < n; b += chunk) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - b), blocks = div_round_up(m, kBlock);
    net_.inference(d_coords + 3 * b, d_values + b, m, nullptr, m, stream);   // what vnrAmdNeuralVolumeInference gives, corrected in place
    if (form == kFormNone && !c.scale) continue;   // no flagged cell and no range: the inference as it stands
    dispatch_form(form, [&](auto f) {
      correction_sample_kernel<decltype(f)::value><<<blocks, kBlock, 0, stream>>>(d_coords + 3 * b, d_values + b, m, c, k, g, view);
    });
    VNR_HIP_CHECK(hipGetLastError());
  }
  VNR_HIP_CHECK(hipStreamSynchronize(stream));   // on return the values are there
}

// ---- the direct build: field and network -> resident planes plus index, no fixed-width code in between ----------------------------------------
// (include/vnr_amd.h, "corrections built straight into bit planes").  Pass 1 is the rate pass for one tolerance with more taken from
// it: a group's nbits into one byte per group of the GRID, the per-cell pair, and both error reports -- in a cell that ends up not
// flagged every q is 0 and corrected_value(dec, 0) is dec (kind 2: dec has ref's bits), so the error after needs no cell table.  The
// host sees n_cells pairs (correction_direct.cpp).  The index kernel copies the flagged cells' nbits into the packed group table,
// scans them into d_plane_groups and counts the cell's groups that store planes; the scan of guided_sampler.hip turns the counts into
// each cell's place in the list of those groups, so the list is in the walk's order whatever order the waves ran in.  Pass 2 evaluates
// the listed groups alone and stores their planes, lane b plane b, as correction_pack.hip does.
namespace {

static_assert(sizeof(CorrectionDirectStat) == sizeof(RateCell), "the per-cell pair goes to correction_direct_plan as it is");

struct DirectCell { uint64_t grid_group0; uint32_t group0, groups; };   // a flagged cell: its first group in the walk, in the packed table; its groups

// a lane's voxel of a group: ref through the strides, the decoded value, the x-fastest index in the grid
template <typename T>
struct GroupLane {
  bool has;   // the pack fills the other lanes with codes of value 0
  T rv, dec;
  uint64_t index;
};

template <typename T>
__device__ __forceinline__ GroupLane<T> load_group_lane(const T* __restrict__ ref, int64_t sx, int64_t sy, int64_t sz, const GroupWalk& w, const GroupWalk::Place& p,
                                                        uint32_t lane, const float* __restrict__ value, const Conversion& c)
{
  GroupLane<T> v{false, T(0), T(0), 0};
  const uint32_t li = p.group * 64u + lane;
  v.has = li < p.voxels;
  if (v.has) {
    const uint32_t row = li / p.cx, lx = li - row * p.cx, lz = row / p.cy, ly = row - lz * p.cy;
    const uint32_t x = p.x0 + lx, y = p.y0 + ly, z = p.z0 + lz;
    v.rv = ref[(int64_t)x * sx + (int64_t)y * sy + (int64_t)z * sz];
    v.dec = convert_value<T>(*value, c);
    v.index = x + (uint64_t)w.dx * (y + (uint64_t)w.dy * z);
  }
  return v;
}

// the build's code of a voxel and its unsigned z of the packed form
template <typename T>
__device__ __forceinline__ uint64_t code_z(T dec, T rv, const Quantiser& k, int64_t& q, uint32_t& aq, bool& nan)
{
  quantise<T>(dec, rv, k, q, aq, nan);
  if constexpr (std::is_floating_point_v<T>) {
    if (k.kind == kCorrectionVerbatim) return (uint64_t)bits_of(rv);
  }
  return ((uint64_t)q << 1) ^ (uint64_t)(q >> 63);
}

// greater, or equal with the lower index (a NaN never wins): a lane meets its groups in no order of the grid index
__device__ __forceinline__ void take_worst(double& mx, uint64_t& mi, double a, uint64_t i)
{
  if (a > mx || (a == mx && i < mi)) { mx = a; mi = i; }
}

// pass 1.  groups [g0, g0 + n_groups) of the walk, values as in correction_rate_kernel.  group_nbits[group of the grid] gets every
// group's nbits (kind 2: of ref's bit patterns, whether or not the group differs); the cell's pair is folded as the rate kernel folds
// it; before / after: a partial per block, a = voxels with q != 0, b = NaN voxels (before only).
template <typename T>
__global__ void __launch_bounds__(kBlock) correction_direct_measure_kernel(const T* __restrict__ ref, int64_t sx, int64_t sy, int64_t sz, GroupWalk w, uint64_t g0,
                                                                           uint32_t n_groups, const float* __restrict__ values, Conversion c, Quantiser k,
                                                                           RateCell* __restrict__ stats, uint8_t* __restrict__ group_nbits,
                                                                           Partial* __restrict__ before, Partial* __restrict__ after)
{
  const uint32_t lane = threadIdx.x & 63u, waves = kBlock / 64;
  double bmx = -1.0, amx = -1.0;
  uint64_t bmi = ~0ull, ami = ~0ull, n_over = 0, n_nan = 0;
  for (uint32_t g = blockIdx.x * waves + (threadIdx.x >> 6); g < n_groups; g += gridDim.x * waves) {
    const GroupWalk::Place p = w.place(g0 + g);
    const GroupLane<T> v = load_group_lane<T>(ref, sx, sy, sz, w, p, lane, values + ((size_t)g * 64 + lane), c);
    int64_t q = 0; uint32_t aq = 0; bool nan = false;
    uint64_t z = 0;
    if (v.has) {
      z = code_z<T>(v.dec, v.rv, k, q, aq, nan);
      take_worst(bmx, bmi, fabs((double)v.dec - (double)v.rv), v.index);
      T out = corrected_value<T>(v.dec, q, k);
      if constexpr (std::is_floating_point_v<T>) {
        if (k.kind == kCorrectionVerbatim) out = v.rv;
      }
      take_worst(amx, ami, fabs((double)out - (double)v.rv), v.index);
      n_over += aq ? 1 : 0;
      n_nan += nan ? 1 : 0;
    }
    const uint64_t differ = __ballot(q != 0);
    const uint32_t nbits = wave_max(z ? 64u - (uint32_t)__clzll((long long)z) : 0u);
    const uint32_t m = wave_max(aq);
    if (lane == 0) {
      group_nbits[g0 + g] = (uint8_t)nbits;
      if (differ != 0 || k.kind == kCorrectionVerbatim) {
        RateCell* s = stats + p.cell;
        if (m) atomicMax(&s->max_q, m);
        if (nbits) atomicAdd(&s->nbits, nbits);
      }
    }
  }
  block_reduce(bmx, bmi, n_over, n_nan);
  if (threadIdx.x == 0) merge_partial<uint64_t>(before, bmx, bmi, n_over, n_nan);
  __syncthreads();   // (block_reduce's LDS is read by thread 0 until here)
  uint64_t na = 0, nb = 0;
  block_reduce(amx, ami, na, nb);
  if (threadIdx.x == 0) merge_partial<uint64_t>(after, amx, ami, 0, 0);
}

// exclusive prefix sum over the lanes of a wave
__device__ __forceinline__ uint32_t wave_exclusive_sum(uint32_t v, uint32_t lane)
{
  uint32_t incl = v;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(incl, off, 64);
    if (lane >= (uint32_t)off) incl += t;
  }
  return incl - v;
}

// the index: a block is one wave and takes flagged cells by block stride, lane g the cell's group g (a cell has at most 64)
__global__ void __launch_bounds__(64) correction_direct_index_kernel(const DirectCell* __restrict__ cells, uint32_t n_cells, const uint8_t* __restrict__ group_nbits,
                                                                     uint8_t* __restrict__ table, uint32_t* __restrict__ plane_groups, uint64_t* __restrict__ stored)
{
  const uint32_t lane = threadIdx.x;
  for (uint64_t c = blockIdx.x; c < n_cells; c += gridDim.x) {
    const DirectCell dc = cells[c];
    const uint32_t nbits = lane < dc.groups ? group_nbits[dc.grid_group0 + lane] : 0u;
    const uint32_t first = wave_exclusive_sum(nbits, lane);   // at most 63 * 64
    if (lane < dc.groups) {
      table[dc.group0 + lane] = (uint8_t)nbits;
      plane_groups[dc.group0 + lane] = first | nbits << 16;
    }
    const uint64_t with_planes = __ballot(nbits != 0);
    if (lane == 0) stored[c] = (uint64_t)__popcll(with_planes);
  }
}

// stored: now the inclusive sums of the cells' counts.  The cell's groups that store planes go to the list, in their order
__global__ void __launch_bounds__(64) correction_direct_list_kernel(const DirectCell* __restrict__ cells, uint32_t n_cells, const uint32_t* __restrict__ plane_groups,
                                                                    const uint64_t* __restrict__ stored, uint64_t* __restrict__ list)
{
  const uint32_t lane = threadIdx.x;
  for (uint64_t c = blockIdx.x; c < n_cells; c += gridDim.x) {
    const DirectCell dc = cells[c];
    const uint32_t nbits = lane < dc.groups ? plane_groups[dc.group0 + lane] >> 16 : 0u;
    const uint64_t with_planes = __ballot(nbits != 0);
    const uint64_t first = stored[c] - (uint64_t)__popcll(with_planes);
    if (nbits) list[first + (uint64_t)__popcll(with_planes & ((1ull << lane) - 1ull))] = dc.grid_group0 + lane;
  }
}

// pass 2.  groups list[0 .. n_groups) of the walk, all of flagged cells and with nbits > 0, values[64 * g + lane]: z again, one ballot
// per plane, lane b keeps plane b, one 8-byte store per lane at the cell's first word + the group's
template <typename T>
__global__ void __launch_bounds__(kBlock) correction_direct_planes_kernel(const T* __restrict__ ref, int64_t sx, int64_t sy, int64_t sz, GroupWalk w,
                                                                          const uint64_t* __restrict__ list, uint32_t n_groups, const float* __restrict__ values,
                                                                          Conversion c, Quantiser k, const Correction::PlaneCell* __restrict__ cells,
                                                                          const uint32_t* __restrict__ plane_groups, uint64_t* __restrict__ planes)
{
  const uint32_t lane = threadIdx.x & 63u, waves = kBlock / 64;
  for (uint32_t g = blockIdx.x * waves + (threadIdx.x >> 6); g < n_groups; g += gridDim.x * waves) {
    const GroupWalk::Place p = w.place(list[g]);
    const GroupLane<T> v = load_group_lane<T>(ref, sx, sy, sz, w, p, lane, values + ((size_t)g * 64 + lane), c);
    int64_t q; uint32_t aq; bool nan;
    const uint64_t z = v.has ? code_z<T>(v.dec, v.rv, k, q, aq, nan) : 0ull;   // a lane beyond its cell's voxels contributes 0
    const Correction::PlaneCell pc = cells[p.cell];
    const uint32_t gi = (uint32_t)__builtin_amdgcn_readfirstlane((int)plane_groups[pc.group0 + p.group]);
    const uint32_t nb = std::min(gi >> 16, 64u);
    uint64_t keep = 0;
    for (uint32_t b = 0; b < nb; ++b) {
      const uint64_t plane = __ballot((int)((z >> b) & 1));
      if (lane == b) keep = plane;
    }
    if (lane < nb) planes[pc.word0 + (gi & 0xffffu) + lane] = keep;
  }
}

}  // namespace

std::shared_ptr<Correction> NeuralVolume::build_correction_packed(const DeviceSource& ref, float range_lo, float range_hi, double eps)
{
  if (!net_.valid()) throw std::runtime_error("neural volume has no valid network");
  if (!(eps >= 0.0) || !std::isfinite(eps)) throw std::runtime_error("eps must be a finite tolerance >= 0 in data units, got " + std::to_string(eps));
  const vec3i grid = desc.dims;
  vec3i lower;
  const BoxLayout L = validate_box_array(ref.data, ref.type, ref.strides, nullptr, nullptr, grid, lower, range_lo, range_hi);
  const int64_t sx = ref.strides ? ref.strides[0] : 1, sy = ref.strides ? ref.strides[1] : (int64_t)L.bx, sz = ref.strides ? ref.strides[2] : (int64_t)(L.bx * L.by);
  const vec3f rdims = {1.0f / (float)grid.x, 1.0f / (float)grid.y, 1.0f / (float)grid.z};
  const Conversion c{range_lo, range_hi - range_lo, range_lo < range_hi};
  const bool is_float = correction_type_is_float(ref.type);
  const uint32_t kind = !is_float ? kCorrectionInteger : (eps > 0.0 ? kCorrectionFloat : kCorrectionVerbatim);
  const Quantiser k = make_quantiser(kind, eps);
  const GroupWalk w = make_group_walk(grid);
  const int dims[3] = {grid.x, grid.y, grid.z};
  const uint64_t n_cells = correction_n_cells(dims);
  const uint64_t chunk_groups = std::min(std::max<uint64_t>(1, chunk_samples() / 64), w.n_groups);   // whole groups, as the rate pass

  auto corr = std::make_shared<Correction>(CorrectionOrigin::BuiltDirect);
  CorrectionHeader& h = corr->data.h;
  h.value_type = ref.type;
  for (int a = 0; a < 3; ++a) h.dims[a] = dims[a];
  h.eps = eps; h.range_lo = range_lo; h.range_hi = range_hi; h.kind = kind;
  h.step = correction_step(kind, eps);
  h.n_params = net_.n_params();
  h.params_hash = params_hash();

  const uint32_t max_blocks = (uint32_t)Runtime::get().n_cus * 8;
  dd_coords_.ensure(3 * 64 * chunk_groups);
  dd_values_.ensure(64 * chunk_groups);
  dd_partials_.ensure((size_t)2 * (max_blocks + 1) * (sizeof(Partial) / sizeof(double)));
  Partial* before_partials = (Partial*)dd_partials_.ptr;
  Partial* after_partials = before_partials + (max_blocks + 1);
  DeviceBuffer<RateCell> stats(MemTag::Network);
  DeviceBuffer<uint8_t> group_nbits(MemTag::Network);
  stats.resize(n_cells);
  group_nbits.resize(w.n_groups);   // (every byte is written by pass 1)
  EventGuard ev;
  wait_for(ref.producer, stream, ev);

  // pass 1
  worst_init_kernel<<<div_round_up(2 * (max_blocks + 1), kBlock), kBlock, 0, stream>>>(before_partials, 2 * (max_blocks + 1));
  VNR_HIP_CHECK(hipGetLastError());
  stats.zero(stream);
  for (uint64_t g0 = 0; g0 < w.n_groups; g0 += chunk_groups) {
    const uint32_t n_groups = (uint32_t)std::min(chunk_groups, w.n_groups - g0), n = 64 * n_groups;
    correction_rate_coords_kernel<<<div_round_up(n, kBlock), kBlock, 0, stream>>>(w, g0, n, rdims, dd_coords_.ptr);
    VNR_HIP_CHECK(hipGetLastError());
    net_.inference(dd_coords_.ptr, dd_values_.ptr, n, nullptr, n, stream);
    const uint32_t blocks = std::max(1u, std::min(div_round_up(n_groups, kBlock / 64), max_blocks));
    dispatch_type(ref.type, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      correction_direct_measure_kernel<T><<<blocks, kBlock, 0, stream>>>((const T*)ref.data, sx, sy, sz, w, g0, n_groups, dd_values_.ptr, c, k, stats.ptr,
                                                                         group_nbits.ptr, before_partials, after_partials);
    });
    VNR_HIP_CHECK(hipGetLastError());
  }
  worst_final_kernel<<<1, kBlock, 0, stream>>>(before_partials, max_blocks, before_partials + max_blocks);
  VNR_HIP_CHECK(hipGetLastError());
  worst_final_kernel<<<1, kBlock, 0, stream>>>(after_partials, max_blocks, after_partials + max_blocks);
  VNR_HIP_CHECK(hipGetLastError());
  Partial before, after;
  std::vector<CorrectionDirectStat> cells(n_cells);
  VNR_HIP_CHECK(hipMemcpyAsync(&before, before_partials + max_blocks, sizeof(before), hipMemcpyDeviceToHost, stream));
  VNR_HIP_CHECK(hipMemcpyAsync(&after, after_partials + max_blocks, sizeof(after), hipMemcpyDeviceToHost, stream));
  VNR_HIP_CHECK(hipMemcpyAsync(cells.data(), stats.ptr, n_cells * sizeof(RateCell), hipMemcpyDeviceToHost, stream));
  VNR_HIP_CHECK(hipStreamSynchronize(stream));

  // the host: n_cells pairs in, the entries and the flagged cells' places out
  const CorrectionDirectPlan plan = correction_direct_plan(dims, kind, (uint32_t)device_value_type_size(ref.type), cells.data(), n_cells);
  if (plan.refused)
    throw std::runtime_error("the tolerance needs codes wider than 32 bits: eps " + std::to_string(eps) + " against a maximum error of " + std::to_string(before.max_abs));
  if (plan.n_groups > 0xffffffffull) throw std::runtime_error("the correction has more than 2^32 groups");
  corr->data.cells = plan.cells;
  set_report(*corr, before, after, L);
  corr->resident_form = 1;
  if (plan.cells.empty()) return corr;   // holds nothing, as every correction without a flagged cell

  const uint32_t n_flagged = (uint32_t)plan.cells.size();
  const uint64_t table_bytes = correction_group_table_bytes(plan.n_groups);
  std::vector<Correction::PlaneCell> plane_cells(n_cells, Correction::PlaneCell{~0ull, 0, 0});
  std::vector<DirectCell> direct_cells(n_flagged);
  for (uint32_t i = 0; i < n_flagged; ++i) {
    const CorrectionDirectPlace& at = plan.places[i];
    plane_cells[plan.cells[i].cell] = Correction::PlaneCell{at.word0, (uint32_t)at.group0, 0};
    direct_cells[i] = DirectCell{at.grid_group0, (uint32_t)at.group0, (uint32_t)correction_cell_groups(correction_cell_voxels(dims, plan.cells[i].cell))};
  }
  DeviceBuffer<DirectCell> d_cells(MemTag::Network);
  DeviceBuffer<uint64_t> stored(MemTag::Network), scan_scratch(MemTag::Network), list(MemTag::Network);
  d_cells.upload(direct_cells.data(), n_flagged, stream);
  corr->d_plane_cells.upload(plane_cells.data(), n_cells, stream);
  corr->d_plane_groups.resize(plan.n_groups);
  corr->d_packed.resize(table_bytes + 8 * plan.n_words);
  VNR_HIP_CHECK(hipMemsetAsync(corr->d_packed.ptr, 0, table_bytes, stream));   // (the table's padding)
  stored.resize(n_flagged);
  const uint32_t cell_blocks = std::min(n_flagged, 1u << 20);
  correction_direct_index_kernel<<<cell_blocks, 64, 0, stream>>>(d_cells.ptr, n_flagged, group_nbits.ptr, corr->d_packed.ptr, corr->d_plane_groups.ptr, stored.ptr);
  VNR_HIP_CHECK(hipGetLastError());
  device_inclusive_scan(stored.ptr, n_flagged, scan_scratch, stream);
  uint64_t n_stored = 0;   // groups with planes: one count, no code, crosses to the host
  VNR_HIP_CHECK(hipMemcpyAsync(&n_stored, stored.ptr + (n_flagged - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  VNR_HIP_CHECK(hipStreamSynchronize(stream));   // (the host vectors above are done with, too)
  if (n_stored > plan.n_groups) throw std::runtime_error("internal error: more groups store planes than the flagged cells have");
  if (n_stored) {
    list.resize(n_stored);
    correction_direct_list_kernel<<<cell_blocks, 64, 0, stream>>>(d_cells.ptr, n_flagged, corr->d_plane_groups.ptr, stored.ptr, list.ptr);
    VNR_HIP_CHECK(hipGetLastError());
    uint64_t* planes = reinterpret_cast<uint64_t*>(corr->d_packed.ptr + table_bytes);
    // pass 2: the network a second time, for the groups that store planes alone
    for (uint64_t l0 = 0; l0 < n_stored; l0 += chunk_groups) {
      const uint32_t n_groups = (uint32_t)std::min(chunk_groups, n_stored - l0), n = 64 * n_groups;
      correction_list_coords_kernel<<<div_round_up(n, kBlock), kBlock, 0, stream>>>(w, list.ptr + l0, n, rdims, dd_coords_.ptr);
      VNR_HIP_CHECK(hipGetLastError());
      net_.inference(dd_coords_.ptr, dd_values_.ptr, n, nullptr, n, stream);
      const uint32_t blocks = std::max(1u, std::min(div_round_up(n_groups, kBlock / 64), max_blocks));
      dispatch_type(ref.type, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        correction_direct_planes_kernel<T><<<blocks, kBlock, 0, stream>>>((const T*)ref.data, sx, sy, sz, w, list.ptr + l0, n_groups, dd_values_.ptr, c, k,
                                                                          corr->d_plane_cells.ptr, corr->d_plane_groups.ptr, planes);
      });
      VNR_HIP_CHECK(hipGetLastError());
    }
    VNR_HIP_CHECK(hipStreamSynchronize(stream));   // the scratch of this call goes out of scope
  }
  return corr;
}

}  // namespace vnr
