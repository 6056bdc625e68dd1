// correction_format.h — the serialised form of an error-bound correction (include/vnr_amd.h, "error-bounded round trip"): layout,
// writer and validating reader.  Host only, no HIP include (like json.h): tests build it with the host compiler under sanitizers.
//
// Little-endian.  Header (kCorrectionHeaderBytes), then n_flagged entries {uint32 cell, uint32 width}, then the payload:
//   char[8] magic "VNRCORR1" | u32 version = 1 | u32 value_type | i32 dims[3] | u32 n_flagged | f64 eps | f32 range_lo | f32 range_hi |
//   u32 kind | u32 reserved = 0 | u64 step | u64 params_hash | u64 n_params | u64 payload_bytes | f64 max_abs_after | u64 reserved = 0
// The payload holds, cell after cell in ascending cell index, the codes of every voxel of the cell (order lx + cx * (ly + cy * lz), the
// cell's own ragged extents), `width` bytes each, little-endian signed (kind 2: the bit pattern of the value), padded with zero
// bytes to a multiple of 16 bytes per cell.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace vnr {

constexpr size_t kCorrectionHeaderBytes = 104;
constexpr int kCorrectionCell = 16;                       // the macrocell edge (volume.h kMacrocellSize)
constexpr double kCorrectionMaxIntegerEps = 1099511627776.0;   // 2^40: floor(eps) is taken of min(eps, this); no 32-bit voxel can miss 2^32

enum CorrectionKind : uint32_t { kCorrectionInteger = 0, kCorrectionFloat = 1, kCorrectionVerbatim = 2 };

struct CorrectionHeader {
  int value_type = 8;
  int dims[3] = {0, 0, 0};
  double eps = 0.0;
  float range_lo = 0.0f, range_hi = 0.0f;
  uint32_t kind = 0;
  uint64_t step = 0;            // kind 0: 2 floor(eps) + 1; kind 1: the bits of the double 2 eps; kind 2: 0
  uint64_t params_hash = 0, n_params = 0;
  double max_abs_after = 0.0;
};

struct CorrectionCellEntry { uint32_t cell, width; };

struct CorrectionData {
  CorrectionHeader h;
  std::vector<CorrectionCellEntry> cells;   // strictly ascending
  std::vector<uint8_t> payload;
};

// bytes of a value type a correction may have; 0 for every other type
size_t correction_type_size(int value_type);
inline bool correction_type_is_float(int value_type) { return value_type == 8 || value_type == 12; }
uint64_t correction_n_cells(const int dims[3]);
// voxels of a macrocell (ragged at the upper faces); the cell must be in range
uint64_t correction_cell_voxels(const int dims[3], uint32_t cell);
inline uint64_t correction_padded_bytes(uint64_t voxels, uint32_t width) { return (voxels * width + 15) / 16 * 16; }
// the step the header carries for this kind and tolerance
uint64_t correction_step(uint32_t kind, double eps);
uint64_t fnv1a64(const void* bytes, size_t size);

inline size_t correction_serialized_bytes(const CorrectionData& c) { return kCorrectionHeaderBytes + 8 * c.cells.size() + c.payload.size(); }
std::vector<uint8_t> correction_write(const CorrectionData& c);
// throws std::runtime_error that names the rule the bytes break; everything is validated before anything is allocated by their say
CorrectionData correction_parse(const void* bytes, size_t size);

}  // namespace vnr
