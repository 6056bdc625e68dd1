// correction_format.cpp — writer and validating reader of a serialised correction (correction_format.h).  Host only.
#include "correction_format.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

namespace vnr {

namespace {

const char kMagic[8] = {'V', 'N', 'R', 'C', 'O', 'R', 'R', '1'};

// (the library is built for little-endian hosts only, like its BSON reader: values are copied as they lie in memory)
template <typename T> void put(std::vector<uint8_t>& out, T v)
{
  uint8_t b[sizeof(T)];
  std::memcpy(b, &v, sizeof(T));
  out.insert(out.end(), b, b + sizeof(T));
}
template <typename T> T get(const uint8_t* p)
{
  T v;
  std::memcpy(&v, p, sizeof(T));
  return v;
}

[[noreturn]] void refuse(const std::string& what) { throw std::runtime_error("malformed correction bytes: " + what); }

}  // namespace

size_t correction_type_size(int t)
{
  switch (t) {
  case 0: case 1: return 1;
  case 2: case 3: return 2;
  case 4: case 5: case 8: return 4;
  case 12: return 8;
  default: return 0;
  }
}

uint64_t correction_n_cells(const int dims[3])
{
  unsigned __int128 n = 1;
  for (int a = 0; a < 3; ++a) n *= (uint64_t)((dims[a] > 0 ? (int64_t)dims[a] : 0) + kCorrectionCell - 1) / kCorrectionCell;
  return n > (unsigned __int128)UINT64_MAX ? UINT64_MAX : (uint64_t)n;
}

uint64_t correction_cell_voxels(const int dims[3], uint32_t cell)
{
  const uint64_t mx = ((uint64_t)dims[0] + 15) / 16, my = ((uint64_t)dims[1] + 15) / 16;
  const uint64_t ix = cell % mx, iy = (cell / mx) % my, iz = cell / (mx * my);
  const uint64_t cx = std::min<uint64_t>(16, (uint64_t)dims[0] - 16 * ix), cy = std::min<uint64_t>(16, (uint64_t)dims[1] - 16 * iy),
                 cz = std::min<uint64_t>(16, (uint64_t)dims[2] - 16 * iz);
  return cx * cy * cz;
}

uint64_t correction_step(uint32_t kind, double eps)
{
  if (kind == kCorrectionInteger) return 2 * (uint64_t)std::floor(std::min(eps, kCorrectionMaxIntegerEps)) + 1;
  if (kind == kCorrectionFloat) {
    const double s = 2.0 * eps;
    return get<uint64_t>((const uint8_t*)&s);
  }
  return 0;
}

uint64_t fnv1a64(const void* bytes, size_t size)
{
  uint64_t h = 0xcbf29ce484222325ull;
  const uint8_t* p = (const uint8_t*)bytes;
  for (size_t i = 0; i < size; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
  return h;
}

std::vector<uint8_t> correction_write(const CorrectionData& c)
{
  std::vector<uint8_t> out;
  out.reserve(correction_serialized_bytes(c));
  out.insert(out.end(), kMagic, kMagic + 8);
  put<uint32_t>(out, 1);
  put<uint32_t>(out, (uint32_t)c.h.value_type);
  for (int a = 0; a < 3; ++a) put<int32_t>(out, c.h.dims[a]);
  put<uint32_t>(out, (uint32_t)c.cells.size());
  put<double>(out, c.h.eps);
  put<float>(out, c.h.range_lo);
  put<float>(out, c.h.range_hi);
  put<uint32_t>(out, c.h.kind);
  put<uint32_t>(out, 0);
  put<uint64_t>(out, c.h.step);
  put<uint64_t>(out, c.h.params_hash);
  put<uint64_t>(out, c.h.n_params);
  put<uint64_t>(out, (uint64_t)c.payload.size());
  put<double>(out, c.h.max_abs_after);
  put<uint64_t>(out, 0);
  for (const CorrectionCellEntry& e : c.cells) { put<uint32_t>(out, e.cell); put<uint32_t>(out, e.width); }
  out.insert(out.end(), c.payload.begin(), c.payload.end());
  return out;
}

CorrectionData correction_parse(const void* bytes, size_t size)
{
  if (!bytes) refuse("null bytes");
  const uint8_t* p = (const uint8_t*)bytes;
  if (size < kCorrectionHeaderBytes) refuse("the size (" + std::to_string(size) + " bytes) is shorter than the header");
  if (std::memcmp(p, kMagic, 8) != 0) refuse("bad magic");
  if (get<uint32_t>(p + 8) != 1) refuse("unsupported version " + std::to_string(get<uint32_t>(p + 8)));
  CorrectionData c;
  CorrectionHeader& h = c.h;
  const uint32_t type = get<uint32_t>(p + 12);
  if (type > 12 || correction_type_size((int)type) == 0) refuse("unknown value type " + std::to_string(type));
  h.value_type = (int)type;
  const size_t ts = correction_type_size(h.value_type);
  for (int a = 0; a < 3; ++a) h.dims[a] = get<int32_t>(p + 16 + 4 * a);
  if (h.dims[0] <= 0 || h.dims[1] <= 0 || h.dims[2] <= 0)
    refuse("dims must be positive: " + std::to_string(h.dims[0]) + " x " + std::to_string(h.dims[1]) + " x " + std::to_string(h.dims[2]));
  const uint64_t n_cells = correction_n_cells(h.dims);
  if (n_cells > 0xffffffffull) refuse("the dims give more than 2^32 cells");
  const uint32_t n_flagged = get<uint32_t>(p + 28);
  if (n_flagged > n_cells) refuse("n_flagged (" + std::to_string(n_flagged) + ") exceeds the number of cells (" + std::to_string(n_cells) + ")");
  h.eps = get<double>(p + 32);
  h.range_lo = get<float>(p + 40);
  h.range_hi = get<float>(p + 44);
  h.kind = get<uint32_t>(p + 48);
  if (get<uint32_t>(p + 52) != 0 || get<uint64_t>(p + 96) != 0) refuse("a reserved field is not zero");
  h.step = get<uint64_t>(p + 56);
  h.params_hash = get<uint64_t>(p + 64);
  h.n_params = get<uint64_t>(p + 72);
  const uint64_t payload_bytes = get<uint64_t>(p + 80);
  h.max_abs_after = get<double>(p + 88);
  if (h.kind > kCorrectionVerbatim) refuse("unknown kind " + std::to_string(h.kind));
  const bool is_float = correction_type_is_float(h.value_type);
  const bool consistent = std::isfinite(h.eps) && h.eps >= 0.0 &&
                          (h.kind == kCorrectionInteger ? !is_float : (is_float && (h.kind == kCorrectionFloat ? h.eps > 0.0 : h.eps == 0.0))) &&
                          h.step == correction_step(h.kind, h.eps);
  if (!consistent) refuse("kind, step and eps are inconsistent (kind " + std::to_string(h.kind) + ", value type " + std::to_string(type) + ")");
  if ((size - kCorrectionHeaderBytes) / 8 < n_flagged) refuse("the size is shorter than the cell entries");
  const uint8_t* entries = p + kCorrectionHeaderBytes;
  uint64_t sum = 0, previous = 0;
  for (uint32_t i = 0; i < n_flagged; ++i) {
    const uint32_t cell = get<uint32_t>(entries + 8 * (size_t)i), width = get<uint32_t>(entries + 8 * (size_t)i + 4);
    if (cell >= n_cells) refuse("cell " + std::to_string(cell) + " is out of range (" + std::to_string(n_cells) + " cells)");
    if (i > 0 && cell <= previous) refuse("cells must be strictly ascending");
    previous = cell;
    const bool legal = h.kind == kCorrectionVerbatim ? width == ts : (width == 1 || width == 2 || width == 4);
    if (!legal) refuse("illegal code width " + std::to_string(width) + " for kind " + std::to_string(h.kind));
    sum += correction_padded_bytes(correction_cell_voxels(h.dims, cell), width);
  }
  if (payload_bytes != sum)
    refuse("payload_bytes (" + std::to_string(payload_bytes) + ") differs from the sum of the padded cell sizes (" + std::to_string(sum) + ")");
  const uint64_t rest = (uint64_t)(size - kCorrectionHeaderBytes) - 8ull * n_flagged;
  if (rest != payload_bytes) refuse("the size differs from header + entries + payload (" + std::to_string(rest) + " payload bytes present, " + std::to_string(payload_bytes) + " declared)");
  c.cells.resize(n_flagged);
  for (uint32_t i = 0; i < n_flagged; ++i) c.cells[i] = CorrectionCellEntry{get<uint32_t>(entries + 8 * (size_t)i), get<uint32_t>(entries + 8 * (size_t)i + 4)};
  const uint8_t* payload = entries + 8 * (size_t)n_flagged;
  c.payload.assign(payload, payload + payload_bytes);
  return c;
}

}  // namespace vnr
