// correction_packed_format.cpp — writer, validating reader and host unpack of a packed correction (correction_packed_format.h).  Host only.
// The header and entry rules are correction_format.cpp's, restated: that reader checks its own magic first and copies a payload.
#include "correction_packed_format.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

namespace vnr {

namespace {

const char kMagic[8] = {'V', 'N', 'R', 'C', 'O', 'R', 'P', '1'};

// (little-endian hosts only, like correction_format.cpp: values are copied as they lie in memory)
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

[[noreturn]] void refuse(const std::string& what) { throw std::runtime_error("malformed packed correction bytes: " + what); }

// the lanes of group k of a cell that hold a voxel's code, as a mask
uint64_t lane_mask(uint64_t voxels, uint64_t k)
{
  const uint64_t lanes = voxels - kCorrectionGroup * k;
  return lanes >= kCorrectionGroup ? ~0ull : (1ull << lanes) - 1;
}

}  // namespace

std::vector<CorrectionCellLayout> correction_cell_layout(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells)
{
  std::vector<CorrectionCellLayout> out;
  out.reserve(cells.size());
  uint64_t codes = 0, group = 0;
  for (const CorrectionCellEntry& e : cells) {
    const uint64_t voxels = correction_cell_voxels(h.dims, e.cell), groups = correction_cell_groups(voxels);
    out.push_back(CorrectionCellLayout{codes, group, (uint32_t)voxels, (uint32_t)groups});
    codes += correction_padded_bytes(voxels, e.width);
    group += groups;
  }
  return out;
}

uint64_t correction_n_groups(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells)
{
  uint64_t n = 0;
  for (const CorrectionCellEntry& e : cells) n += correction_cell_groups(correction_cell_voxels(h.dims, e.cell));
  return n;
}

uint64_t correction_fixed_payload_bytes(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells)
{
  uint64_t n = 0;
  for (const CorrectionCellEntry& e : cells) n += correction_padded_bytes(correction_cell_voxels(h.dims, e.cell), e.width);
  return n;
}

std::vector<uint8_t> correction_packed_write(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const std::vector<uint8_t>& payload)
{
  std::vector<uint8_t> out;
  out.reserve(kCorrectionHeaderBytes + 8 * cells.size() + payload.size());
  out.insert(out.end(), kMagic, kMagic + 8);
  put<uint32_t>(out, 1);
  put<uint32_t>(out, (uint32_t)h.value_type);
  for (int a = 0; a < 3; ++a) put<int32_t>(out, h.dims[a]);
  put<uint32_t>(out, (uint32_t)cells.size());
  put<double>(out, h.eps);
  put<float>(out, h.range_lo);
  put<float>(out, h.range_hi);
  put<uint32_t>(out, h.kind);
  put<uint32_t>(out, 0);
  put<uint64_t>(out, h.step);
  put<uint64_t>(out, h.params_hash);
  put<uint64_t>(out, h.n_params);
  put<uint64_t>(out, (uint64_t)payload.size());
  put<double>(out, h.max_abs_after);
  put<uint64_t>(out, 0);
  for (const CorrectionCellEntry& e : cells) { put<uint32_t>(out, e.cell); put<uint32_t>(out, e.width); }
  out.insert(out.end(), payload.begin(), payload.end());
  return out;
}

CorrectionPacked correction_packed_parse(const void* bytes, size_t size)
{
  if (!bytes) refuse("null bytes");
  const uint8_t* p = (const uint8_t*)bytes;
  if (size < kCorrectionHeaderBytes) refuse("the size (" + std::to_string(size) + " bytes) is shorter than the header");
  if (std::memcmp(p, kMagic, 8) != 0) refuse("bad magic");
  if (get<uint32_t>(p + 8) != 1) refuse("unsupported version " + std::to_string(get<uint32_t>(p + 8)));
  CorrectionPacked c;
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
  uint64_t n_groups = 0, previous = 0;
  for (uint32_t i = 0; i < n_flagged; ++i) {
    const uint32_t cell = get<uint32_t>(entries + 8 * (size_t)i), width = get<uint32_t>(entries + 8 * (size_t)i + 4);
    if (cell >= n_cells) refuse("cell " + std::to_string(cell) + " is out of range (" + std::to_string(n_cells) + " cells)");
    if (i > 0 && cell <= previous) refuse("cells must be strictly ascending");
    previous = cell;
    const bool legal = h.kind == kCorrectionVerbatim ? width == ts : (width == 1 || width == 2 || width == 4);
    if (!legal) refuse("illegal code width " + std::to_string(width) + " for kind " + std::to_string(h.kind));
    n_groups += correction_cell_groups(correction_cell_voxels(h.dims, cell));   // (at most 2^32 cells of 64 groups)
  }
  const uint64_t rest = (uint64_t)(size - kCorrectionHeaderBytes) - 8ull * n_flagged;
  if (rest != payload_bytes) refuse("the size differs from header + entries + payload (" + std::to_string(rest) + " payload bytes present, " + std::to_string(payload_bytes) + " declared)");
  const uint64_t table_bytes = correction_group_table_bytes(n_groups);
  if (payload_bytes < table_bytes) refuse("payload_bytes (" + std::to_string(payload_bytes) + ") is shorter than the group table (" + std::to_string(table_bytes) + " bytes)");

  // the group table: every nbits within its cell's width, the padding zero, the planes it announces exactly what is there
  const uint8_t* table = entries + 8 * (size_t)n_flagged;
  uint64_t g = 0, words = 0;
  for (uint32_t i = 0; i < n_flagged; ++i) {
    const uint32_t cell = get<uint32_t>(entries + 8 * (size_t)i), width = get<uint32_t>(entries + 8 * (size_t)i + 4);
    const uint64_t groups = correction_cell_groups(correction_cell_voxels(h.dims, cell));
    for (uint64_t k = 0; k < groups; ++k, ++g) {
      if (table[g] > 8 * width) refuse("nbits " + std::to_string(table[g]) + " of group " + std::to_string(g) + " exceeds 8 * width (width " + std::to_string(width) + ")");
      words += table[g];
    }
  }
  for (; g < table_bytes; ++g)
    if (table[g] != 0) refuse("nonzero group table padding");
  if (payload_bytes - table_bytes != 8 * words)
    refuse("payload_bytes (" + std::to_string(payload_bytes) + ") differs from the sum the group table gives (" + std::to_string(table_bytes + 8 * words) + ")");

  // the planes: canonical (the top plane of a group is not empty), nothing in a lane that has no voxel
  const uint8_t* planes = table + table_bytes;
  uint64_t w = 0;
  g = 0;
  for (uint32_t i = 0; i < n_flagged; ++i) {
    const uint64_t voxels = correction_cell_voxels(h.dims, get<uint32_t>(entries + 8 * (size_t)i)), groups = correction_cell_groups(voxels);
    for (uint64_t k = 0; k < groups; ++k, ++g) {
      const uint32_t nbits = table[g];
      if (nbits == 0) continue;
      if (get<uint64_t>(planes + 8 * (w + nbits - 1)) == 0)
        refuse("the top plane of group " + std::to_string(g) + " is zero while nbits is " + std::to_string(nbits) + " (the form is canonical)");
      const uint64_t idle = ~lane_mask(voxels, k);
      for (uint32_t b = 0; idle && b < nbits; ++b)
        if (get<uint64_t>(planes + 8 * (w + b)) & idle) refuse("a bit is set in a lane beyond the cell's voxels (group " + std::to_string(g) + ")");
      w += nbits;
    }
  }
  c.cells.resize(n_flagged);
  for (uint32_t i = 0; i < n_flagged; ++i) c.cells[i] = CorrectionCellEntry{get<uint32_t>(entries + 8 * (size_t)i), get<uint32_t>(entries + 8 * (size_t)i + 4)};
  c.payload.assign(table, table + payload_bytes);
  return c;
}

std::vector<uint8_t> correction_unpack(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const std::vector<uint8_t>& packed_payload)
{
  std::vector<uint8_t> out(correction_fixed_payload_bytes(h, cells), 0);
  const uint8_t* table = packed_payload.data();
  const uint8_t* planes = table + correction_group_table_bytes(correction_n_groups(h, cells));
  uint64_t g = 0, w = 0, offset = 0;
  for (const CorrectionCellEntry& e : cells) {
    const uint64_t voxels = correction_cell_voxels(h.dims, e.cell), groups = correction_cell_groups(voxels);
    for (uint64_t k = 0; k < groups; ++k, ++g) {
      const uint32_t nbits = table[g];
      if (nbits == 0) continue;   // (the codes are zero already)
      const uint64_t lanes = std::min<uint64_t>(kCorrectionGroup, voxels - kCorrectionGroup * k);
      for (uint64_t l = 0; l < lanes; ++l) {
        uint64_t z = 0;
        for (uint32_t b = 0; b < nbits; ++b) z |= ((get<uint64_t>(planes + 8 * (w + b)) >> l) & 1) << b;
        const uint64_t code = h.kind == kCorrectionVerbatim ? z : (z >> 1) ^ (0 - (z & 1));   // the low `width` bytes are the signed code
        std::memcpy(out.data() + offset + (kCorrectionGroup * k + l) * e.width, &code, e.width);
      }
      w += nbits;
    }
    offset += correction_padded_bytes(voxels, e.width);
  }
  return out;
}

CorrectionPlaneIndex correction_plane_index_of_table(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const uint8_t* table, uint64_t n_groups)
{
  CorrectionPlaneIndex ix;
  ix.cell_group0.reserve(cells.size());
  ix.cell_word0.reserve(cells.size());
  ix.group_word.reserve(n_groups);
  for (const CorrectionCellLayout& c : correction_cell_layout(h, cells)) {
    if (c.group0 + c.groups > n_groups) throw std::runtime_error("the group table is shorter than the cells' groups");
    ix.cell_group0.push_back(c.group0);
    ix.cell_word0.push_back(ix.n_words);
    uint32_t in_cell = 0;   // at most 64 groups of at most 64 planes
    for (uint64_t g = c.group0; g < c.group0 + c.groups; ++g) {
      if (table[g] > kCorrectionGroup) throw std::runtime_error("nbits " + std::to_string(table[g]) + " of group " + std::to_string(g) + " exceeds 64");
      ix.group_word.push_back((uint16_t)in_cell);
      in_cell += table[g];
    }
    ix.n_words += in_cell;
  }
  return ix;
}

CorrectionPlaneIndex correction_plane_index(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const std::vector<uint8_t>& packed_payload)
{
  const uint64_t n_groups = correction_n_groups(h, cells), table_bytes = correction_group_table_bytes(n_groups);
  if (packed_payload.size() < table_bytes) throw std::runtime_error("the packed payload is shorter than its group table");
  CorrectionPlaneIndex ix = correction_plane_index_of_table(h, cells, packed_payload.data(), n_groups);
  if (packed_payload.size() - table_bytes != 8 * ix.n_words) throw std::runtime_error("the packed payload does not have the size its group table gives");
  return ix;
}

}  // namespace vnr
