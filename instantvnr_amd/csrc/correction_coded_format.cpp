// correction_coded_format.cpp — writer, validating reader and host transcoders of a coded correction (correction_coded_format.h).  Host only.
// The header and entry rules are correction_format.cpp's, restated as in correction_packed_format.cpp.
#include "correction_coded_format.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

namespace vnr {

namespace {

const char kMagic[8] = {'V', 'N', 'R', 'C', 'O', 'R', 'C', '1'};

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

[[noreturn]] void refuse(const std::string& what) { throw std::runtime_error("malformed coded correction bytes: " + what); }

// the lanes of group k of a cell that hold a voxel's code, as a mask
uint64_t lane_mask(uint64_t voxels, uint64_t k)
{
  const uint64_t lanes = voxels - kCorrectionGroup * k;
  return lanes >= kCorrectionGroup ? ~0ull : (1ull << lanes) - 1;
}

uint32_t bit_length(uint64_t v) { return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u; }

// one cell's stream, read field by field; a field beyond the cell's words is refused
struct BitReader {
  const uint8_t* words;
  uint64_t n_bits, pos = 0;
  uint64_t take(uint32_t n)   // 1 .. 64 bits
  {
    if (n > n_bits - pos) refuse("a record runs past its cell's words (" + std::to_string(n_bits / 64) + " words)");
    const uint64_t w = pos / 64, o = pos % 64;
    uint64_t v = get<uint64_t>(words + 8 * w) >> o;
    if (o + n > 64) v |= get<uint64_t>(words + 8 * (w + 1)) << (64 - o);   // (o > 0 here)
    pos += n;
    return n == 64 ? v : v & ((1ull << n) - 1);
  }
};

// the streams being written: fields appended at `pos` bits behind word `base`
struct BitWriter {
  std::vector<uint64_t> words;
  uint64_t base = 0, pos = 0;
  void append(uint64_t v, uint32_t n)   // 1 .. 64 bits, v < 2^n
  {
    const uint64_t w = base + pos / 64, o = pos % 64;
    if (w >= words.size()) words.resize(w + 1, 0);
    words[w] |= v << o;
    if (o + n > 64) words.push_back(v >> (64 - o));
    pos += n;
  }
  uint32_t close_cell()   // -> its words; the next field starts the next cell
  {
    const uint64_t n = (pos + 63) / 64;
    base += n;
    pos = 0;
    return (uint32_t)n;
  }
};

// One record -> m of every lane and the mask of the signs; refuses what breaks a rule of the form.  Returns nbits of the group's z.
uint32_t read_group(BitReader& r, uint32_t width, bool verbatim, uint64_t idle, uint64_t m[kCorrectionGroup], uint64_t& signs)
{
  std::fill(m, m + kCorrectionGroup, 0ull);
  signs = 0;
  const uint32_t mbits = (uint32_t)r.take(7);
  if (mbits > 8 * width) refuse("mbits " + std::to_string(mbits) + " exceeds 8 * width (width " + std::to_string(width) + ")");
  uint64_t nonzero = 0;
  for (uint32_t b = mbits; b-- > 0;) {
    uint64_t plane = 0;
    if (r.take(1)) {
      const uint32_t c = (uint32_t)r.take(4);
      if (c > kCodedListMax) refuse("a list count is above 9 (" + std::to_string(c) + ")");
      if (c == 0 && b == mbits - 1) refuse("the top plane is empty while mbits is " + std::to_string(mbits) + " (the form is canonical)");
      int previous = -1;
      for (uint32_t j = 0; j < c; ++j) {
        const int lane = (int)r.take(6);
        if (lane <= previous) refuse("list lanes are not strictly ascending");
        previous = lane;
        plane |= 1ull << lane;
      }
    } else {
      plane = r.take(64);
      if ((uint32_t)__builtin_popcountll(plane) <= kCodedListMax) refuse("a plane is stored dense with 9 or fewer bits set (the form is canonical)");
    }
    if (plane & idle) refuse("a bit is set in a lane beyond the cell's voxels");
    for (uint64_t rest = plane; rest; rest &= rest - 1) m[__builtin_ctzll(rest)] |= 1ull << b;
    nonzero |= plane;
  }
  if (verbatim) return mbits;
  const uint64_t limit = 1ull << (8 * width - 1);   // legal only as the most negative code
  uint64_t z_or = 0;
  for (uint64_t rest = nonzero; rest; rest &= rest - 1) {
    const int lane = __builtin_ctzll(rest);
    const uint64_t s = r.take(1);
    if (m[lane] > limit || (m[lane] == limit && !s)) refuse("a code does not fit the width " + std::to_string(width));
    signs |= s << lane;
    z_or |= 2 * m[lane] - s;
  }
  return bit_length(z_or);
}

void write_group(BitWriter& w, const uint64_t z[kCorrectionGroup], bool verbatim)
{
  uint64_t m[kCorrectionGroup], any = 0, signs = 0;
  for (uint32_t l = 0; l < kCorrectionGroup; ++l) {
    m[l] = verbatim ? z[l] : (z[l] >> 1) + (z[l] & 1);   // |q| of z = (q << 1) ^ (q >> 63)
    if (!verbatim) signs |= (z[l] & 1) << l;
    any |= m[l];
  }
  const uint32_t mbits = bit_length(any);
  w.append(mbits, 7);
  for (uint32_t b = mbits; b-- > 0;) {
    uint64_t plane = 0;
    for (uint32_t l = 0; l < kCorrectionGroup; ++l) plane |= ((m[l] >> b) & 1) << l;
    const uint32_t c = (uint32_t)__builtin_popcountll(plane);
    if (c <= kCodedListMax) {
      w.append(1 | c << 1, 5);
      for (uint64_t rest = plane; rest; rest &= rest - 1) w.append((uint64_t)__builtin_ctzll(rest), 6);
    } else {
      w.append(0, 1);
      w.append(plane, 64);
    }
  }
  if (verbatim) return;
  for (uint32_t l = 0; l < kCorrectionGroup; ++l)
    if (m[l]) w.append((signs >> l) & 1, 1);
}

// table and streams as they are serialised
std::vector<uint8_t> coded_payload(const std::vector<uint32_t>& cell_words, const BitWriter& w)
{
  std::vector<uint8_t> out(correction_coded_table_bytes(cell_words.size()) + 8 * w.words.size(), 0);
  if (!cell_words.empty()) std::memcpy(out.data(), cell_words.data(), 4 * cell_words.size());
  if (!w.words.empty()) std::memcpy(out.data() + correction_coded_table_bytes(cell_words.size()), w.words.data(), 8 * w.words.size());
  return out;
}

}  // namespace

uint32_t correction_coded_record_bits(const uint64_t m[kCorrectionGroup], uint32_t kind)
{
  uint64_t any = 0;
  uint32_t nonzero = 0;
  for (uint32_t l = 0; l < kCorrectionGroup; ++l) {
    any |= m[l];
    nonzero += m[l] != 0;
  }
  uint32_t bits = 7;
  for (uint32_t b = 0; b < bit_length(any); ++b) {
    uint32_t c = 0;
    for (uint32_t l = 0; l < kCorrectionGroup; ++l) c += (uint32_t)((m[l] >> b) & 1);
    bits += c <= kCodedListMax ? 5 + 6 * c : 65;
  }
  return kind == kCorrectionVerbatim ? bits : bits + nonzero;
}

std::vector<uint8_t> correction_coded_write(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const std::vector<uint8_t>& payload)
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

CorrectionCoded correction_coded_parse(const void* bytes, size_t size)
{
  if (!bytes) refuse("null bytes");
  const uint8_t* p = (const uint8_t*)bytes;
  if (size < kCorrectionHeaderBytes) refuse("the size (" + std::to_string(size) + " bytes) is shorter than the header");
  if (std::memcmp(p, kMagic, 8) != 0) refuse("bad magic");
  if (get<uint32_t>(p + 8) != 1) refuse("unsupported version " + std::to_string(get<uint32_t>(p + 8)));
  CorrectionCoded c;
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
  uint64_t previous = 0;
  for (uint32_t i = 0; i < n_flagged; ++i) {
    const uint32_t cell = get<uint32_t>(entries + 8 * (size_t)i), width = get<uint32_t>(entries + 8 * (size_t)i + 4);
    if (cell >= n_cells) refuse("cell " + std::to_string(cell) + " is out of range (" + std::to_string(n_cells) + " cells)");
    if (i > 0 && cell <= previous) refuse("cells must be strictly ascending");
    previous = cell;
    const bool legal = h.kind == kCorrectionVerbatim ? width == ts : (width == 1 || width == 2 || width == 4);
    if (!legal) refuse("illegal code width " + std::to_string(width) + " for kind " + std::to_string(h.kind));
  }
  const uint64_t rest = (uint64_t)(size - kCorrectionHeaderBytes) - 8ull * n_flagged;
  if (rest != payload_bytes) refuse("the size differs from header + entries + payload (" + std::to_string(rest) + " payload bytes present, " + std::to_string(payload_bytes) + " declared)");
  const uint64_t table_bytes = correction_coded_table_bytes(n_flagged);
  if (payload_bytes < table_bytes) refuse("payload_bytes (" + std::to_string(payload_bytes) + ") is shorter than the cell table (" + std::to_string(table_bytes) + " bytes)");

  // the cell table: the padding zero, the streams it announces exactly what is there
  const uint8_t* table = entries + 8 * (size_t)n_flagged;
  uint64_t words = 0;
  for (uint32_t i = 0; i < n_flagged; ++i) words += get<uint32_t>(table + 4 * (size_t)i);   // (at most 2^32 entries below 2^32)
  for (uint64_t at = 4ull * n_flagged; at < table_bytes; ++at)
    if (table[at] != 0) refuse("nonzero cell table padding");
  if ((payload_bytes - table_bytes) % 8 != 0 || (payload_bytes - table_bytes) / 8 != words)
    refuse("payload_bytes (" + std::to_string(payload_bytes) + ") differs from the sum the cell table gives (" + std::to_string(table_bytes) + " + 8 * " + std::to_string(words) + ")");

  // the streams: every record of every cell; the group table of the packed form grows as records prove valid
  const uint8_t* stream = table + table_bytes;
  const bool verbatim = h.kind == kCorrectionVerbatim;
  uint64_t m[kCorrectionGroup], signs;
  for (uint32_t i = 0; i < n_flagged; ++i) {
    const uint32_t cell = get<uint32_t>(entries + 8 * (size_t)i), width = get<uint32_t>(entries + 8 * (size_t)i + 4);
    const uint64_t voxels = correction_cell_voxels(h.dims, cell), groups = correction_cell_groups(voxels);
    const uint64_t cell_words = get<uint32_t>(table + 4 * (size_t)i);
    BitReader r{stream, 64 * cell_words};
    for (uint64_t k = 0; k < groups; ++k) c.group_nbits.push_back((uint8_t)read_group(r, width, verbatim, ~lane_mask(voxels, k), m, signs));
    if ((r.pos + 63) / 64 != cell_words)
      refuse("the table entry of cell " + std::to_string(cell) + " (" + std::to_string(cell_words) + " words) differs from the length its records have (" +
             std::to_string((r.pos + 63) / 64) + " words)");
    if (r.pos % 64 && get<uint64_t>(stream + 8 * (cell_words - 1)) >> (r.pos % 64)) refuse("stream padding is not zero (cell " + std::to_string(cell) + ")");
    stream += 8 * cell_words;
  }
  c.cells.resize(n_flagged);
  for (uint32_t i = 0; i < n_flagged; ++i) c.cells[i] = CorrectionCellEntry{get<uint32_t>(entries + 8 * (size_t)i), get<uint32_t>(entries + 8 * (size_t)i + 4)};
  c.payload.assign(table, table + payload_bytes);
  return c;
}

std::vector<uint8_t> correction_coded_from_packed(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const std::vector<uint8_t>& packed_payload)
{
  const uint64_t table_bytes = correction_group_table_bytes(correction_n_groups(h, cells));
  if (packed_payload.size() < table_bytes) throw std::runtime_error("the packed payload is shorter than its group table");
  const uint8_t* table = packed_payload.data();
  const uint8_t* planes = table + table_bytes;
  const uint64_t n_words = (packed_payload.size() - table_bytes) / 8;
  const bool verbatim = h.kind == kCorrectionVerbatim;
  std::vector<uint32_t> cell_words;
  cell_words.reserve(cells.size());
  BitWriter out;
  uint64_t g = 0, w = 0, z[kCorrectionGroup];
  for (const CorrectionCellEntry& e : cells) {
    const uint64_t groups = correction_cell_groups(correction_cell_voxels(h.dims, e.cell));
    for (uint64_t k = 0; k < groups; ++k, ++g) {
      const uint32_t nbits = table[g];
      if (nbits > kCorrectionGroup || nbits > n_words - w) throw std::runtime_error("the packed payload does not have the size its group table gives");
      std::fill(z, z + kCorrectionGroup, 0ull);
      for (uint32_t b = 0; b < nbits; ++b)
        for (uint64_t rest = get<uint64_t>(planes + 8 * (w + b)); rest; rest &= rest - 1) z[__builtin_ctzll(rest)] |= 1ull << b;
      w += nbits;
      write_group(out, z, verbatim);
    }
    cell_words.push_back(out.close_cell());
  }
  return coded_payload(cell_words, out);
}

std::vector<uint8_t> correction_coded_from_fixed(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const std::vector<uint8_t>& fixed_payload)
{
  if (fixed_payload.size() != correction_fixed_payload_bytes(h, cells)) throw std::runtime_error("the fixed-width payload does not have the size its entries give");
  const bool verbatim = h.kind == kCorrectionVerbatim;
  std::vector<uint32_t> cell_words;
  cell_words.reserve(cells.size());
  BitWriter out;
  uint64_t offset = 0, z[kCorrectionGroup];
  for (const CorrectionCellEntry& e : cells) {
    const uint64_t voxels = correction_cell_voxels(h.dims, e.cell), groups = correction_cell_groups(voxels);
    for (uint64_t k = 0; k < groups; ++k) {
      const uint64_t lanes = std::min<uint64_t>(kCorrectionGroup, voxels - kCorrectionGroup * k);
      std::fill(z, z + kCorrectionGroup, 0ull);
      for (uint64_t l = 0; l < lanes; ++l) {
        uint64_t u = 0;
        std::memcpy(&u, fixed_payload.data() + offset + (kCorrectionGroup * k + l) * e.width, e.width);
        if (verbatim) { z[l] = u; continue; }
        const uint32_t shift = 64 - 8 * e.width;
        const int64_t q = (int64_t)(u << shift) >> shift;   // sign-extended
        z[l] = ((uint64_t)q << 1) ^ (uint64_t)(q >> 63);
      }
      write_group(out, z, verbatim);
    }
    cell_words.push_back(out.close_cell());
    offset += correction_padded_bytes(voxels, e.width);
  }
  return coded_payload(cell_words, out);
}

std::vector<uint8_t> correction_coded_to_packed(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const std::vector<uint8_t>& coded,
                                                const std::vector<uint8_t>& group_nbits)
{
  const uint64_t n_groups = correction_n_groups(h, cells), table_bytes = correction_group_table_bytes(n_groups);
  if (group_nbits.size() != n_groups) throw std::runtime_error("the group table does not have a byte for every group");
  uint64_t n_words = 0;
  for (uint8_t nbits : group_nbits) n_words += nbits;
  std::vector<uint8_t> out(table_bytes + 8 * n_words, 0);
  if (n_groups) std::memcpy(out.data(), group_nbits.data(), n_groups);
  const uint64_t coded_table = correction_coded_table_bytes(cells.size());
  if (coded.size() < coded_table) throw std::runtime_error("the coded payload is shorter than its cell table");
  const uint8_t* stream = coded.data() + coded_table;
  const bool verbatim = h.kind == kCorrectionVerbatim;
  uint64_t g = 0, w = 0, m[kCorrectionGroup], signs;
  for (size_t i = 0; i < cells.size(); ++i) {
    const uint64_t voxels = correction_cell_voxels(h.dims, cells[i].cell), groups = correction_cell_groups(voxels);
    const uint64_t cell_words = get<uint32_t>(coded.data() + 4 * i);
    if (cell_words > (uint64_t)(coded.data() + coded.size() - stream) / 8) throw std::runtime_error("the coded payload does not have the size its cell table gives");
    BitReader r{stream, 64 * cell_words};
    for (uint64_t k = 0; k < groups; ++k, ++g) {
      const uint32_t nbits = read_group(r, cells[i].width, verbatim, ~lane_mask(voxels, k), m, signs);
      if (nbits != group_nbits[g]) throw std::runtime_error("the group table differs from the records");
      for (uint32_t l = 0; l < kCorrectionGroup; ++l) {
        const uint64_t z = verbatim ? m[l] : 2 * m[l] - ((signs >> l) & 1);
        for (uint32_t b = 0; b < nbits; ++b) {
          uint64_t word = get<uint64_t>(out.data() + table_bytes + 8 * (w + b));
          word |= ((z >> b) & 1) << l;
          std::memcpy(out.data() + table_bytes + 8 * (w + b), &word, 8);
        }
      }
      w += nbits;
    }
    stream += 8 * cell_words;
  }
  return out;
}

}  // namespace vnr
