// correction_pack.hip — the packed form of an error-bound correction on the device (correction_packed_format.h defines the bytes,
// include/vnr_amd.h "packed corrections" the interface): pack from the resident fixed-width payload, unpack into it.
//
// A group is 64 consecutive codes of a flagged cell, and a wavefront of gfx950 is 64 lanes: one wave takes one group, lane l its code l.
// The group's nbits is the bit length of the OR of the lanes' z, plane b is one 64-bit __ballot of bit b, and lane b keeps plane b, so
// that the nbits words of a group leave as one coalesced 8-byte store per lane.  A block is one wave and walks the (at most 64) groups
// of one flagged cell, which makes the offsets simple: lane g holds nbits of group g, a wave scan gives the group's first word inside
// the cell, and the cells' first words are the prefix sum of n_flagged small integers, taken on the host between the two pack kernels
// (the codes never leave the device; tests/correction_pack_ref.py restates the format in numpy and is matched byte for byte).
// Every offset is 64-bit.  The unpack runs the same walk backwards into a zeroed payload; the apply of correction.hip reads that.
// The two launches at the end take what they work on as arguments: when they run and where the result is kept is correction_store.hip's.
#include "correction_wave.h"

namespace vnr {

namespace {

// a flagged cell in both forms
struct PackCell {
  uint64_t codes;    // byte offset of its codes in the fixed-width payload (a multiple of 16)
  uint64_t group0;   // its first group in the group table
  uint32_t voxels, width;
};

// code i of a cell as the unsigned z of the packed form: the zigzag of the sign-extended code, or (verbatim) the bit pattern
__device__ __forceinline__ uint64_t load_z(const uint8_t* __restrict__ codes, uint32_t width, uint32_t i, bool verbatim)
{
  int64_t q;
  uint64_t u;
  if (width == 1) { const int8_t v = reinterpret_cast<const int8_t*>(codes)[i]; q = v; u = (uint8_t)v; }
  else if (width == 2) { const int16_t v = reinterpret_cast<const int16_t*>(codes)[i]; q = v; u = (uint16_t)v; }
  else if (width == 4) { const int32_t v = reinterpret_cast<const int32_t*>(codes)[i]; q = v; u = (uint32_t)v; }
  else { u = reinterpret_cast<const uint64_t*>(codes)[i]; q = (int64_t)u; }
  return verbatim ? u : (((uint64_t)q << 1) ^ (uint64_t)(q >> 63));
}

__device__ __forceinline__ void store_z(uint8_t* __restrict__ codes, uint32_t width, uint32_t i, uint64_t z, bool verbatim)
{
  const uint64_t code = verbatim ? z : ((z >> 1) ^ (0 - (z & 1)));   // its low `width` bytes are the signed code
  if (width == 1) codes[i] = (uint8_t)code;
  else if (width == 2) reinterpret_cast<uint16_t*>(codes)[i] = (uint16_t)code;
  else if (width == 4) reinterpret_cast<uint32_t*>(codes)[i] = (uint32_t)code;
  else reinterpret_cast<uint64_t*>(codes)[i] = code;
}

// pack, pass 1: nbits of every group into the table, the plane words of every cell
__global__ void __launch_bounds__(kWave) correction_pack_measure_kernel(const uint8_t* __restrict__ payload, const PackCell* __restrict__ cells, uint32_t n_cells,
                                                                        bool verbatim, uint8_t* __restrict__ table, uint32_t* __restrict__ cell_words)
{
  const uint32_t lane = threadIdx.x;
  for (uint64_t c = blockIdx.x; c < n_cells; c += gridDim.x) {
    const PackCell pc = cells[c];
    const uint32_t groups = (pc.voxels + kWave - 1) / kWave;
    uint32_t nbits = 0;   // lane g: of group g
    for (uint32_t g = 0; g < groups; ++g) {
      const uint32_t i = g * kWave + lane;
      const uint64_t any = wave_or(i < pc.voxels ? load_z(payload + pc.codes, pc.width, i, verbatim) : 0);
      if (lane == g) nbits = any ? 64u - (uint32_t)__clzll((long long)any) : 0u;
    }
    if (lane < groups) table[pc.group0 + lane] = (uint8_t)nbits;
    uint32_t total = nbits;
    for (int off = kWave / 2; off > 0; off >>= 1) total += __shfl_xor(total, off, kWave);
    if (lane == 0) cell_words[c] = total;   // at most 64 * 64
  }
}

// pack, pass 2: the planes
__global__ void __launch_bounds__(kWave) correction_pack_planes_kernel(const uint8_t* __restrict__ payload, const PackCell* __restrict__ cells,
                                                                       const uint64_t* __restrict__ cell_word0, uint32_t n_cells, bool verbatim,
                                                                       const uint8_t* __restrict__ table, uint64_t* __restrict__ planes)
{
  const uint32_t lane = threadIdx.x;
  for (uint64_t c = blockIdx.x; c < n_cells; c += gridDim.x) {
    const PackCell pc = cells[c];
    const uint32_t groups = (pc.voxels + kWave - 1) / kWave;
    const uint32_t nbits = lane < groups ? table[pc.group0 + lane] : 0u;
    const uint32_t first = wave_exclusive_scan(nbits, lane);
    uint64_t* __restrict__ out = planes + cell_word0[c];
    for (uint32_t g = 0; g < groups; ++g) {
      const uint32_t nb = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(nbits, (int)g, kWave));
      if (nb == 0) continue;
      const uint32_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(first, (int)g, kWave));
      const uint32_t i = g * kWave + lane;
      const uint64_t z = i < pc.voxels ? load_z(payload + pc.codes, pc.width, i, verbatim) : 0;
      uint64_t keep = 0;
      for (uint32_t b = 0; b < nb; ++b) {
        const uint64_t plane = __ballot((int)((z >> b) & 1));
        if (lane == b) keep = plane;
      }
      if (lane < nb) out[at + lane] = keep;
    }
  }
}

// unpack: table and planes as they were serialised -> the fixed-width payload (zeroed before: groups of nbits 0, lanes without a
// voxel and the cells' padding are not written)
__global__ void __launch_bounds__(kWave) correction_unpack_kernel(const uint8_t* __restrict__ table, const uint64_t* __restrict__ planes, const PackCell* __restrict__ cells,
                                                                  const uint64_t* __restrict__ cell_word0, uint32_t n_cells, bool verbatim,
                                                                  uint8_t* __restrict__ payload)
{
  const uint32_t lane = threadIdx.x;
  for (uint64_t c = blockIdx.x; c < n_cells; c += gridDim.x) {
    const PackCell pc = cells[c];
    const uint32_t groups = (pc.voxels + kWave - 1) / kWave;
    const uint32_t nbits = lane < groups ? table[pc.group0 + lane] : 0u;
    const uint32_t first = wave_exclusive_scan(nbits, lane);
    const uint64_t* __restrict__ in = planes + cell_word0[c];
    for (uint32_t g = 0; g < groups; ++g) {
      const uint32_t nb = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(nbits, (int)g, kWave));
      if (nb == 0) continue;
      const uint32_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(first, (int)g, kWave));
      const uint64_t word = lane < nb ? in[at + lane] : 0;   // lane b: plane b
      uint64_t z = 0;
      for (uint32_t b = 0; b < nb; ++b) {
        const uint64_t plane = (uint64_t)__shfl((unsigned long long)word, (int)b, kWave);
        z |= ((plane >> lane) & 1) << b;
      }
      const uint32_t i = g * kWave + lane;
      if (i < pc.voxels) store_z(payload + pc.codes, pc.width, i, z, verbatim);
    }
  }
}

DeviceBuffer<PackCell> upload_pack_cells(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, hipStream_t stream)
{
  const std::vector<CorrectionCellLayout> layout = correction_cell_layout(h, cells);
  std::vector<PackCell> host(cells.size());
  for (size_t i = 0; i < host.size(); ++i) host[i] = PackCell{layout[i].codes, layout[i].group0, layout[i].voxels, cells[i].width};
  DeviceBuffer<PackCell> d_cells(MemTag::Network);
  d_cells.upload(host.data(), host.size(), stream);
  VNR_HIP_CHECK(hipStreamSynchronize(stream));   // `host` goes out of scope
  return d_cells;
}

}  // namespace

void correction_unpack_on_device(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const uint8_t* table, const uint8_t* d_packed,
                                 uint64_t packed_bytes, uint8_t* d_payload, hipStream_t stream)
{
  const uint64_t n_groups = correction_n_groups(h, cells), table_bytes = correction_group_table_bytes(n_groups);
  // the cells' first plane words, from the table (validated when the bytes were read)
  const CorrectionPlaneIndex ix = correction_plane_index_of_table(h, cells, table, n_groups);
  if (packed_bytes != table_bytes + 8 * ix.n_words) throw std::runtime_error("the packed payload does not have the size its group table gives");
  const DeviceBuffer<PackCell> d_cells = upload_pack_cells(h, cells, stream);
  DeviceBuffer<uint64_t> d_word0(MemTag::Network);
  d_word0.upload(ix.cell_word0.data(), ix.cell_word0.size(), stream);
  VNR_HIP_CHECK(hipMemsetAsync(d_payload, 0, correction_fixed_payload_bytes(h, cells), stream));
  correction_unpack_kernel<<<cell_blocks(cells.size()), kWave, 0, stream>>>(d_packed, reinterpret_cast<const uint64_t*>(d_packed + table_bytes), d_cells.ptr, d_word0.ptr,
                                                                             (uint32_t)cells.size(), h.kind == kCorrectionVerbatim, d_payload);
  VNR_HIP_CHECK(hipGetLastError());
  VNR_HIP_CHECK(hipStreamSynchronize(stream));   // the index and the scratch go out of scope
}

std::vector<uint8_t> correction_pack_on_device(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const uint8_t* d_payload, hipStream_t stream)
{
  const uint32_t n = (uint32_t)cells.size();
  const uint64_t table_bytes = correction_group_table_bytes(correction_n_groups(h, cells));
  const bool verbatim = h.kind == kCorrectionVerbatim;
  const DeviceBuffer<PackCell> d_cells = upload_pack_cells(h, cells, stream);
  DeviceBuffer<uint8_t> d_table(MemTag::Network);
  DeviceBuffer<uint32_t> d_cell_words(MemTag::Network);
  d_table.resize(table_bytes);
  d_table.zero(stream);   // (its padding)
  d_cell_words.resize(n);
  correction_pack_measure_kernel<<<cell_blocks(n), kWave, 0, stream>>>(d_payload, d_cells.ptr, n, verbatim, d_table.ptr, d_cell_words.ptr);
  VNR_HIP_CHECK(hipGetLastError());
  // the cells' first words: n_flagged small integers through the host
  std::vector<uint32_t> cell_words(n);
  d_cell_words.download(cell_words.data(), n, stream);   // (synchronises)
  std::vector<uint64_t> word0(n);
  uint64_t words = 0;
  for (uint32_t i = 0; i < n; ++i) { word0[i] = words; words += cell_words[i]; }
  std::vector<uint8_t> packed(table_bytes + 8 * words);
  DeviceBuffer<uint64_t> d_word0(MemTag::Network), d_planes(MemTag::Network);
  d_word0.upload(word0.data(), n, stream);
  if (words) {
    d_planes.resize(words);
    correction_pack_planes_kernel<<<cell_blocks(n), kWave, 0, stream>>>(d_payload, d_cells.ptr, d_word0.ptr, n, verbatim, d_table.ptr, d_planes.ptr);
    VNR_HIP_CHECK(hipGetLastError());
    VNR_HIP_CHECK(hipMemcpyAsync(packed.data() + table_bytes, d_planes.ptr, 8 * words, hipMemcpyDeviceToHost, stream));
  }
  d_table.download(packed.data(), table_bytes, stream);   // (synchronises)
  return packed;
}

}  // namespace vnr
