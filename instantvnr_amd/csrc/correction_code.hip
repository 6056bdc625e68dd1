// correction_code.hip — the coded form of an error-bound correction on the device (correction_coded_format.h defines the bytes,
// include/vnr_amd.h "coded corrections" the interface): encode from whichever form is resident, decode into the packed resident form.
//
// A group is 64 codes and a wavefront of gfx950 is 64 lanes: one wave takes one group, lane l its code l.  A plane of the magnitudes is
// one 64-bit __ballot, its count one popcount, and with the counts the length of a record is known in closed form before a bit of it
// is written.  Encode, pass 1: a block of one wave walks the (at most 64) groups of a flagged cell, lane g keeps the bits of record g,
// their sum is the cell's words.  The cells' words are scanned on the device (guided_sampler.hip).  Pass 2: the same walk; a wave scan
// gives every record its first bit, the cell's stream is assembled in LDS (fields are OR-ed into zeroed words: a lane of a list writes
// its own 6 bits at its rank among the set lanes) and leaves as whole 8-byte words, one coalesced store a lane.  No global atomics.
// The LDS holds the longest legal stream, 64 groups of 64 dense 64-bit planes = 4 167 words, so there is one code path.
// Decode: a wave stages its cell's stream in LDS and walks the records in order (all lanes read the same field, a broadcast), each
// lane collects its own magnitude and sign, and the planes of z leave by ballot exactly as correction_pack.hip writes them, at the
// places the host parse's group table gives.  Every offset is 64-bit.  tests/correction_coded_ref.py restates the format in numpy.
// The encoder and the decode launch at the end take what they work on as arguments: when they run is correction_store.hip's.
#include "correction_wave.h"

#include <cstring>

namespace vnr {

namespace {

constexpr uint32_t kStageWords = kCodedMaxCellWords;

// a flagged cell to be encoded
struct CodeCell {
  uint64_t src;      // fixed-width source: byte offset of its codes in the payload; planes: its cell index in the grid
  uint32_t group0;   // its first group
  uint32_t voxels, width;
};

// where the codes are resident: `codes` (the fixed-width payload) or, if that is null, the planes and their index
struct CodeSource {
  const uint8_t* codes;
  const Correction::PlaneCell* plane_cells;
  const uint32_t* plane_groups;
  const uint64_t* planes;
};

// a flagged cell to be decoded
struct DecodeCell {
  uint64_t stream0, word0;   // its first stream word; its first plane word
  uint32_t stream_words, group0, voxels, width;
};

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask, uint32_t lane) { return (uint32_t)__popcll(mask & ((1ull << lane) - 1)); }

// the z of the packed form (correction_pack.hip) of lane `lane` of group g of a cell, from either resident form
__device__ __forceinline__ uint64_t load_z(const CodeSource& s, const CodeCell& c, uint64_t word0, uint32_t g, uint32_t lane, bool verbatim)
{
  if (s.codes) {
    const uint32_t i = g * kWave + lane;
    if (i >= c.voxels) return 0;
    const uint8_t* __restrict__ codes = s.codes + c.src;
    int64_t q;
    uint64_t u;
    if (c.width == 1) { const int8_t v = reinterpret_cast<const int8_t*>(codes)[i]; q = v; u = (uint8_t)v; }
    else if (c.width == 2) { const int16_t v = reinterpret_cast<const int16_t*>(codes)[i]; q = v; u = (uint16_t)v; }
    else if (c.width == 4) { const int32_t v = reinterpret_cast<const int32_t*>(codes)[i]; q = v; u = (uint32_t)v; }
    else { u = reinterpret_cast<const uint64_t*>(codes)[i]; q = (int64_t)u; }
    return verbatim ? u : (((uint64_t)q << 1) ^ (uint64_t)(q >> 63));
  }
  const uint32_t e = s.plane_groups[c.group0 + g], nb = e >> 16, at = e & 0xffffu;
  const uint64_t word = lane < nb ? s.planes[word0 + at + lane] : 0;   // lane b: plane b
  uint64_t z = 0;
  for (uint32_t b = 0; b < nb; ++b) {
    const uint64_t plane = (uint64_t)__shfl((unsigned long long)word, (int)b, kWave);
    z |= ((plane >> lane) & 1) << b;
  }
  return z;
}

// the magnitude the coded form stores for z: |q| of the zigzag, or (verbatim) the pattern itself
__device__ __forceinline__ uint64_t magnitude(uint64_t z, bool verbatim) { return verbatim ? z : (z >> 1) + (z & 1); }

__device__ __forceinline__ uint32_t bit_length(uint64_t v) { return v ? 64u - (uint32_t)__clzll((long long)v) : 0u; }

// encode, pass 1: the bits of every record, the words of every cell
__global__ void __launch_bounds__(kWave) correction_code_measure_kernel(CodeSource s, const CodeCell* __restrict__ cells, uint32_t n_cells, bool verbatim,
                                                                        uint32_t* __restrict__ group_bits, uint32_t* __restrict__ cell_words, uint64_t* __restrict__ cell_end)
{
  const uint32_t lane = threadIdx.x;
  for (uint64_t c = blockIdx.x; c < n_cells; c += gridDim.x) {
    const CodeCell cc = cells[c];
    const uint32_t groups = (cc.voxels + kWave - 1) / kWave;
    const uint64_t word0 = s.codes ? 0 : s.plane_cells[cc.src].word0;
    uint32_t mine = 0;   // lane g: the bits of record g
    for (uint32_t g = 0; g < groups; ++g) {
      const uint64_t m = magnitude(load_z(s, cc, word0, g, lane, verbatim), verbatim);
      const uint32_t mbits = bit_length(wave_or(m));
      uint32_t bits = 7;
      for (uint32_t b = 0; b < mbits; ++b) {
        const uint32_t count = (uint32_t)__popcll(__ballot((int)((m >> b) & 1)));
        bits += count <= kCodedListMax ? 5 + 6 * count : 65;
      }
      if (!verbatim) bits += (uint32_t)__popcll(__ballot(m != 0));
      if (lane == g) mine = bits;
    }
    if (lane < groups) group_bits[cc.group0 + lane] = mine;
    uint32_t total = mine;
    for (int off = kWave / 2; off > 0; off >>= 1) total += __shfl_xor(total, off, kWave);
    if (lane == 0) {
      cell_words[c] = (total + 63) / 64;   // at most kCodedMaxCellWords
      cell_end[c] = (total + 63) / 64;     // (scanned next)
    }
  }
}

// n bits (at most 32, v < 2^n) OR-ed into the zeroed stage at stream bit `pos`
__device__ __forceinline__ void stage_put(uint32_t* stage, uint32_t limit, uint32_t pos, uint32_t v, uint32_t n)
{
  const uint32_t w = pos >> 5, o = pos & 31;
  if (w < limit) atomicOr(&stage[w], v << o);
  if (o + n > 32 && w + 1 < limit) atomicOr(&stage[w + 1], v >> (32 - o));   // (o > 0 here)
}

// encode, pass 2: the streams.  cell_end is the inclusive scan of the cells' words.
__global__ void __launch_bounds__(kWave) correction_code_write_kernel(CodeSource s, const CodeCell* __restrict__ cells, uint32_t n_cells, bool verbatim,
                                                                      const uint32_t* __restrict__ group_bits, const uint64_t* __restrict__ cell_end,
                                                                      uint64_t* __restrict__ out)
{
  __shared__ uint32_t stage[2 * kStageWords];
  const uint32_t lane = threadIdx.x;
  for (uint64_t c = blockIdx.x; c < n_cells; c += gridDim.x) {
    const CodeCell cc = cells[c];
    const uint32_t groups = (cc.voxels + kWave - 1) / kWave;
    const uint64_t word0 = s.codes ? 0 : s.plane_cells[cc.src].word0;
    const uint64_t end = cell_end[c], first = c ? cell_end[c - 1] : 0;
    const uint32_t words = (uint32_t)min((uint64_t)kStageWords, end - first), limit = 2 * words;
    for (uint32_t i = lane; i < limit; i += kWave) stage[i] = 0;
    __syncthreads();
    const uint32_t start = wave_exclusive_scan(lane < groups ? group_bits[cc.group0 + lane] : 0u, lane);
    for (uint32_t g = 0; g < groups; ++g) {
      uint32_t pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(start, (int)g, kWave));
      const uint64_t z = load_z(s, cc, word0, g, lane, verbatim);
      const uint64_t m = magnitude(z, verbatim);
      const uint32_t mbits = bit_length(wave_or(m));
      if (lane == 0) stage_put(stage, limit, pos, mbits, 7);
      pos += 7;
      for (uint32_t b = mbits; b-- > 0;) {
        const uint64_t plane = __ballot((int)((m >> b) & 1));
        const uint32_t count = (uint32_t)__popcll(plane);
        if (count <= kCodedListMax) {
          if (lane == 0) stage_put(stage, limit, pos, 1u | count << 1, 5);
          if ((plane >> lane) & 1) stage_put(stage, limit, pos + 5 + 6 * lanes_below(plane, lane), lane, 6);
          pos += 5 + 6 * count;
        } else {   // one bit 0, then the plane
          if (lane == 0) stage_put(stage, limit, pos + 1, (uint32_t)plane, 32);
          if (lane == 1) stage_put(stage, limit, pos + 33, (uint32_t)(plane >> 32), 32);
          pos += 65;
        }
      }
      if (!verbatim) {
        const uint64_t nonzero = __ballot(m != 0);
        if (m != 0 && (z & 1)) stage_put(stage, limit, pos + lanes_below(nonzero, lane), 1u, 1);
      }
    }
    __syncthreads();
    for (uint32_t i = lane; i < words; i += kWave) out[first + i] = (uint64_t)stage[2 * i] | (uint64_t)stage[2 * i + 1] << 32;
    __syncthreads();   // the next cell zeroes the stage
  }
}

// n bits (1 .. 64) of the staged stream at bit `pos`; beyond the cell's words (the host reader has refused such bytes) zeros
__device__ __forceinline__ uint64_t stage_take(const uint64_t* stage, uint32_t words, uint32_t pos, uint32_t n)
{
  if (pos + n > 64 * words) return 0;
  const uint32_t w = pos >> 6, o = pos & 63;
  uint64_t v = stage[w] >> o;
  if (o + n > 64) v |= stage[w + 1] << (64 - o);   // (o > 0 here)
  return n == 64 ? v : v & ((1ull << n) - 1);
}

// decode: the streams as they were serialised -> the planes of z, group after group at the places the index gives
__global__ void __launch_bounds__(kWave) correction_code_decode_kernel(const uint64_t* __restrict__ streams, const DecodeCell* __restrict__ cells, uint32_t n_cells,
                                                                       bool verbatim, const uint32_t* __restrict__ plane_groups, uint64_t* __restrict__ planes)
{
  __shared__ uint64_t stage[kStageWords];
  const uint32_t lane = threadIdx.x;
  for (uint64_t c = blockIdx.x; c < n_cells; c += gridDim.x) {
    const DecodeCell dc = cells[c];
    const uint32_t groups = (dc.voxels + kWave - 1) / kWave;
    const uint32_t words = min(dc.stream_words, kStageWords);
    for (uint32_t i = lane; i < words; i += kWave) stage[i] = streams[dc.stream0 + i];
    __syncthreads();
    uint32_t pos = 0;
    for (uint32_t g = 0; g < groups; ++g) {
      const uint32_t e = plane_groups[dc.group0 + g], nb = min(e >> 16, (uint32_t)kWave), at = e & 0xffffu;
      const uint32_t mbits = min((uint32_t)stage_take(stage, words, pos, 7), (uint32_t)kWave);
      pos += 7;
      uint64_t m = 0;
      for (uint32_t b = mbits; b-- > 0;) {
        if (stage_take(stage, words, pos, 1)) {
          const uint32_t count = (uint32_t)stage_take(stage, words, pos + 1, 4);
          for (uint32_t j = 0; j < count; ++j)
            if (stage_take(stage, words, pos + 5 + 6 * j, 6) == lane) m |= 1ull << b;
          pos += 5 + 6 * count;
        } else {
          m |= ((stage_take(stage, words, pos + 1, 64) >> lane) & 1) << b;
          pos += 65;
        }
      }
      uint64_t z = m;
      if (!verbatim) {
        const uint64_t nonzero = __ballot(m != 0);
        const uint64_t sign = m != 0 ? stage_take(stage, words, pos + lanes_below(nonzero, lane), 1) : 0;
        pos += (uint32_t)__popcll(nonzero);
        z = 2 * m - sign;   // the zigzag of +-m
      }
      uint64_t keep = 0;
      for (uint32_t b = 0; b < nb; ++b) {
        const uint64_t plane = __ballot((int)((z >> b) & 1));
        if (lane == b) keep = plane;
      }
      if (lane < nb) planes[dc.word0 + at + lane] = keep;
    }
    __syncthreads();   // the next cell overwrites the stage
  }
}

}  // namespace

void CorrectionEncoder::measure(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& entries, hipStream_t stream)
{
  n = (uint32_t)entries.size();
  verbatim = h.kind == kCorrectionVerbatim;
  const std::vector<CorrectionCellLayout> layout = correction_cell_layout(h, entries);
  const uint64_t n_groups = n ? layout.back().group0 + layout.back().groups : 0;
  if (n_groups > 0xffffffffull) throw std::runtime_error("the correction has more than 2^32 groups");
  std::vector<CodeCell> host(n);
  for (uint32_t i = 0; i < n; ++i) host[i] = CodeCell{d_codes ? layout[i].codes : (uint64_t)entries[i].cell, (uint32_t)layout[i].group0, layout[i].voxels, entries[i].width};
  cells.upload(reinterpret_cast<const uint8_t*>(host.data()), n * sizeof(CodeCell), stream);
  group_bits.resize(n_groups);
  cell_words.resize(n);
  cell_end.resize(n);
  correction_code_measure_kernel<<<cell_blocks(n), kWave, 0, stream>>>(CodeSource{d_codes, d_plane_cells, d_plane_groups, d_planes}, reinterpret_cast<const CodeCell*>(cells.ptr), n,
                                                                       verbatim, group_bits.ptr, cell_words.ptr, cell_end.ptr);
  VNR_HIP_CHECK(hipGetLastError());
  device_inclusive_scan(cell_end.ptr, n, scan_scratch, stream);
  VNR_HIP_CHECK(hipMemcpyAsync(&words, cell_end.ptr + (n - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, stream));   // one count crosses to the host
  VNR_HIP_CHECK(hipStreamSynchronize(stream));   // (`host` goes out of scope, too)
  if (words > (uint64_t)n * kCodedMaxCellWords) throw std::runtime_error("internal error: the coded streams are longer than the format allows");
}

void CorrectionEncoder::write(uint8_t* d_out, hipStream_t stream)
{
  const uint64_t table_bytes = correction_coded_table_bytes(n);
  VNR_HIP_CHECK(hipMemcpyAsync(d_out, cell_words.ptr, 4ull * n, hipMemcpyDeviceToDevice, stream));
  if (table_bytes > 4ull * n) VNR_HIP_CHECK(hipMemsetAsync(d_out + 4ull * n, 0, table_bytes - 4ull * n, stream));
  if (!words) return;
  correction_code_write_kernel<<<cell_blocks(n), kWave, 0, stream>>>(CodeSource{d_codes, d_plane_cells, d_plane_groups, d_planes}, reinterpret_cast<const CodeCell*>(cells.ptr), n,
                                                                     verbatim, group_bits.ptr, cell_end.ptr, reinterpret_cast<uint64_t*>(d_out + table_bytes));
  VNR_HIP_CHECK(hipGetLastError());
}

void correction_decode_on_device(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const std::vector<uint8_t>& coded_payload,
                                 const CorrectionPlaneIndex& ix, const uint32_t* d_plane_groups, uint64_t* d_planes, hipStream_t stream)
{
  const uint32_t n = (uint32_t)cells.size();
  const uint64_t coded_table = correction_coded_table_bytes(n);
  if (ix.group_word.size() > 0xffffffffull || ix.cell_word0.size() != n || coded_payload.size() < coded_table)
    throw std::runtime_error("internal error: a coded correction without the group table of its parse");
  // the cells' places in both payloads
  const std::vector<CorrectionCellLayout> layout = correction_cell_layout(h, cells);
  std::vector<DecodeCell> host(n);
  uint64_t stream0 = 0;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t stream_words;
    std::memcpy(&stream_words, coded_payload.data() + 4ull * i, 4);
    host[i] = DecodeCell{stream0, ix.cell_word0[i], stream_words, (uint32_t)ix.cell_group0[i], layout[i].voxels, cells[i].width};
    stream0 += stream_words;
  }
  if (coded_payload.size() != coded_table + 8 * stream0) throw std::runtime_error("internal error: the coded payload does not have the size its cell table gives");
  DeviceBuffer<uint8_t> d_coded(MemTag::Network);
  DeviceBuffer<DecodeCell> d_cells(MemTag::Network);
  d_coded.upload(coded_payload.data(), coded_payload.size(), stream);   // as it is (hipMalloc aligns it; the streams start at a multiple of 8)
  d_cells.upload(host.data(), n, stream);
  if (ix.n_words) {
    correction_code_decode_kernel<<<cell_blocks(n), kWave, 0, stream>>>(reinterpret_cast<const uint64_t*>(d_coded.ptr + coded_table), d_cells.ptr, n,
                                                                         h.kind == kCorrectionVerbatim, d_plane_groups, d_planes);
    VNR_HIP_CHECK(hipGetLastError());
  }
  VNR_HIP_CHECK(hipStreamSynchronize(stream));   // the stream has drained: the host vector and the coded copy are released
}

}  // namespace vnr
