// correction_packed_format.h — the packed serialised form of an error-bound correction (include/vnr_amd.h, "packed corrections"):
// validating reader, writer and the host unpack.  Host only, no HIP include: tests build it, with correction_format.cpp, with the
// host compiler under sanitizers.
//
// Little-endian.  The header of correction_format.h with magic "VNRCORP1", version 1 and payload_bytes the size of the packed payload;
// the same n_flagged entries {uint32 cell, uint32 width}; then the packed payload.  The codes of a flagged cell (its fixed-width codes
// in their order, lx + cx * (ly + cy * lz)) are cut into groups of 64 consecutive codes, the last group of a cell filled up with codes
// of value 0: ceil(voxels / 64) groups a cell, at most 64.  A code becomes an unsigned z: kinds 0 and 1 z = (q << 1) ^ (q >> 63) of the
// sign-extended code, kind 2 the stored bit pattern.  nbits of a group is the bit length of its largest z.  The payload is
//   1. the group table: one byte nbits per group, all groups of all flagged cells in cell order, zero bytes up to a multiple of 8;
//   2. the planes: group after group, nbits words of u64; bit l of word b is bit b of the z of the group's code l.
#pragma once

#include "correction_format.h"

namespace vnr {

constexpr uint32_t kCorrectionGroup = 64;   // codes of a group: one wavefront (correction_pack.hip)

struct CorrectionPacked {
  CorrectionHeader h;
  std::vector<CorrectionCellEntry> cells;   // strictly ascending; width is the fixed-width form's
  std::vector<uint8_t> payload;             // group table and planes
};

inline uint64_t correction_cell_groups(uint64_t voxels) { return (voxels + kCorrectionGroup - 1) / kCorrectionGroup; }
// groups of all flagged cells
uint64_t correction_n_groups(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells);
inline uint64_t correction_group_table_bytes(uint64_t n_groups) { return (n_groups + 7) / 8 * 8; }
// the payload size of the fixed-width form: the sum of the padded cell sizes
uint64_t correction_fixed_payload_bytes(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells);

// Where a flagged cell lies in the fixed-width payload and in the group table: the one walk over the entries that every form's
// offsets start from (the entries must be ones a reader accepted or a build made)
struct CorrectionCellLayout {
  uint64_t codes;    // byte offset of its codes in the fixed-width payload (a multiple of 16)
  uint64_t group0;   // its first group in the group table
  uint32_t voxels, groups;
};
std::vector<CorrectionCellLayout> correction_cell_layout(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells);

std::vector<uint8_t> correction_packed_write(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const std::vector<uint8_t>& payload);
// throws std::runtime_error("malformed packed correction bytes: <rule>"); everything is validated before anything is allocated by the
// bytes' say.  What it accepts, correction_packed_write gives back byte for byte.
CorrectionPacked correction_packed_parse(const void* bytes, size_t size);
// the fixed-width payload (correction_format.h) of a packed payload that correction_packed_parse accepted; the cells' padding is zero
std::vector<uint8_t> correction_unpack(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const std::vector<uint8_t>& packed_payload);

// Where a code lies in the planes, for a reader that starts at a voxel (the apply that reads the planes, correction.hip): code li of
// flagged cell i is lane li % 64 of group cell_group0[i] + li / 64, whose nbits plane words start at word
// cell_word0[i] + group_word[that group] of the planes.
struct CorrectionPlaneIndex {
  std::vector<uint64_t> cell_group0, cell_word0;   // per flagged cell: the groups and the plane words in front of it
  std::vector<uint16_t> group_word;                // per group: the plane words of its cell in front of it, at most 63 * 64
  uint64_t n_words = 0;                            // plane words in all
};
// from a group table alone (one byte nbits per group, without padding: a packed payload's first bytes, or the coded parse's
// by-product); throws if n_groups is less than the entries' or an nbits exceeds 64
CorrectionPlaneIndex correction_plane_index_of_table(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const uint8_t* table, uint64_t n_groups);
// of a packed payload that correction_packed_parse accepted or the device pack made; throws if the payload's size is not the one its
// group table gives
CorrectionPlaneIndex correction_plane_index(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const std::vector<uint8_t>& packed_payload);

}  // namespace vnr
