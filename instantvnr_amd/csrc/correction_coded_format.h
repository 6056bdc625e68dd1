// correction_coded_format.h — the coded serialised form of an error-bound correction (include/vnr_amd.h, "coded corrections"):
// validating reader, writer and the host transcoders to and from the packed payload.  Host only, no HIP include: tests build it, with
// correction_packed_format.cpp and correction_format.cpp, with the host compiler under sanitizers.
//
// Little-endian.  The header of correction_format.h with magic "VNRCORC1", version 1 and payload_bytes the size of the coded payload;
// the same n_flagged entries {uint32 cell, uint32 width}; then the coded payload:
//   1. the cell table: one u32 per flagged cell in entry order, the 64-bit words of that cell's stream; zero bytes up to a multiple of 8;
//   2. the cell streams, in entry order.
// A stream is a run of u64 words; stream bit i is bit i % 64 of word i / 64; a field of n bits is appended least significant bit
// first; every cell's stream starts on a word and is filled up with zero bits to a whole word.  A cell's stream is the records of its
// groups in order (the packed form's groups: 64 consecutive codes, the last group filled with codes of 0).
// Group record, kinds 0 and 1, with m_l = |q_l| (0 .. 2^31) and s_l = (q_l < 0) of the sign-extended code q_l of lane l:
//   1. mbits, 7 bits: the bit length of the largest m_l; 0 ends the record;
//   2. for b = mbits - 1 down to 0, with P the lanes whose m_l has bit b and c = |P|:
//        c <= 9: one bit 1, c in 4 bits, the lanes of P ascending in 6 bits each (5 + 6 c bits against 65: 9 is the largest that pays);
//        else:   one bit 0, then 64 bits, bit l set for l in P;
//   3. for every lane with m_l != 0, ascending: one bit s_l.
// Kind 2 (verbatim patterns): m_l is the stored bit pattern, mbits 0 .. 64, and there is no step 3.
// The form is canonical: what correction_coded_parse accepts, correction_coded_write gives back byte for byte.
#pragma once

#include "correction_packed_format.h"

namespace vnr {

constexpr uint32_t kCodedListMax = 9;   // the largest count of a plane that is stored as a list of lanes
// the longest cell stream: 64 groups of 64-bit verbatim patterns with every plane dense, 64 * (7 + 64 * 65) bits
constexpr uint32_t kCodedMaxCellWords = 7 + 64 * 65;

struct CorrectionCoded {
  CorrectionHeader h;
  std::vector<CorrectionCellEntry> cells;   // strictly ascending; width is the fixed-width form's
  std::vector<uint8_t> payload;             // cell table and streams
  std::vector<uint8_t> group_nbits;         // by-product of the walk: the packed form's group table (nbits of z), without its padding
};

inline uint64_t correction_coded_table_bytes(uint64_t n_flagged) { return (4 * n_flagged + 7) / 8 * 8; }

// The bits of a group's record in closed form, from the magnitudes m_l of its 64 lanes (kind 2: the patterns; lanes beyond the cell's
// voxels 0) and the kind: 7, then 5 + 6 c or 65 for each plane below the bit length of the largest m_l by its count c, then (kinds 0
// and 1) a bit per m_l != 0.  A cell's stream is ceil(the sum over its groups / 64) words.  This is what the rate pass of
// correction.hip and the encoder of correction_code.hip count on the device; nothing on the device calls it, it is here to be held
// to what the writer below really writes.
uint32_t correction_coded_record_bits(const uint64_t m[kCorrectionGroup], uint32_t kind);

std::vector<uint8_t> correction_coded_write(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const std::vector<uint8_t>& payload);
// throws std::runtime_error("malformed coded correction bytes: <rule>"); everything is validated before anything is allocated by the
// bytes' say
CorrectionCoded correction_coded_parse(const void* bytes, size_t size);

// the coded payload of a packed payload that correction_packed_parse accepted or the device pack made, and of a fixed-width payload
std::vector<uint8_t> correction_coded_from_packed(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const std::vector<uint8_t>& packed_payload);
std::vector<uint8_t> correction_coded_from_fixed(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const std::vector<uint8_t>& fixed_payload);
// the packed payload of a coded payload that correction_coded_parse accepted (group_nbits is that parse's)
std::vector<uint8_t> correction_coded_to_packed(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const std::vector<uint8_t>& coded_payload,
                                                const std::vector<uint8_t>& group_nbits);

}  // namespace vnr
