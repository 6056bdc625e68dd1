// correction_record.h — an error-bound correction (vnrAmdCorrection of include/vnr_amd.h) as ONE record of what is held where, the conversions
// of it (correction_store.hip, which states every route) and the device work they launch (correction_pack.hip, correction_code.hip).
#pragma once

#include "common.h"
#include "correction_coded_format.h"

namespace vnr {

// how it came to be; never changes.  Asked only where a route depends on it and not on what is held (correction_store.hip)
enum class CorrectionOrigin { Built, BuiltDirect, FixedBytes, PackedBytes, CodedBytes };
enum class CorrectionForm { Fixed = 0, Packed = 1, Coded = 2 };   // VNR_AMD_CORRECTION_FORM_*

struct CorrectionTableEntry { uint64_t offset; uint32_t width, pad; };   // per macrocell: byte offset of its codes in the payload, or ~0

// Header and entries are validated facts, and with them the size of every payload.  A payload is held whole or not at all: on the
// host a vector that is not empty, on the device a buffer that is allocated (a conversion assigns it once its content is complete);
// every payload of a correction with a flagged cell has at least one byte.  A correction without a flagged cell holds every form,
// all of them empty, and nothing on the device.  The predicates below are the only code that looks.
struct Correction {
  explicit Correction(CorrectionOrigin o) : origin(o) {}
  const CorrectionOrigin origin;
  CorrectionData data;   // data.payload: the fixed-width payload
  uint64_t n_voxels_flagged = 0, n_nan = 0;   // the report of the build that made it (unknown to a correction read from bytes)
  double max_abs_before = 0.0;
  int worst_after[3] = {-1, -1, -1};
  // group table and planes; cell table and streams; the coded parse's by-product, the packed form's nbits of every group
  std::vector<uint8_t> packed_payload, coded_payload, group_table;
  // The resident form (vnrAmdCorrectionSetResidentForm): what the apply reads on the device.  0, fixed: d_table and d_payload.
  // 1, packed: d_packed, the packed payload as it is serialised, and the index of correction_plane_index, {first plane word, first
  // group} for every cell of the grid and {first word inside the cell, nbits} for every group.
  int resident_form = 0;
  struct PlaneCell { uint64_t word0; uint32_t group0, pad; };   // word0 = ~0: the cell is not flagged
  DeviceBuffer<uint8_t> d_payload{MemTag::Network}, d_packed{MemTag::Network};
  DeviceBuffer<CorrectionTableEntry> d_table{MemTag::Network};
  DeviceBuffer<PlaneCell> d_plane_cells{MemTag::Network};
  DeviceBuffer<uint32_t> d_plane_groups{MemTag::Network};   // word | nbits << 16

  bool empty() const { return data.cells.empty(); }
  bool host_fixed() const { return empty() || !data.payload.empty(); }
  bool host_packed() const { return empty() || !packed_payload.empty(); }
  bool host_coded() const { return empty() || !coded_payload.empty(); }
  // the packed form's group table, as the head of the packed payload or from the coded parse
  const uint8_t* host_group_table() const { return !packed_payload.empty() ? packed_payload.data() : (!group_table.empty() ? group_table.data() : nullptr); }
  bool device_payload() const { return d_payload.ptr != nullptr; }                  // the fixed-width payload, with or without its table
  bool device_fixed() const { return device_payload() && d_table.ptr != nullptr; }   // what the apply of form 0 reads
  bool device_planes() const { return d_packed.ptr != nullptr; }                    // what the apply of form 1 reads, index included
  bool on_device() const { return device_payload() || device_planes(); }
  const uint64_t* d_planes() const { return reinterpret_cast<const uint64_t*>(d_packed.ptr + correction_group_table_bytes(d_plane_groups.count)); }
};

// ---- correction_store.hip: the requests.  Each has synchronised on return; none touches a device for an empty correction.
// per-cell {offset, width} of every cell of the grid from the flagged ones, in payload order: what d_table holds
std::vector<CorrectionTableEntry> correction_make_table(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells);
// a payload on the host, cached in the record
const std::vector<uint8_t>& correction_fixed_payload(Correction& corr, hipStream_t stream);
const std::vector<uint8_t>& correction_packed_payload(Correction& corr, hipStream_t stream);
const std::vector<uint8_t>& correction_coded_payload(Correction& corr, hipStream_t stream);
// vnrAmdCorrectionSerialize / SerializePacked / SerializeCoded: header, entries and that payload
std::vector<uint8_t> correction_serialize(Correction& corr, CorrectionForm form, hipStream_t stream);
// what the apply of resident form `form` reads made resident, and what only the other form reads released once the stream has drained
void correction_make_resident(Correction& corr, int form, hipStream_t stream);
// vnrAmdCorrectionSetResidentForm: a correction that holds nothing on the device only notes the form, any other is converted at once
void correction_set_resident_form(Correction& corr, int form, hipStream_t stream);
// vnrAmdCorrectionSerializePackedToDevice / SerializeCodedToDevice: those bytes into device memory, the payload device to device or
// encoded straight into the destination where it is resident.  d_bytes null: only *size.
void correction_serialize_to_device(Correction& corr, CorrectionForm form, void* d_bytes, size_t capacity, size_t* size, hipStream_t consumer);
// whether answering a serialisation request runs anything on a device (an entry point initialises one only then)
bool correction_needs_device(const Correction& corr, CorrectionForm form, bool to_device_memory);

// ---- correction_pack.hip, correction_code.hip: the launches.  They know nothing of a correction's state; all but write() have synchronised.
// the packed payload of the fixed-width payload at d_payload: two kernels, n_flagged small integers through the host
std::vector<uint8_t> correction_pack_on_device(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const uint8_t* d_payload, hipStream_t stream);
// d_packed (packed_bytes of table and planes; `table`: the same table on the host) unpacked into d_payload (correction_fixed_payload_bytes)
void correction_unpack_on_device(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const uint8_t* table, const uint8_t* d_packed,
                                 uint64_t packed_bytes, uint8_t* d_payload, hipStream_t stream);
// The device encode in two steps, so that the size is known before the destination is: measure (pass 1 and the scan of the cells'
// words), then write (pass 2: table, padding and streams at d_out, 8-byte aligned, payload_bytes() of room; enqueued only).
struct CorrectionEncoder {
  const uint8_t* d_codes;   // the source: the fixed-width payload or, if this is null, the planes and their index
  const Correction::PlaneCell* d_plane_cells;
  const uint32_t* d_plane_groups;
  const uint64_t* d_planes;
  void measure(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& entries, hipStream_t stream);
  uint64_t payload_bytes() const { return correction_coded_table_bytes(n) + 8 * words; }
  void write(uint8_t* d_out, hipStream_t stream);
  // what both passes share; lives as long as the kernels run
  bool verbatim = false;
  uint32_t n = 0;
  uint64_t words = 0;        // of all streams, after measure()
  DeviceBuffer<uint8_t> cells{MemTag::Network};   // the kernels' view of the flagged cells
  DeviceBuffer<uint32_t> group_bits{MemTag::Network}, cell_words{MemTag::Network};
  DeviceBuffer<uint64_t> cell_end{MemTag::Network}, scan_scratch{MemTag::Network};
};
// the streams of a coded payload that correction_coded_parse accepted, uploaded as they are and decoded by one kernel into the planes
// at d_planes, at the places `ix` (of that parse's group table) and its device form d_plane_groups give
void correction_decode_on_device(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells, const std::vector<uint8_t>& coded_payload,
                                 const CorrectionPlaneIndex& ix, const uint32_t* d_plane_groups, uint64_t* d_planes, hipStream_t stream);

}  // namespace vnr
