// correction_store.hip — every conversion between what a correction holds (correction_record.h): the ONE place where routes are decided.
// No kernel is here: the device work is launched through correction_pack.hip and correction_code.hip, which know nothing of that state.
//
// Host: hF, hP, hC the fixed-width, packed and coded payload, hT the coded parse's group table.  Device: dF the fixed-width payload
// (with its table T: what the apply of form FIXED reads), dP the planes with their index (form PACKED).  A correction without a
// flagged cell holds every form, empty: all requests are answered from header and entries, none touches the device (a ...ToDevice
// with a destination copies the header there).  Request, starting state, what is done:
// host fixed (Serialize)         hF held: as it is.  Built direct without hP: "host packed" first (downloads dP).  Coded bytes without
//                                hP: hC transcoded to hP on the host -- also while dP is resident, where "host packed" downloads dP
//                                instead; both are kept as they were.  Then hP unpacked on the host; cached.
// host packed (SerializePacked)  hP held: as it is.  Coded bytes: dP resident: downloaded; else hC transcoded on the host.  Built
//                                direct: dP downloaded.  Built, fixed bytes: "device fixed", then the device pack of dF.  Cached.
// host coded (SerializeCoded)    hC held: as it is.  Nothing on the device: transcoded on the host from hP if held, else from hF.  dP
//                                resident: encoded on the device from the planes; else from dF.  Cached.
// device fixed (dF; the apply    dF resident: nothing.  Built or fixed bytes without dP: hF uploaded.  dP resident: unpacked on the
// of form FIXED adds T)          device from dP, with the table of hP if held, else hT (coded bytes decoded on the device), else "host
//                                packed" first (built direct).  Else (packed bytes, coded bytes, built direct): "host packed" uploaded
//                                to scratch and unpacked on the device -- packed bytes do so even when hF has been unpacked on the host.
//                                T: from the entries, uploaded.  Then dP and its index are released.
// device planes (the apply of    dP resident: nothing.  Else "host packed", uploaded as it is, the index from its table.  Then dF and
// form PACKED)                   T are released.
// before either apply            coded bytes without hP and with nothing on the device: hC uploaded and decoded on the device into dP,
//                                the index from hT (form FIXED then unpacks dP as above)
// packed bytes to device         size: hP's if held, else dP's; neither: "host packed" first.  Form PACKED without dP: "device planes"
//                                first.  dP resident: device to device; else hP, host to device.
// coded bytes to device          hC held, or nothing on the device: "host coded", host to device.  Else encoded on the device straight
//                                into the destination (through scratch if that is off the 8-byte grid); not cached.
// SetResidentForm                nothing on the device: the form is noted, the first apply brings it.  Else converted at once.
#include "box_walk.h"
#include "correction_record.h"

#include <cstring>

namespace vnr {

std::vector<CorrectionTableEntry> correction_make_table(const CorrectionHeader& h, const std::vector<CorrectionCellEntry>& cells)
{
  std::vector<CorrectionTableEntry> t(correction_n_cells(h.dims), CorrectionTableEntry{~0ull, 0, 0});
  const std::vector<CorrectionCellLayout> layout = correction_cell_layout(h, cells);
  for (size_t i = 0; i < cells.size(); ++i) t[cells[i].cell] = CorrectionTableEntry{layout[i].codes, cells[i].width, 0};
  return t;
}

namespace {

bool holds_coded_alone(const Correction& c) { return c.origin == CorrectionOrigin::CodedBytes && !c.host_packed(); }   // hC and hT alone on the host
void transcode_coded_on_host(Correction& c) { if (holds_coded_alone(c)) c.packed_payload = correction_coded_to_packed(c.data.h, c.data.cells, c.coded_payload, c.group_table); }

void download_planes(Correction& c, hipStream_t stream)
{
  if (!c.device_planes()) throw std::runtime_error("internal error: a direct correction holds its planes neither on the host nor on the device");
  std::vector<uint8_t> packed(c.d_packed.count);
  c.d_packed.download(packed.data(), packed.size(), stream);   // (synchronises)
  c.packed_payload = std::move(packed);
}

// the device form of the index: {first plane word, first group} for every cell of the grid, word | nbits << 16 for every group
void upload_plane_index(Correction& c, const CorrectionPlaneIndex& ix, const uint8_t* table, hipStream_t stream)
{
  if (ix.group_word.size() > 0xffffffffull) throw std::runtime_error("the correction has more than 2^32 groups");
  std::vector<Correction::PlaneCell> cells(correction_n_cells(c.data.h.dims), Correction::PlaneCell{~0ull, 0, 0});
  for (size_t i = 0; i < c.data.cells.size(); ++i) cells[c.data.cells[i].cell] = Correction::PlaneCell{ix.cell_word0[i], (uint32_t)ix.cell_group0[i], 0};
  std::vector<uint32_t> groups(ix.group_word.size());
  for (size_t g = 0; g < groups.size(); ++g) groups[g] = (uint32_t)ix.group_word[g] | (uint32_t)table[g] << 16;
  c.d_plane_cells.upload(cells.data(), cells.size(), stream);
  c.d_plane_groups.upload(groups.data(), groups.size(), stream);
  VNR_HIP_CHECK(hipStreamSynchronize(stream));   // the host vectors go out of scope
}

// the first use on the device of a correction read from coded bytes: hC -> dP and its index
void decode_coded_on_device(Correction& c, hipStream_t stream)
{
  const CorrectionData& d = c.data;
  const uint64_t n_groups = c.group_table.size(), table_bytes = correction_group_table_bytes(n_groups);
  if (n_groups != correction_n_groups(d.h, d.cells)) throw std::runtime_error("internal error: a coded correction without the group table of its parse");
  const CorrectionPlaneIndex ix = correction_plane_index_of_table(d.h, d.cells, c.group_table.data(), n_groups);
  upload_plane_index(c, ix, c.group_table.data(), stream);
  DeviceBuffer<uint8_t> d_packed(MemTag::Network);
  d_packed.resize(table_bytes + 8 * ix.n_words);
  VNR_HIP_CHECK(hipMemsetAsync(d_packed.ptr, 0, table_bytes, stream));   // (the table's padding)
  VNR_HIP_CHECK(hipMemcpyAsync(d_packed.ptr, c.group_table.data(), n_groups, hipMemcpyHostToDevice, stream));
  correction_decode_on_device(d.h, d.cells, c.coded_payload, ix, c.d_plane_groups.ptr, reinterpret_cast<uint64_t*>(d_packed.ptr + table_bytes), stream);
  c.d_packed = std::move(d_packed);
}

// "device fixed" without T: what the device pack and encode read, too
void ensure_device_payload(Correction& c, hipStream_t stream)
{
  if (c.device_payload() || c.empty()) return;
  const CorrectionData& d = c.data;
  DeviceBuffer<uint8_t> d_payload(MemTag::Network), scratch(MemTag::Network);
  if ((c.origin == CorrectionOrigin::Built || c.origin == CorrectionOrigin::FixedBytes) && !c.device_planes()) {
    d_payload.upload(d.payload.data(), d.payload.size(), stream);
    VNR_HIP_CHECK(hipStreamSynchronize(stream));
  } else {
    if (!(c.device_planes() && c.host_group_table())) correction_packed_payload(c, stream);
    // as it is (hipMalloc aligns it; the planes start at a multiple of 8), unless the planes are resident already
    if (!c.device_planes()) scratch.upload(c.packed_payload.data(), c.packed_payload.size(), stream);
    const DeviceBuffer<uint8_t>& packed = c.device_planes() ? c.d_packed : scratch;
    d_payload.resize(correction_fixed_payload_bytes(d.h, d.cells));
    correction_unpack_on_device(d.h, d.cells, c.host_group_table(), packed.ptr, packed.count, d_payload.ptr, stream);
  }
  c.d_payload = std::move(d_payload);
}

// the device encode from whichever form is resident
CorrectionEncoder resident_encoder(const Correction& c)
{
  return CorrectionEncoder{c.device_planes() ? nullptr : c.d_payload.ptr, c.d_plane_cells.ptr, c.d_plane_groups.ptr, c.device_planes() ? c.d_planes() : nullptr};
}

}  // namespace

const std::vector<uint8_t>& correction_fixed_payload(Correction& c, hipStream_t stream)
{
  if (c.host_fixed()) return c.data.payload;
  if (c.origin == CorrectionOrigin::BuiltDirect) correction_packed_payload(c, stream);
  transcode_coded_on_host(c);
  if (!c.host_packed()) throw std::runtime_error("internal error: the correction holds its codes neither on the host nor on the device");
  c.data.payload = correction_unpack(c.data.h, c.data.cells, c.packed_payload);
  return c.data.payload;
}

const std::vector<uint8_t>& correction_packed_payload(Correction& c, hipStream_t stream)
{
  if (c.host_packed()) return c.packed_payload;
  if (c.origin == CorrectionOrigin::CodedBytes && !c.device_planes()) {
    transcode_coded_on_host(c);
  } else if (c.origin == CorrectionOrigin::CodedBytes || c.origin == CorrectionOrigin::BuiltDirect) {
    download_planes(c, stream);
  } else {
    ensure_device_payload(c, stream);
    c.packed_payload = correction_pack_on_device(c.data.h, c.data.cells, c.d_payload.ptr, stream);
  }
  return c.packed_payload;
}

const std::vector<uint8_t>& correction_coded_payload(Correction& c, hipStream_t stream)
{
  if (c.host_coded()) return c.coded_payload;
  const CorrectionData& d = c.data;
  if (!c.on_device()) {
    if (c.host_packed()) c.coded_payload = correction_coded_from_packed(d.h, d.cells, c.packed_payload);
    else if (c.host_fixed()) c.coded_payload = correction_coded_from_fixed(d.h, d.cells, d.payload);
    else throw std::runtime_error("internal error: the correction holds its codes neither on the host nor on the device");
    return c.coded_payload;
  }
  CorrectionEncoder enc = resident_encoder(c);
  enc.measure(d.h, d.cells, stream);
  DeviceBuffer<uint8_t> d_out(MemTag::Network);
  d_out.resize(enc.payload_bytes());
  enc.write(d_out.ptr, stream);
  std::vector<uint8_t> coded(enc.payload_bytes());
  d_out.download(coded.data(), coded.size(), stream);   // (synchronises)
  c.coded_payload = std::move(coded);
  return c.coded_payload;
}

std::vector<uint8_t> correction_serialize(Correction& c, CorrectionForm form, hipStream_t stream)
{
  if (form == CorrectionForm::Packed) return correction_packed_write(c.data.h, c.data.cells, correction_packed_payload(c, stream));
  if (form == CorrectionForm::Coded) return correction_coded_write(c.data.h, c.data.cells, correction_coded_payload(c, stream));
  correction_fixed_payload(c, stream);
  return correction_write(c.data);
}

void correction_make_resident(Correction& c, int form, hipStream_t stream)
{
  if (c.empty()) return;
  const CorrectionData& d = c.data;
  if (holds_coded_alone(c) && !c.on_device()) decode_coded_on_device(c, stream);
  if (form == 0) {
    if (!c.device_fixed()) {
      ensure_device_payload(c, stream);
      const std::vector<CorrectionTableEntry> table = correction_make_table(d.h, d.cells);
      DeviceBuffer<CorrectionTableEntry> d_table(MemTag::Network);
      d_table.upload(table.data(), table.size(), stream);
      VNR_HIP_CHECK(hipStreamSynchronize(stream));   // `table` goes out of scope
      c.d_table = std::move(d_table);
    }
    if (c.device_planes()) {
      VNR_HIP_CHECK(hipStreamSynchronize(stream));   // no apply still reads the planes
      c.d_packed.release(); c.d_plane_cells.release(); c.d_plane_groups.release();
    }
    return;
  }
  if (!c.device_planes()) {
    const std::vector<uint8_t>& packed = correction_packed_payload(c, stream);   // (the device pack, once, of a correction that has no packed form yet)
    upload_plane_index(c, correction_plane_index(d.h, d.cells, packed), packed.data(), stream);
    DeviceBuffer<uint8_t> d_packed(MemTag::Network);
    d_packed.upload(packed.data(), packed.size(), stream);   // as it is (hipMalloc aligns it; the planes start at a multiple of 8)
    VNR_HIP_CHECK(hipStreamSynchronize(stream));
    c.d_packed = std::move(d_packed);
  }
  if (c.device_payload()) {
    VNR_HIP_CHECK(hipStreamSynchronize(stream));   // no apply or pack still reads the fixed-width payload
    c.d_payload.release(); c.d_table.release();
  }
}

void correction_set_resident_form(Correction& c, int form, hipStream_t stream)
{
  if (form != 0 && form != 1) throw std::runtime_error("unknown resident form " + std::to_string(form) + " (0: fixed-width, 1: packed)");
  if (form != c.resident_form && c.on_device()) correction_make_resident(c, form, stream);   // nothing on the device yet: the first apply brings this form
  c.resident_form = form;
}

bool correction_needs_device(const Correction& c, CorrectionForm form, bool to_device_memory)
{
  if (to_device_memory) return true;
  if (form == CorrectionForm::Packed) return !c.host_packed() && !(holds_coded_alone(c) && !c.device_planes());
  if (form == CorrectionForm::Coded) return !c.host_coded() && c.on_device();
  return !c.host_fixed() && !c.host_packed() && c.origin == CorrectionOrigin::BuiltDirect;
}

void correction_serialize_to_device(Correction& c, CorrectionForm form, void* d_bytes, size_t capacity, size_t* size, hipStream_t consumer)
{
  if (!size) throw std::runtime_error("null result");
  const CorrectionData& d = c.data;
  const bool coded = form == CorrectionForm::Coded;
  hipStream_t stream = Runtime::get().stream;
  CorrectionEncoder enc = resident_encoder(c);
  const bool encode = coded && !c.host_coded() && c.on_device();   // else: the host copy, transcoded there if need be
  uint64_t payload_bytes;
  if (encode) {
    enc.measure(d.h, d.cells, stream);
    payload_bytes = enc.payload_bytes();
  } else if (coded) {
    payload_bytes = correction_coded_payload(c, stream).size();
  } else {   // the host copy's if there is one (the device pack's is cached as by SerializePacked), else the resident planes'
    if (!c.device_planes()) correction_packed_payload(c, stream);
    payload_bytes = c.host_packed() ? c.packed_payload.size() : c.d_packed.bytes();
  }
  std::vector<uint8_t> head = coded ? correction_coded_write(d.h, d.cells, std::vector<uint8_t>()) : correction_packed_write(d.h, d.cells, std::vector<uint8_t>());
  std::memcpy(head.data() + 80, &payload_bytes, sizeof(uint64_t));   // payload_bytes of the header (correction_format.h)
  *size = head.size() + payload_bytes;
  if (!d_bytes) return;
  if (capacity < *size)
    throw std::runtime_error("capacity (" + std::to_string(capacity) + " bytes) is smaller than the " + (coded ? "coded" : "packed") + " correction (" +
                             std::to_string(*size) + " bytes)");
  require_room(d_bytes, *size, coded ? "the coded bytes" : "the packed bytes");
  if (!coded && payload_bytes && !c.device_planes() && c.resident_form == 1) correction_make_resident(c, 1, stream);   // PACKED: the planes, then device to device
  EventGuard ev;
  wait_for(consumer, stream, ev);   // what the destination held may still be being read
  uint8_t* d_payload = (uint8_t*)d_bytes + head.size();
  DeviceBuffer<uint8_t> aligned(MemTag::Network);   // the encode stores whole words: a destination off the 8-byte grid is reached by a copy
  VNR_HIP_CHECK(hipMemcpyAsync(d_bytes, head.data(), head.size(), hipMemcpyHostToDevice, stream));
  if (encode) {
    if ((uintptr_t)d_payload % 8 == 0) {
      enc.write(d_payload, stream);
    } else {
      aligned.resize(payload_bytes);
      enc.write(aligned.ptr, stream);
      VNR_HIP_CHECK(hipMemcpyAsync(d_payload, aligned.ptr, payload_bytes, hipMemcpyDeviceToDevice, stream));
    }
  } else if (payload_bytes) {
    if (!coded && c.device_planes()) VNR_HIP_CHECK(hipMemcpyAsync(d_payload, c.d_packed.ptr, payload_bytes, hipMemcpyDeviceToDevice, stream));
    else VNR_HIP_CHECK(hipMemcpyAsync(d_payload, (coded ? c.coded_payload : c.packed_payload).data(), payload_bytes, hipMemcpyHostToDevice, stream));
  }
  VNR_HIP_CHECK(hipStreamSynchronize(stream));   // on return the bytes are there; `head` and the encoder go out of scope
}

}  // namespace vnr
