// capi.cpp — C-ABI of libvnr_amd (include/vnr_amd.h): opaque handles over the C++ objects, error codes
// + last-error string instead of the reference's exceptions (api.cpp).
#include "../../include/vnr_amd.h"

#include <cstdlib>
#include <cstdio>
#include <fstream>
#include <limits>
#include <memory>

#include "correction_budget.h"
#include "correction_record.h"
#include "dist.h"
#include "renderer.h"
#include "scene.h"

using namespace vnr;

struct vnrAmdVolume_t { std::shared_ptr<VolumeBase> v; };
struct vnrAmdRenderer_t { std::unique_ptr<Renderer> r; std::shared_ptr<VolumeBase> volume; };
struct vnrAmdTransferFunction_t { TransferFunctionData d; };
struct vnrAmdCamera_t { CameraData d; };
struct vnrAmdCorrection_t { std::shared_ptr<Correction> c; };

namespace {
thread_local std::string g_last_error;

template <typename F>
int guarded(F&& f)
{
  try {
    f();
    return VNR_AMD_OK;
  } catch (const std::exception& e) {
    g_last_error = e.what();
  } catch (...) {
    g_last_error = "unknown error";
  }
  return VNR_AMD_ERROR;
}

template <typename T, typename F>
T* guarded_new(F&& f)
{
  T* out = nullptr;
  guarded([&]() { out = f(); });
  return out;
}

Json parse_json_arg(const void* data, size_t size, int format)
{
  if (!data) throw std::runtime_error("null JSON argument");
  switch (format) {
  case VNR_AMD_JSON_TEXT: return Json::parse_text((const char*)data, size);
  case VNR_AMD_JSON_BSON: return Json::from_bson((const uint8_t*)data, size);
  case VNR_AMD_JSON_TEXT_FILE: return Json::load_text_file(std::string((const char*)data, size ? strnlen((const char*)data, size) : strlen((const char*)data)));
  case VNR_AMD_JSON_BSON_FILE: return Json::load_bson_file(std::string((const char*)data, size ? strnlen((const char*)data, size) : strlen((const char*)data)));
  default: throw std::runtime_error("unknown JSON format");
  }
}

// api.cpp:180-185: a config that is a JSON string is a path to a JSON text file
Json resolve_config(const Json& j) { return j.is_string() ? Json::load_text_file(j.as_string()) : j; }
// api.cpp:269-278: params that are a JSON string are a path to a BSON file
Json resolve_params(const Json& j) { return j.is_string() ? Json::load_bson_file(j.as_string()) : j; }

NeuralVolume* as_neural(vnrAmdVolume v)
{
  if (!v || !v->v) throw std::runtime_error("null volume");
  if (!v->v->is_network()) throw std::runtime_error("expecting a neural volume");  // api.cpp:137-139
  return static_cast<NeuralVolume*>(v->v.get());
}
SimpleVolume* as_simple(vnrAmdVolume v)
{
  if (!v || !v->v) throw std::runtime_error("null volume");
  if (v->v->is_network()) throw std::runtime_error("expecting a simple volume");  // api.cpp:128-130
  return static_cast<SimpleVolume*>(v->v.get());
}
Correction* as_correction(vnrAmdCorrection c)
{
  if (!c || !c->c) throw std::runtime_error("null correction");
  return c->c.get();
}
void* dup_bytes(const void* p, size_t n)
{
  void* out = std::malloc(n ? n : 1);
  if (!out) throw std::runtime_error("out of host memory");
  if (n) std::memcpy(out, p, n);
  return out;
}

// vnrAmdCorrectionSerialize*, to the host and into device memory; a device is asked for only where the route runs on one
int serialize_correction(vnrAmdCorrection c, CorrectionForm form, void** bytes, size_t* size)
{
  return guarded([&]() {
    Correction* k = as_correction(c);
    if (!bytes || !size) throw std::runtime_error("null result");
    if (correction_needs_device(*k, form, false) && !Runtime::get().ready()) Runtime::get().init(-1);
    const std::vector<uint8_t> b = correction_serialize(*k, form, Runtime::get().stream);
    *bytes = dup_bytes(b.data(), b.size());
    *size = b.size();
  });
}
int serialize_correction_to_device(vnrAmdCorrection c, CorrectionForm form, void* d_bytes, size_t capacity, size_t* size, void* stream)
{
  return guarded([&]() {
    Correction* k = as_correction(c);
    if (!size) throw std::runtime_error("null result");
    if (correction_needs_device(*k, form, d_bytes != nullptr) && !Runtime::get().ready()) Runtime::get().init(-1);
    correction_serialize_to_device(*k, form, d_bytes, capacity, size, (hipStream_t)stream);
  });
}
// the tail of vnrAmdCreateCorrectionFrom*Bytes: what only a build knows is unknown (worst_after = -1, -1, -1 and the counts 0 likewise)
vnrAmdCorrection_t* read_correction(std::shared_ptr<Correction> k, CorrectionHeader h, std::vector<CorrectionCellEntry> cells)
{
  k->data.h = h;
  k->data.cells = std::move(cells);
  k->max_abs_before = std::numeric_limits<double>::quiet_NaN();
  return new vnrAmdCorrection_t{std::move(k)};
}
// vnrAmdNeuralVolumeBuildCorrectionWithinBytes / CodedWithinBytes after their own refusals: the search over rate passes, the build at its tolerance,
// and what was promised is what was built.  FIXED, PACKED: the two-call build (the device pack stays cached); CODED: the direct build, encoded once.
vnrAmdCorrection_t* build_within_bytes(vnrAmdVolume v, const DeviceSource& ref, float range_lo, float range_hi, uint64_t max_bytes, CorrectionForm form,
                                       double eps_hi, int rounds, vnrAmdCorrectionBudget* report)
{
  correction_budget_check(eps_hi, rounds);
  NeuralVolume* n = as_neural(v);
  const bool coded = form == CorrectionForm::Coded, packed = form == CorrectionForm::Packed;
  const CorrectionBudgetResult r = correction_budget_search(
      [&](const double* eps, int n_eps, uint64_t* bytes, int* refused) {
        CorrectionRateCoded rates[kCorrectionBudgetLadder];
        CorrectionRate plain[kCorrectionBudgetLadder];
        if (coded) n->correction_rates_coded(ref, range_lo, range_hi, eps, n_eps, rates);
        else n->correction_rates(ref, range_lo, range_hi, eps, n_eps, plain);
        for (int k = 0; k < n_eps; ++k) {
          const CorrectionRate& rate = coded ? rates[k].rate : plain[k];
          bytes[k] = coded ? rates[k].coded_serialized_bytes : (packed ? rate.packed_serialized_bytes : rate.serialized_bytes);
          refused[k] = rate.refused;
        }
      },
      max_bytes, eps_hi, rounds);
  std::shared_ptr<Correction> corr = coded ? n->build_correction_packed(ref, range_lo, range_hi, r.eps) : n->build_correction(ref, range_lo, range_hi, r.eps);
  hipStream_t s = Runtime::get().stream;
  const uint64_t built = kCorrectionHeaderBytes + 8 * corr->data.cells.size() +
                         (coded ? correction_coded_payload(*corr, s) : (packed ? correction_packed_payload(*corr, s) : correction_fixed_payload(*corr, s))).size();
  if (built != r.bytes) {
    char e[40];
    std::snprintf(e, sizeof(e), "%.17g", r.eps);
    throw std::runtime_error(std::string("internal error: the correction built at eps ") + e + " has " + std::to_string(built) + " serialised bytes" +
                             (coded ? " in the coded form" : "") + ", the rate pass gave " + std::to_string(r.bytes));
  }
  *report = vnrAmdCorrectionBudget{r.eps, r.bytes, r.eps_tighter, r.bytes_tighter, r.rate_passes};
  return new vnrAmdCorrection_t{std::move(corr)};
}
}  // namespace

// ------------------------------------------------------------------------------------------------ runtime
Runtime& Runtime::get()
{
  static Runtime r;
  return r;
}

void Runtime::init(int dev)
{
  if (ready() && (dev < 0 || dev == device)) return;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) throw std::runtime_error("[vnr] no HIP capable devices found!");
  if (dev < 0) {
    dev = 0;
    if (const char* e = std::getenv("VNR_AMD_DEVICE")) dev = std::atoi(e);
    else if (const char* e2 = std::getenv("VNR_CUDA_DEVICE")) dev = std::atoi(e2);  // renderer.cpp:300
  }
  if (dev >= count) throw std::runtime_error("[vnr] device index out of range");
  // Moving to another device destroys the library's streams (the ray parts' pool included, whose handles live renderers hold) and strands
  // every buffer on the old device: only an empty library may move.  A rank binds its device first: vnrAmdDistInit* before
  // any volume or renderer.
  if (ready() && dev != device && bytes_renderer + bytes_network > 0)
    throw std::runtime_error("[vnr] the library runs on device " + std::to_string(device) + " and holds " + std::to_string(bytes_renderer + bytes_network) +
                             " bytes there: release every volume and renderer before moving it to device " + std::to_string(dev));
  VNR_HIP_CHECK(hipSetDevice(dev));
  hipDeviceProp_t prop;
  VNR_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
  n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (stream) (void)hipStreamDestroy(stream);
  for (hipStream_t& ps : part_streams) if (ps) { (void)hipStreamDestroy(ps); ps = nullptr; }   // (another device: the pool belongs to the old one)
  VNR_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  // the two part streams every renderer uses, right behind it: the runtime gives the first four streams of a process a hardware queue each and
  // every later one the least used queue (ties: any), so the three rendering streams are on three queues whatever is created afterwards
  for (int i = 1; i <= 2; ++i) VNR_HIP_CHECK(hipStreamCreateWithFlags(&part_streams[i], hipStreamNonBlocking));
  device = dev;
}

hipStream_t Runtime::part_stream(int part)
{
  if (part < 1 || part > 3) throw std::runtime_error("internal: ray part stream index");
  if (!ready()) init(-1);
  if (!part_streams[part]) VNR_HIP_CHECK(hipStreamCreateWithFlags(&part_streams[part], hipStreamNonBlocking));
  return part_streams[part];
}

extern "C" {

const char* vnrAmdGetLastError(void) { return g_last_error.c_str(); }
const char* vnrAmdVersion(void) { return "instantvnr_amd 0.1 (gfx950)"; }
int vnrAmdInit(int device) { return guarded([&]() { Runtime::get().init(device); }); }
int vnrAmdDeviceCount(void)
{
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return 0;
  return count;
}
int vnrAmdHasDevice(void) { return vnrAmdDeviceCount() > 0 ? 1 : 0; }

void* vnrAmdMalloc(size_t bytes)
{
  void* p = nullptr;
  guarded([&]() {
    if (!Runtime::get().ready()) Runtime::get().init(-1);
    VNR_HIP_CHECK(hipMalloc(&p, bytes ? bytes : 1));
  });
  return p;
}
int vnrAmdFree(void* p) { return guarded([&]() { if (p) VNR_HIP_CHECK(hipFree(p)); }); }
int vnrAmdMemcpyH2D(void* d, const void* h, size_t n)
{
  return guarded([&]() {
    VNR_HIP_CHECK(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, Runtime::get().stream));
    VNR_HIP_CHECK(hipStreamSynchronize(Runtime::get().stream));
  });
}
int vnrAmdMemcpyD2H(void* h, const void* d, size_t n)
{
  return guarded([&]() {
    VNR_HIP_CHECK(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, Runtime::get().stream));
    VNR_HIP_CHECK(hipStreamSynchronize(Runtime::get().stream));
  });
}
int vnrAmdMemset(void* d, int value, size_t n)
{
  return guarded([&]() {
    VNR_HIP_CHECK(hipMemsetAsync(d, value, n, Runtime::get().stream));
    VNR_HIP_CHECK(hipStreamSynchronize(Runtime::get().stream));
  });
}
int vnrAmdSynchronize(void) { return guarded([&]() { VNR_HIP_CHECK(hipDeviceSynchronize()); }); }
void* vnrAmdDefaultStream(void)
{
  void* s = nullptr;
  guarded([&]() { if (!Runtime::get().ready()) Runtime::get().init(-1); s = (void*)Runtime::get().stream; });
  return s;
}

// ------------------------------------------------------------------------------------------------ JSON
int vnrAmdJsonConvert(const void* data, size_t size, int format_in, int format_out, void** out, size_t* out_size)
{
  return guarded([&]() {
    const Json j = parse_json_arg(data, size, format_in);
    if (format_out == VNR_AMD_JSON_BSON) {
      const std::vector<uint8_t> b = j.to_bson();
      *out = dup_bytes(b.data(), b.size());
      *out_size = b.size();
    } else if (format_out == VNR_AMD_JSON_TEXT) {
      const std::string s = j.dump(4);
      *out = dup_bytes(s.data(), s.size());
      *out_size = s.size();
    } else {
      throw std::runtime_error("format_out must be TEXT or BSON");
    }
  });
}

int vnrAmdJsonSave(const void* data, size_t size, int format_in, const char* filename, int format_out)
{
  return guarded([&]() {
    const Json j = parse_json_arg(data, size, format_in);
    if (format_out == VNR_AMD_JSON_BSON || format_out == VNR_AMD_JSON_BSON_FILE) {  // api.cpp:41-47
      const std::vector<uint8_t> b = j.to_bson();
      std::ofstream ofs(filename, std::ios::binary | std::ios::out);
      ofs.write((const char*)b.data(), (std::streamsize)b.size());
      if (!ofs) throw std::runtime_error(std::string("cannot write ") + filename);
    } else {  // api.cpp:34-39
      std::ofstream ofs(filename, std::ios::out);
      ofs << j.dump(4) << std::endl;
      if (!ofs) throw std::runtime_error(std::string("cannot write ") + filename);
    }
  });
}

void vnrAmdFreeHost(void* p) { std::free(p); }

// ------------------------------------------------------------------------------------------------ camera
vnrAmdCamera vnrAmdCreateCamera(void) { return guarded_new<vnrAmdCamera_t>([]() { return new vnrAmdCamera_t(); }); }
int vnrAmdCameraSet(vnrAmdCamera c, const float from[3], const float at[3], const float up[3])
{
  return guarded([&]() {
    if (!c) throw std::runtime_error("null camera");
    c->d.from = {from[0], from[1], from[2]};
    c->d.at = {at[0], at[1], at[2]};
    c->d.up = {up[0], up[1], up[2]};
  });
}
int vnrAmdCameraSetFromScene(vnrAmdCamera c, const void* scene, size_t size, int format)
{
  return guarded([&]() {
    if (!c) throw std::runtime_error("null camera");
    (void)parse_scene_camera(resolve_config(parse_json_arg(scene, size, format)), c->d);
  });
}
int vnrAmdCameraSetFovy(vnrAmdCamera c, float fovy)
{
  return guarded([&]() { if (!c) throw std::runtime_error("null camera"); c->d.fovy = fovy; });
}
int vnrAmdCameraGet(vnrAmdCamera c, float from[3], float at[3], float up[3], float* fovy)
{
  return guarded([&]() {
    if (!c) throw std::runtime_error("null camera");
    if (from) { from[0] = c->d.from.x; from[1] = c->d.from.y; from[2] = c->d.from.z; }
    if (at) { at[0] = c->d.at.x; at[1] = c->d.at.y; at[2] = c->d.at.z; }
    if (up) { up[0] = c->d.up.x; up[1] = c->d.up.y; up[2] = c->d.up.z; }
    if (fovy) *fovy = c->d.fovy;
  });
}
void vnrAmdReleaseCamera(vnrAmdCamera c) { delete c; }

// ------------------------------------------------------------------------------------------------ transfer function
vnrAmdTransferFunction vnrAmdCreateTransferFunction(void)
{
  return guarded_new<vnrAmdTransferFunction_t>([]() { return new vnrAmdTransferFunction_t(); });
}
int vnrAmdTransferFunctionSetColor(vnrAmdTransferFunction t, const float* rgb, int n)
{
  return guarded([&]() {
    if (!t) throw std::runtime_error("null transfer function");
    t->d.color.resize((size_t)n);
    for (int i = 0; i < n; ++i) t->d.color[i] = {rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]};
  });
}
int vnrAmdTransferFunctionSetAlpha(vnrAmdTransferFunction t, const float* xy, int n)
{
  return guarded([&]() {
    if (!t) throw std::runtime_error("null transfer function");
    t->d.alpha.resize((size_t)n);
    for (int i = 0; i < n; ++i) t->d.alpha[i] = {xy[2 * i], xy[2 * i + 1]};
  });
}
int vnrAmdTransferFunctionSetValueRange(vnrAmdTransferFunction t, float lo, float hi)
{
  return guarded([&]() {
    if (!t) throw std::runtime_error("null transfer function");
    t->d.range_lo = lo; t->d.range_hi = hi; t->d.range_set = true;
  });
}
int vnrAmdTransferFunctionGetSizes(vnrAmdTransferFunction t, int* nc, int* na)
{
  return guarded([&]() {
    if (!t) throw std::runtime_error("null transfer function");
    if (nc) *nc = (int)t->d.color.size();
    if (na) *na = (int)t->d.alpha.size();
  });
}
int vnrAmdTransferFunctionGet(vnrAmdTransferFunction t, float* rgb, float* xy, float range[2])
{
  return guarded([&]() {
    if (!t) throw std::runtime_error("null transfer function");
    if (rgb) for (size_t i = 0; i < t->d.color.size(); ++i) { rgb[3 * i] = t->d.color[i].x; rgb[3 * i + 1] = t->d.color[i].y; rgb[3 * i + 2] = t->d.color[i].z; }
    if (xy) for (size_t i = 0; i < t->d.alpha.size(); ++i) { xy[2 * i] = t->d.alpha[i].x; xy[2 * i + 1] = t->d.alpha[i].y; }
    if (range) { range[0] = t->d.range_lo; range[1] = t->d.range_hi; }
  });
}
void vnrAmdReleaseTransferFunction(vnrAmdTransferFunction t) { delete t; }

// ------------------------------------------------------------------------------------------------ simple volume
vnrAmdVolume vnrAmdCreateSimpleVolumeFromMemory(const void* host_data, const int dims[3], int value_type, float lo, float hi)
{
  return guarded_new<vnrAmdVolume_t>([&]() {
    auto sv = std::make_shared<SimpleVolume>();
    sv->load_host(host_data, {dims[0], dims[1], dims[2]}, value_type, lo, hi);
    auto* h = new vnrAmdVolume_t();
    h->v = sv;
    return h;
  });
}
vnrAmdVolume vnrAmdCreateSimpleVolumeFromRawFile(const char* filename, const int dims[3], int value_type, size_t offset,
                                                 int big_endian, float lo, float hi)
{
  return guarded_new<vnrAmdVolume_t>([&]() {
    auto sv = std::make_shared<SimpleVolume>();
    sv->load_raw_file(filename, {dims[0], dims[1], dims[2]}, value_type, offset, big_endian != 0, lo, hi);
    auto* h = new vnrAmdVolume_t();
    h->v = sv;
    return h;
  });
}
vnrAmdVolume vnrAmdCreateSimpleVolumePerlin(const int dims[3], uint32_t seed, int octaves, float base_frequency)
{
  return guarded_new<vnrAmdVolume_t>([&]() {
    auto sv = std::make_shared<SimpleVolume>();
    sv->generate_perlin({dims[0], dims[1], dims[2]}, seed, octaves, base_frequency);
    auto* h = new vnrAmdVolume_t();
    h->v = sv;
    return h;
  });
}
vnrAmdVolume vnrAmdCreateSimpleVolumeOutOfCore(const char* filename, const int dims[3], int value_type, size_t offset, float lo, float hi,
                                               uint64_t n_concurrent_blocks, uint64_t n_blocks)
{
  return guarded_new<vnrAmdVolume_t>([&]() {
    // neural_sampler.cpp:1054-1062
    uint64_t ncb = n_concurrent_blocks, nb = n_blocks;
    if (ncb == 0) {
      ncb = 1024;
      if (const char* e = std::getenv("VNR_NUM_CONCURRENT_BLOCKS")) ncb = (uint64_t)std::max(1, std::atoi(e));
    }
    if (nb == 0) {
      nb = ncb * 64;
      if (const char* e = std::getenv("VNR_NUM_BLOCKS")) nb = (uint64_t)std::max(1, std::atoi(e));
    }
    auto sv = std::make_shared<SimpleVolume>();
    sv->load_out_of_core(filename, {dims[0], dims[1], dims[2]}, value_type, offset, lo, hi, ncb, nb);
    auto* h = new vnrAmdVolume_t();
    h->v = sv;
    return h;
  });
}
vnrAmdVolume vnrAmdCreateSimpleVolumeFromScene(const void* scene, size_t size, int format, const char* mode, int save_loaded_volume)
{
  return guarded_new<vnrAmdVolume_t>([&]() {
    const SceneVolume sc = parse_scene_volume(resolve_config(parse_json_arg(scene, size, format)));
    auto sv = std::make_shared<SimpleVolume>();
    sv->load_scene(sc, mode ? mode : "GPU", save_loaded_volume != 0);
    auto* h = new vnrAmdVolume_t();
    h->v = sv;
    return h;
  });
}
int vnrAmdSimpleVolumeGetNumberOfTimeSteps(vnrAmdVolume v)
{
  int n = -1;
  guarded([&]() { n = as_simple(v)->num_timesteps(); });
  return n;
}
int vnrAmdSimpleVolumeSetCurrentTimeStep(vnrAmdVolume v, int index)
{
  return guarded([&]() { as_simple(v)->set_current_timestep(index); });
}
int vnrAmdSceneGetValueRange(const void* scene, size_t size, int format, float range[2])
{
  int none = 0;
  const int st = guarded([&]() {
    float lo, hi;
    if (parse_scene_tfn_range(resolve_config(parse_json_arg(scene, size, format)), lo, hi)) { range[0] = lo; range[1] = hi; }
    else none = 2;
  });
  return st != 0 ? st : none;
}
int vnrAmdSimpleVolumeOutOfCoreInfo(vnrAmdVolume v, vnrAmdOutOfCoreInfo* info)
{
  return guarded([&]() {
    OutOfCoreSampler* o = as_simple(v)->out_of_core();
    if (!o) throw std::runtime_error("not an out-of-core volume");
    const vec3i d = o->dims(), b = o->block_dims(), g = o->block_index_space();
    info->file_dims[0] = d.x; info->file_dims[1] = d.y; info->file_dims[2] = d.z;
    info->block_dims[0] = b.x; info->block_dims[1] = b.y; info->block_dims[2] = b.z;
    info->block_index_space[0] = g.x; info->block_index_space[1] = g.y; info->block_index_space[2] = g.z;
    info->n_blocks = o->n_blocks(); info->n_concurrent_blocks = o->n_concurrent_blocks();
    info->block_size_aligned = o->block_size_aligned(); info->bytes_read = o->bytes_read();
  });
}
int vnrAmdSimpleVolumeOutOfCoreSetAsyncRefresh(vnrAmdVolume v, int enable)
{
  return guarded([&]() {
    OutOfCoreSampler* o = as_simple(v)->out_of_core();
    if (!o) throw std::runtime_error("not an out-of-core volume");
    o->set_async_refresh(enable != 0);
  });
}
int vnrAmdSimpleVolumeOutOfCoreRefreshStats(vnrAmdVolume v, uint64_t* refreshes, uint64_t* steps_without_refresh)
{
  return guarded([&]() {
    OutOfCoreSampler* o = as_simple(v)->out_of_core();
    if (!o) throw std::runtime_error("not an out-of-core volume");
    if (refreshes) *refreshes = o->refreshes();
    if (steps_without_refresh) *steps_without_refresh = o->steps_without_refresh();
  });
}
int vnrAmdSimpleVolumeOutOfCoreBlocks(vnrAmdVolume v, int* block_index_yz, size_t n_slots)
{
  return guarded([&]() {
    OutOfCoreSampler* o = as_simple(v)->out_of_core();
    if (!o) throw std::runtime_error("not an out-of-core volume");
    const std::vector<OocBlock> b = o->blocks();
    if (n_slots != b.size()) throw std::runtime_error("slot count mismatch");
    for (size_t i = 0; i < b.size(); ++i) { block_index_yz[2 * i] = b[i].index_y; block_index_yz[2 * i + 1] = b[i].index_z; }
  });
}
vnrAmdVolume vnrAmdCreateSimpleVolumeFromDevice(const void* d_data, const int dims[3], int value_type, const int64_t strides[3],
                                                float lo, float hi, void* stream, float used_range[2])
{
  return guarded_new<vnrAmdVolume_t>([&]() {
    if (!dims) throw std::runtime_error("null dims");
    auto sv = std::make_shared<SimpleVolume>();
    sv->create_from_device(DeviceSource{d_data, value_type, strides, (hipStream_t)stream}, {dims[0], dims[1], dims[2]}, lo, hi, used_range);
    auto* h = new vnrAmdVolume_t();
    h->v = sv;
    return h;
  });
}
int vnrAmdSimpleVolumeUpdateFromDevice(vnrAmdVolume v, const void* d_data, int value_type, const int64_t strides[3], float lo, float hi,
                                       void* stream, float used_range[2])
{
  return guarded([&]() {
    as_simple(v)->update_from_device(DeviceSource{d_data, value_type, strides, (hipStream_t)stream}, lo, hi, used_range);
  });
}
int vnrAmdSimpleVolumeAppendTimeStepFromDevice(vnrAmdVolume v, const void* d_data, int value_type, const int64_t strides[3], float lo,
                                               float hi, void* stream, float used_range[2])
{
  int index = -1;
  guarded([&]() {
    index = as_simple(v)->append_from_device(DeviceSource{d_data, value_type, strides, (hipStream_t)stream}, lo, hi, used_range);
  });
  return index;
}
const float* vnrAmdSimpleVolumeDeviceData(vnrAmdVolume v)
{
  const float* p = nullptr;
  guarded([&]() { p = as_simple(v)->d_data(); });
  return p;
}

// ------------------------------------------------------------------------------------------------ neural volume
vnrAmdVolume vnrAmdCreateNeuralVolume(const void* config, size_t size, int format, vnrAmdVolume groundtruth, int online_mc)
{
  return guarded_new<vnrAmdVolume_t>([&]() {
    SimpleVolume* src = as_simple(groundtruth);
    const Json cfg = resolve_config(parse_json_arg(config, size, format));
    auto nv = std::make_shared<NeuralVolume>();
    if (const char* e = std::getenv("VNR_AMD_INIT_SEED")) nv->init_seed = std::strtoull(e, nullptr, 10);
    nv->keep_source_alive(groundtruth->v);
    nv->set_network(src->dims(), cfg, src, !online_mc);  // api.cpp:181-184
    auto* h = new vnrAmdVolume_t();
    h->v = nv;
    return h;
  });
}
vnrAmdVolume vnrAmdCreateNeuralVolumeFromDims(const void* config, size_t size, int format, const int dims[3])
{
  return guarded_new<vnrAmdVolume_t>([&]() {
    const Json cfg = resolve_config(parse_json_arg(config, size, format));
    auto nv = std::make_shared<NeuralVolume>();
    if (const char* e = std::getenv("VNR_AMD_INIT_SEED")) nv->init_seed = std::strtoull(e, nullptr, 10);
    nv->set_network({dims[0], dims[1], dims[2]}, cfg, nullptr, false);  // api.cpp:190-204
    auto* h = new vnrAmdVolume_t();
    h->v = nv;
    return h;
  });
}
vnrAmdVolume vnrAmdCreateNeuralVolumeFromParams(const void* params, size_t size, int format)
{
  return guarded_new<vnrAmdVolume_t>([&]() {
    const Json p = resolve_params(parse_json_arg(params, size, format));
    if (!p.contains("volume")) throw std::runtime_error("expecting a model config with volume dims tag");  // api.cpp:214-216
    const Json& d = p.at("volume").at("dims");
    const vec3i dims = {(int)d.at("x").as_int(), (int)d.at("y").as_int(), (int)d.at("z").as_int()};
    auto nv = std::make_shared<NeuralVolume>();
    nv->init_seed = 1;
    nv->set_network(dims, p.at("model"), nullptr, false);
    nv->load_params_from_json(p);
    auto* h = new vnrAmdVolume_t();
    h->v = nv;
    return h;
  });
}
int vnrAmdNeuralVolumeSetModel(vnrAmdVolume v, const void* config, size_t size, int format)
{
  return guarded([&]() { as_neural(v)->set_model(resolve_config(parse_json_arg(config, size, format))); });
}
int vnrAmdNeuralVolumeSetParams(vnrAmdVolume v, const void* params, size_t size, int format)
{
  return guarded([&]() { as_neural(v)->load_params_from_json(resolve_params(parse_json_arg(params, size, format))); });
}
double vnrAmdNeuralVolumeGetPSNR(vnrAmdVolume v, int verbose)
{
  double r = -1.0;
  guarded([&]() { r = as_neural(v)->get_psnr(!verbose); });
  return r;
}
double vnrAmdNeuralVolumeGetSSIM(vnrAmdVolume v, int verbose)
{
  double r = -1.0;  // SSIM itself lies in (-1, 1]; -1 doubles as the error value like the reference's get_mssim
  guarded([&]() { r = as_neural(v)->get_ssim(!verbose); });
  return r;
}
double vnrAmdNeuralVolumeGetTestingLoss(vnrAmdVolume v)
{
  double r = -1.0;
  guarded([&]() { r = as_neural(v)->test_loss(); });
  return r;
}
double vnrAmdNeuralVolumeGetTrainingLoss(vnrAmdVolume v)
{
  double r = -1.0;
  guarded([&]() { NeuralVolume* n = as_neural(v); r = n->network().training_loss(n->stream); });
  return r;
}
int vnrAmdNeuralVolumeGetTrainingStep(vnrAmdVolume v)
{
  int r = -1;
  guarded([&]() { r = (int)as_neural(v)->network().steps(); });
  return r;
}
int vnrAmdNeuralVolumeGetNumberOfBlobs(vnrAmdVolume v)
{
  int r = -1;
  guarded([&]() { r = as_neural(v)->num_blobs(); });
  return r;
}
int vnrAmdNeuralVolumeTrain(vnrAmdVolume v, int steps, int fast_mode)
{
  return guarded([&]() { as_neural(v)->train((size_t)std::max(steps, 0), fast_mode != 0); });
}
int vnrAmdNeuralVolumeDecodeProgressive(vnrAmdVolume v)
{
  return guarded([&]() { as_neural(v)->decode_progressive(); });
}
int vnrAmdNeuralVolumeDecodeInference(vnrAmdVolume v, const char* filename)
{
  return guarded([&]() {
    if (!filename) throw std::runtime_error("filename is null");
    as_neural(v)->save_inference_volume(filename);
  });
}
int vnrAmdNeuralVolumeDecodeReference(vnrAmdVolume v, const char* filename)
{
  return guarded([&]() {
    if (!filename) throw std::runtime_error("filename is null");
    as_neural(v)->save_reference_volume(filename);
  });
}
const float* vnrAmdNeuralVolumeDecodedDeviceData(vnrAmdVolume v)
{
  const float* r = nullptr;
  guarded([&]() { r = as_neural(v)->decoded_data(); });
  return r;
}
int vnrAmdNeuralVolumeDecodeToDevice(vnrAmdVolume v, void* d_out, int value_type, const int64_t strides[3], const int box_lo[3],
                                     const int box_size[3], const int grid_dims[3], float range_lo, float range_hi, void* stream)
{
  return guarded([&]() {
    as_neural(v)->decode_to_device(DeviceTarget{d_out, value_type, strides, (hipStream_t)stream}, box_lo, box_size, grid_dims, range_lo, range_hi);
  });
}
int vnrAmdNeuralVolumeErrorAgainstDevice(vnrAmdVolume v, const void* d_ref, int value_type, const int64_t strides[3], const int box_lo[3],
                                         const int box_size[3], float range_lo, float range_hi, void* stream, vnrAmdDecodeError* out,
                                         float* d_block_max)
{
  static_assert(sizeof(vnrAmdDecodeError) == sizeof(DecodeError), "vnrAmdDecodeError and vnr::DecodeError are one layout");
  return guarded([&]() {
    as_neural(v)->error_against_device(DeviceSource{d_ref, value_type, strides, (hipStream_t)stream}, box_lo, box_size, range_lo, range_hi,
                                       reinterpret_cast<DecodeError*>(out), d_block_max);
  });
}
vnrAmdCorrection vnrAmdNeuralVolumeBuildCorrection(vnrAmdVolume v, const void* d_ref, int value_type, const int64_t strides[3], float range_lo, float range_hi,
                                                   double eps, void* stream)
{
  return guarded_new<vnrAmdCorrection_t>([&]() {
    return new vnrAmdCorrection_t{as_neural(v)->build_correction(DeviceSource{d_ref, value_type, strides, (hipStream_t)stream}, range_lo, range_hi, eps)};
  });
}
vnrAmdCorrection vnrAmdNeuralVolumeBuildCorrectionPacked(vnrAmdVolume v, const void* d_ref, int value_type, const int64_t strides[3], float range_lo, float range_hi,
                                                         double eps, void* stream)
{
  return guarded_new<vnrAmdCorrection_t>([&]() {
    return new vnrAmdCorrection_t{as_neural(v)->build_correction_packed(DeviceSource{d_ref, value_type, strides, (hipStream_t)stream}, range_lo, range_hi, eps)};
  });
}
int vnrAmdCorrectionSerializePackedToDevice(vnrAmdCorrection c, void* d_bytes, size_t capacity, size_t* size, void* stream)
{
  return serialize_correction_to_device(c, CorrectionForm::Packed, d_bytes, capacity, size, stream);
}
int vnrAmdNeuralVolumeCorrectionRates(vnrAmdVolume v, const void* d_ref, int value_type, const int64_t strides[3], float range_lo, float range_hi,
                                      const double* eps, int n_eps, void* stream, vnrAmdCorrectionRate* out)
{
  static_assert(sizeof(vnrAmdCorrectionRate) == sizeof(CorrectionRate), "vnrAmdCorrectionRate and vnr::CorrectionRate are one layout");
  return guarded([&]() {
    correction_rates_check(eps, n_eps, reinterpret_cast<CorrectionRate*>(out));   // (what needs no volume comes first)
    as_neural(v)->correction_rates(DeviceSource{d_ref, value_type, strides, (hipStream_t)stream}, range_lo, range_hi, eps, n_eps,
                                   reinterpret_cast<CorrectionRate*>(out));
  });
}
vnrAmdCorrection vnrAmdNeuralVolumeBuildCorrectionWithinBytes(vnrAmdVolume v, const void* d_ref, int value_type, const int64_t strides[3], float range_lo,
                                                              float range_hi, uint64_t max_bytes, int form, double eps_hi, int rounds, void* stream,
                                                              vnrAmdCorrectionBudget* report)
{
  return guarded_new<vnrAmdCorrection_t>([&]() {
    if (!report) throw std::runtime_error("null result");
    if (form != VNR_AMD_CORRECTION_FORM_FIXED && form != VNR_AMD_CORRECTION_FORM_PACKED)
      throw std::runtime_error("unknown serialised form " + std::to_string(form) + " (0: fixed-width, 1: packed)");
    return build_within_bytes(v, DeviceSource{d_ref, value_type, strides, (hipStream_t)stream}, range_lo, range_hi, max_bytes, (CorrectionForm)form, eps_hi, rounds, report);
  });
}
int vnrAmdNeuralVolumeCorrectionRatesCoded(vnrAmdVolume v, const void* d_ref, int value_type, const int64_t strides[3], float range_lo, float range_hi,
                                           const double* eps, int n_eps, void* stream, vnrAmdCorrectionRateCoded* out)
{
  static_assert(sizeof(vnrAmdCorrectionRateCoded) == sizeof(CorrectionRateCoded) && sizeof(CorrectionRateCoded) == 96 &&
                    offsetof(vnrAmdCorrectionRateCoded, coded_stream_words) == sizeof(vnrAmdCorrectionRate),
                "vnrAmdCorrectionRateCoded and vnr::CorrectionRateCoded are one layout");
  return guarded([&]() {
    CorrectionRateCoded* o = reinterpret_cast<CorrectionRateCoded*>(out);
    correction_rates_check(eps, n_eps, o ? &o->rate : nullptr);   // (what needs no volume comes first)
    as_neural(v)->correction_rates_coded(DeviceSource{d_ref, value_type, strides, (hipStream_t)stream}, range_lo, range_hi, eps, n_eps, o);
  });
}
vnrAmdCorrection vnrAmdNeuralVolumeBuildCorrectionCodedWithinBytes(vnrAmdVolume v, const void* d_ref, int value_type, const int64_t strides[3], float range_lo,
                                                                   float range_hi, uint64_t max_bytes, double eps_hi, int rounds, void* stream,
                                                                   vnrAmdCorrectionBudget* report)
{
  return guarded_new<vnrAmdCorrection_t>([&]() {
    if (!report) throw std::runtime_error("null result");
    return build_within_bytes(v, DeviceSource{d_ref, value_type, strides, (hipStream_t)stream}, range_lo, range_hi, max_bytes, CorrectionForm::Coded, eps_hi, rounds, report);
  });
}
int vnrAmdCorrectionGetInfo(vnrAmdCorrection c, vnrAmdCorrectionInfo* out)
{
  return guarded([&]() {
    Correction* k = as_correction(c);
    if (!out) throw std::runtime_error("null result");
    const CorrectionHeader& h = k->data.h;
    // nothing is moved or converted for this: the fixed-width payload's size follows from the entries
    const uint64_t payload_bytes = correction_fixed_payload_bytes(h, k->data.cells);
    *out = vnrAmdCorrectionInfo{};
    for (int a = 0; a < 3; ++a) { out->dims[a] = h.dims[a]; out->worst_after[a] = k->worst_after[a]; }
    out->value_type = h.value_type; out->kind = (int)h.kind; out->eps = h.eps; out->range_lo = h.range_lo; out->range_hi = h.range_hi;
    out->n_cells = correction_n_cells(h.dims); out->n_flagged = k->data.cells.size(); out->n_voxels_flagged = k->n_voxels_flagged;
    out->payload_bytes = payload_bytes; out->serialized_bytes = kCorrectionHeaderBytes + 8 * k->data.cells.size() + payload_bytes; out->n_nan = k->n_nan;
    out->params_hash = h.params_hash; out->n_params = h.n_params; out->max_abs_before = k->max_abs_before; out->max_abs_after = h.max_abs_after;
  });
}
int vnrAmdCorrectionSerialize(vnrAmdCorrection c, void** bytes, size_t* size)
{
  return serialize_correction(c, CorrectionForm::Fixed, bytes, size);
}
vnrAmdCorrection vnrAmdCreateCorrectionFromBytes(const void* bytes, size_t size)
{
  return guarded_new<vnrAmdCorrection_t>([&]() {
    auto k = std::make_shared<Correction>(CorrectionOrigin::FixedBytes);
    CorrectionData p = correction_parse(bytes, size);
    k->data.payload = std::move(p.payload);
    return read_correction(std::move(k), p.h, std::move(p.cells));
  });
}
int vnrAmdCorrectionSerializePacked(vnrAmdCorrection c, void** bytes, size_t* size)
{
  return serialize_correction(c, CorrectionForm::Packed, bytes, size);
}
vnrAmdCorrection vnrAmdCreateCorrectionFromPackedBytes(const void* bytes, size_t size)
{
  return guarded_new<vnrAmdCorrection_t>([&]() {
    auto k = std::make_shared<Correction>(CorrectionOrigin::PackedBytes);
    CorrectionPacked p = correction_packed_parse(bytes, size);
    k->packed_payload = std::move(p.payload);
    return read_correction(std::move(k), p.h, std::move(p.cells));
  });
}
int vnrAmdCorrectionSerializeCoded(vnrAmdCorrection c, void** bytes, size_t* size)
{
  return serialize_correction(c, CorrectionForm::Coded, bytes, size);
}
vnrAmdCorrection vnrAmdCreateCorrectionFromCodedBytes(const void* bytes, size_t size)
{
  return guarded_new<vnrAmdCorrection_t>([&]() {
    auto k = std::make_shared<Correction>(CorrectionOrigin::CodedBytes);
    CorrectionCoded p = correction_coded_parse(bytes, size);
    k->coded_payload = std::move(p.payload);
    k->group_table = std::move(p.group_nbits);
    return read_correction(std::move(k), p.h, std::move(p.cells));
  });
}
int vnrAmdCorrectionSerializeCodedToDevice(vnrAmdCorrection c, void* d_bytes, size_t capacity, size_t* size, void* stream)
{
  return serialize_correction_to_device(c, CorrectionForm::Coded, d_bytes, capacity, size, stream);
}
int vnrAmdNeuralVolumeDecodeToDeviceCorrected(vnrAmdVolume v, vnrAmdCorrection c, void* d_out, const int64_t strides[3], void* stream, int verify_params)
{
  return vnrAmdNeuralVolumeDecodeBoxToDeviceCorrected(v, c, d_out, strides, nullptr, nullptr, stream, verify_params);   // the whole grid
}
int vnrAmdNeuralVolumeDecodeBoxToDeviceCorrected(vnrAmdVolume v, vnrAmdCorrection c, void* d_out, const int64_t strides[3], const int box_lo[3],
                                                 const int box_size[3], void* stream, int verify_params)
{
  return guarded([&]() {
    NeuralVolume* n = as_neural(v);
    Correction* k = as_correction(c);
    n->decode_to_device_corrected(*k, DeviceTarget{d_out, k->data.h.value_type, strides, (hipStream_t)stream}, box_lo, box_size, verify_params != 0);
  });
}
int vnrAmdNeuralVolumeGatherVoxelsCorrected(vnrAmdVolume v, vnrAmdCorrection c, size_t n, const int32_t* d_voxels, void* d_out, void* stream, int verify_params)
{
  return guarded([&]() {
    Correction* k = as_correction(c);   // (what needs no volume comes first)
    if (!d_voxels) throw std::runtime_error("null voxel list");
    if (!d_out) throw std::runtime_error("null device data");
    const size_t ts = device_value_type_size(k->data.h.value_type);
    if ((uintptr_t)d_voxels % sizeof(int32_t) != 0) throw std::runtime_error("the voxel list is not aligned to 4 bytes");
    if ((uintptr_t)d_out % ts != 0) throw std::runtime_error("device data is not aligned to its value type (" + std::to_string(ts) + " bytes)");
    as_neural(v)->gather_voxels_corrected(*k, n, d_voxels, d_out, (hipStream_t)stream, verify_params != 0);
  });
}
int vnrAmdNeuralVolumeSampleCorrected(vnrAmdVolume v, vnrAmdCorrection c, size_t n, const float* d_coords, float* d_values, void* stream, int verify_params)
{
  return guarded([&]() {
    Correction* k = as_correction(c);
    if (k->data.h.kind == kCorrectionVerbatim)
      throw std::runtime_error("a verbatim correction (kind 2, eps == 0) cannot be sampled: its codes are bit patterns, not residuals");
    if (!d_coords) throw std::runtime_error("null coordinates");
    if (!d_values) throw std::runtime_error("null device data");
    if ((uintptr_t)d_coords % sizeof(float) != 0) throw std::runtime_error("the coordinates are not aligned to 4 bytes");
    if ((uintptr_t)d_values % sizeof(float) != 0) throw std::runtime_error("device data is not aligned to its value type (4 bytes)");
    as_neural(v)->sample_corrected(*k, n, d_coords, d_values, (hipStream_t)stream, verify_params != 0);
  });
}
int vnrAmdCorrectionSetResidentForm(vnrAmdCorrection c, int form)
{
  return guarded([&]() {
    Correction* k = as_correction(c);
    correction_set_resident_form(*k, form, Runtime::get().stream);   // (a correction that holds device memory has initialised the runtime)
  });
}
int vnrAmdCorrectionGetResidency(vnrAmdCorrection c, vnrAmdCorrectionResidency* out)
{
  return guarded([&]() {
    Correction* k = as_correction(c);
    if (!out) throw std::runtime_error("null result");
    *out = vnrAmdCorrectionResidency{};
    out->form = k->resident_form;
    out->payload_device_bytes = k->d_payload.bytes() + k->d_packed.bytes();
    out->index_device_bytes = k->d_plane_cells.bytes() + k->d_plane_groups.bytes();
    out->device_bytes = out->payload_device_bytes + out->index_device_bytes + k->d_table.bytes();
    out->on_device = out->device_bytes != 0;
  });
}
void vnrAmdReleaseCorrection(vnrAmdCorrection c) { delete c; }
int vnrAmdNeuralVolumeSerializeParamsToFile(vnrAmdVolume v, const char* filename)
{
  return guarded([&]() {
    Json root = Json::object();
    as_neural(v)->save_params_to_json(root);
    const std::vector<uint8_t> b = root.to_bson();
    std::ofstream ofs(filename, std::ios::binary | std::ios::out);
    ofs.write((const char*)b.data(), (std::streamsize)b.size());
    if (!ofs) throw std::runtime_error(std::string("cannot write ") + filename);
  });
}
int vnrAmdNeuralVolumeSerializeParams(vnrAmdVolume v, void** bson, size_t* size)
{
  return guarded([&]() {
    Json root = Json::object();
    as_neural(v)->save_params_to_json(root);
    const std::vector<uint8_t> b = root.to_bson();
    *bson = dup_bytes(b.data(), b.size());
    *size = b.size();
  });
}
int vnrAmdNeuralVolumeInference(vnrAmdVolume v, size_t n, const float* d_coords, float* d_values, void* stream)
{
  return guarded([&]() {
    NeuralVolume* nv = as_neural(v);
    if (!nv->network().valid()) throw std::runtime_error("network is not valid");
    nv->inference(n, d_coords, d_values, resolve_stream(stream));
  });
}
int vnrAmdNeuralVolumeEncode(vnrAmdVolume v, size_t n, const float* d_coords, uint16_t* d_features, void* stream)
{
  return guarded([&]() { as_neural(v)->network().encode(d_coords, d_features, n, resolve_stream(stream)); });
}
int vnrAmdNeuralVolumeBrickImageInfo(vnrAmdVolume v, int* in_use, size_t* bytes, float* build_ms)
{
  return guarded([&]() {
    const BrickCache& c = as_neural(v)->network().brick_cache();
    if (in_use) *in_use = c.in_use() ? 1 : 0;
    if (bytes) *bytes = c.bytes();
    if (build_ms) *build_ms = c.build_ms();
  });
}
int vnrAmdNeuralVolumeGetModelKind(vnrAmdVolume v, int* activation, int* output_activation, int* grid_type, int* interpolation, int* mfma_inference,
                                   int* mfma_training)
{
  return guarded([&]() {
    Network& n = as_neural(v)->network();
    if (activation) *activation = (int)n.config().activation;
    if (output_activation) *output_activation = (int)n.config().output_activation;
    if (grid_type) *grid_type = (int)n.config().grid_type;
    if (interpolation) *interpolation = (int)n.config().interpolation;
    if (mfma_inference) *mfma_inference = 1;   // since round 4 there is no other kind of kernel
    if (mfma_training) *mfma_training = 1;
  });
}

int vnrAmdNeuralVolumeGetInfo(vnrAmdVolume v, int* n_levels, int* n_features, int* padded_width, int* n_neurons,
                              int* n_hidden_layers, uint64_t* n_params)
{
  return guarded([&]() {
    Network& n = as_neural(v)->network();
    if (n_levels) *n_levels = (int)n.config().n_levels;
    if (n_features) *n_features = (int)n.config().n_features;
    if (padded_width) *padded_width = (int)n.padded_width();
    if (n_neurons) *n_neurons = (int)n.config().n_neurons;
    if (n_hidden_layers) *n_hidden_layers = (int)n.config().n_hidden_layers;
    if (n_params) *n_params = (uint64_t)n.n_params();
  });
}
int vnrAmdNeuralVolumeLevelTable(vnrAmdVolume v, int max_levels, uint32_t* resolution, uint32_t* entries, uint32_t* offset, uint32_t* kind)
{
  int n = -1;
  guarded([&]() {
    const Network& net = as_neural(v)->network();
    const GridDevice& g = net.grid();
    n = (int)net.config().n_levels;
    for (int l = 0; l < n && l < max_levels; ++l) {
      if (resolution) resolution[l] = g.levels[l].resolution;
      if (entries) entries[l] = g.levels[l].size;
      if (offset) offset[l] = g.levels[l].offset;
      if (kind) kind[l] = g.levels[l].hashed;
    }
  });
  return n;
}
int vnrAmdNeuralVolumeGetParamsFP16(vnrAmdVolume v, uint16_t* host_out, size_t count)
{
  return guarded([&]() { NeuralVolume* n = as_neural(v); n->network().get_params_f16(host_out, count, n->stream); });
}
int vnrAmdNeuralVolumeSetParamsFP16(vnrAmdVolume v, const uint16_t* host_in, size_t count)
{
  return guarded([&]() { NeuralVolume* n = as_neural(v); n->network().set_params_f16(host_in, count, n->stream); });
}
int vnrAmdNeuralVolumeTrainBegin(vnrAmdVolume v) { return guarded([&]() { as_neural(v)->train_begin(); }); }
float* vnrAmdNeuralVolumeGradients(vnrAmdVolume v, size_t* count)
{
  float* p = nullptr;
  guarded([&]() {
    NeuralVolume* nv = as_neural(v);
    Network& n = nv->network();
    p = n.grads_as_f32(nv->stream);
    if (count) *count = n.grads_count();
  });
  return p;
}
int vnrAmdNeuralVolumeTrainEnd(vnrAmdVolume v, float grad_scale, int fast_mode)
{
  return guarded([&]() { as_neural(v)->train_end(grad_scale, fast_mode != 0); });
}
int vnrAmdNeuralVolumeForwardBackward(vnrAmdVolume v, size_t n, const float* d_coords, const float* d_targets)
{
  return guarded([&]() { as_neural(v)->forward_backward(d_coords, d_targets, n); });
}
int vnrAmdNeuralVolumeTrainingBuffer(vnrAmdVolume v, int which, const void** d_ptr, size_t* bytes)
{
  return guarded([&]() {
    size_t b = 0;
    const void* p = as_neural(v)->network().training_buffer(which, &b);
    if (d_ptr) *d_ptr = p;
    if (bytes) *bytes = b;
  });
}
int vnrAmdNeuralVolumeRescatterGridGradients(vnrAmdVolume v, size_t n, const float* d_coords)
{
  return guarded([&]() { NeuralVolume* nv = as_neural(v); nv->network().rescatter_grid_gradients(d_coords, n, nv->stream); });
}
int vnrAmdNeuralVolumeGradientDistance(vnrAmdVolume v, const uint16_t* d_reference, double* out4)
{
  return guarded([&]() { NeuralVolume* nv = as_neural(v); nv->network().gradient_distance(d_reference, out4, nv->stream); });
}
int vnrAmdNeuralVolumeSetSamplerSeed(vnrAmdVolume v, uint64_t seed, uint64_t stream_id)
{
  return guarded([&]() {
    NeuralVolume* n = as_neural(v);
    if (!n->source()) throw std::runtime_error("missing a reference volume");
    n->source()->set_sampler_seed(seed, stream_id);
  });
}
int vnrAmdNeuralVolumeSetInitSeed(vnrAmdVolume v, uint64_t seed)
{
  return guarded([&]() { as_neural(v)->init_seed = seed; });
}

// ------------------------------------------------------------------------------------------------ general volume
int vnrAmdVolumeSetClippingBox(vnrAmdVolume v, const float lower[3], const float upper[3])
{
  return guarded([&]() {  // api.cpp:322-338
    if (!v || !v->v) throw std::runtime_error("null volume");
    VolumeBase& vb = *v->v;
    const vec3f half = {vb.desc.dims.x / 2.0f, vb.desc.dims.y / 2.0f, vb.desc.dims.z / 2.0f};
    const affine3f inv = affine_inverse(vb.transform);
    vb.clipbox.lower = xfm_point(inv, vec3f{lower[0], lower[1], lower[2]} - half);
    vb.clipbox.upper = xfm_point(inv, vec3f{upper[0], upper[1], upper[2]} - half);
  });
}
int vnrAmdVolumeSetScaling(vnrAmdVolume v, const float scale[3])
{
  return guarded([&]() {  // api.cpp:340-351: transform = scale(s) * transform
    if (!v || !v->v) throw std::runtime_error("null volume");
    v->v->transform = affine_scale_then({scale[0], scale[1], scale[2]}, v->v->transform);
  });
}
int vnrAmdMarchingCube(vnrAmdVolume v, float isovalue, float** xyz, size_t* n_vertices, int on_device)
{
  return guarded([&]() {
    if (!v || !v->v) throw std::runtime_error("null volume");
    if (!xyz || !n_vertices) throw std::runtime_error("null output pointer");
    DeviceBuffer<vec3f> verts;
    const size_t n = marching_cubes(*v->v, isovalue, verts);
    *n_vertices = n;
    *xyz = nullptr;
    if (on_device) {   // the caller owns the device array: vnrAmdFree
      *xyz = (float*)verts.ptr;
      verts.counter() -= verts.count * sizeof(vec3f);
      verts.ptr = nullptr; verts.count = 0;
    } else if (n) {
      float* h = (float*)std::malloc(n * sizeof(vec3f));
      if (!h) throw std::runtime_error("out of host memory");
      const hipError_t e = hipMemcpy(h, verts.ptr, n * sizeof(vec3f), hipMemcpyDeviceToHost);
      if (e != hipSuccess) { std::free(h); throw std::runtime_error("device to host copy of the vertices failed"); }
      *xyz = h;
    }
  });
}
int vnrAmdSaveTriangles(const char* filename, const float* xyz, size_t n_vertices)
{
  return guarded([&]() { if (!filename) throw std::runtime_error("null file name"); save_triangles_obj(filename, xyz, n_vertices); });
}
int vnrAmdSimpleVolumeGetDataRange(vnrAmdVolume v, float range[2])
{
  return guarded([&]() {
    if (!v || !v->v || v->v->is_network()) throw std::runtime_error("not a simple volume");
    const SimpleVolume* sv = static_cast<const SimpleVolume*>(v->v.get());
    range[0] = sv->unnormalized_lo; range[1] = sv->unnormalized_hi;
  });
}
int vnrAmdVolumeSetTransform(vnrAmdVolume v, const float m[12])
{
  return guarded([&]() {  // MainRenderer::set_scene(..., matrix, ...) of the OVR plugin (device/device_impl.cpp:175-184): object -> world
    if (!v || !v->v) throw std::runtime_error("null volume");
    v->v->transform = affine3f{{m[0], m[1], m[2]}, {m[3], m[4], m[5]}, {m[6], m[7], m[8]}, {m[9], m[10], m[11]}};
  });
}
int vnrAmdVolumeGetValueRange(vnrAmdVolume v, float range[2])
{
  return guarded([&]() {
    if (!v || !v->v) throw std::runtime_error("null volume");
    range[0] = v->v->desc.range_lo; range[1] = v->v->desc.range_hi;
  });
}
int vnrAmdVolumeGetDims(vnrAmdVolume v, int dims[3])
{
  return guarded([&]() {
    if (!v || !v->v) throw std::runtime_error("null volume");
    dims[0] = v->v->desc.dims.x; dims[1] = v->v->desc.dims.y; dims[2] = v->v->desc.dims.z;
  });
}
int vnrAmdVolumeIsNetwork(vnrAmdVolume v) { return (v && v->v && v->v->is_network()) ? 1 : 0; }
int vnrAmdVolumeGetMacrocell(vnrAmdVolume v, int mc_dims[3], float mc_spacings[3], const float** d_value_range, const float** d_max_opacity)
{
  return guarded([&]() {
    if (!v || !v->v) throw std::runtime_error("null volume");
    MacroCell& m = v->v->macrocell();
    const vec3i d = m.dims();
    const vec3f s = m.spacings();
    if (mc_dims) { mc_dims[0] = d.x; mc_dims[1] = d.y; mc_dims[2] = d.z; }
    if (mc_spacings) { mc_spacings[0] = s.x; mc_spacings[1] = s.y; mc_spacings[2] = s.z; }
    if (d_value_range) *d_value_range = m.d_value_range();
    if (d_max_opacity) *d_max_opacity = m.d_max_opacity();
  });
}
void vnrAmdReleaseVolume(vnrAmdVolume v) { delete v; }

// ------------------------------------------------------------------------------------------------ renderer
vnrAmdRenderer vnrAmdCreateRenderer(vnrAmdVolume v)
{
  return guarded_new<vnrAmdRenderer_t>([&]() {
    if (!v || !v->v) throw std::runtime_error("null volume");
    auto* h = new vnrAmdRenderer_t();
    h->volume = v->v;
    h->r = std::make_unique<Renderer>(v->v);
    return h;
  });
}
#define VNR_REN(r) do { if (!(r) || !(r)->r) throw std::runtime_error("null renderer"); } while (0)
int vnrAmdRendererSetFramebufferSize(vnrAmdRenderer r, int w, int h) { return guarded([&]() { VNR_REN(r); r->r->resize(w, h); }); }
int vnrAmdRendererSetTransferFunction(vnrAmdRenderer r, vnrAmdTransferFunction t)
{
  return guarded([&]() { VNR_REN(r); if (!t) throw std::runtime_error("null transfer function"); r->r->set_transfer_function(t->d); });
}
int vnrAmdRendererSetCamera(vnrAmdRenderer r, vnrAmdCamera c)
{
  return guarded([&]() { VNR_REN(r); if (!c) throw std::runtime_error("null camera"); r->r->set_camera(c->d); });
}
int vnrAmdRendererSetMode(vnrAmdRenderer r, int mode) { return guarded([&]() { VNR_REN(r); r->r->set_mode(mode); }); }
// vnrRendererSetDenoiser (api.cpp:466): the reference runs OptiX's trained denoiser (optix_program.h:151-230, NVIDIA's weights: not something to
// restate).  ONE behaviour (round 5): the call is accepted either way -- the reference's interactive apps make it from a checkbox, and an
// unchanged app must not die of an exception there -- and switching it ON says once on stderr that frames stay undenoised.
// VNR_AMD_DENOISER_STRICT=1 refuses instead, for hosts that would rather fail than show an undenoised frame as a denoised one.
int vnrAmdRendererSetDenoiser(vnrAmdRenderer r, int enable)
{
  return guarded([&]() {
    VNR_REN(r);
    if (!enable) return;
    const char* e = std::getenv("VNR_AMD_DENOISER_STRICT");
    if (e && std::atoi(e) != 0) throw std::runtime_error("the denoiser is not available (the reference's is OptiX's trained denoiser; VNR_AMD_DENOISER_STRICT=1 turns the warning into this error)");
    static bool warned = false;
    if (!warned) { std::fprintf(stderr, "[vnr_amd] vnrRendererSetDenoiser(true): no denoiser here (the reference's is OptiX's); frames are NOT denoised\n"); warned = true; }
  });
}
int vnrAmdRendererSetVolumeSamplingRate(vnrAmdRenderer r, float rate) { return guarded([&]() { VNR_REN(r); r->r->set_sampling_rate(rate); }); }
int vnrAmdRendererSetVolumeDensityScale(vnrAmdRenderer r, float s) { return guarded([&]() { VNR_REN(r); r->r->set_density_scale(s); }); }
int vnrAmdRendererResetAccumulation(vnrAmdRenderer r) { return guarded([&]() { VNR_REN(r); r->r->reset_accumulation(); }); }
int vnrAmdRender(vnrAmdRenderer r) { return guarded([&]() { VNR_REN(r); r->r->render(); }); }
const float* vnrAmdRendererMapFrame(vnrAmdRenderer r)
{
  const float* p = nullptr;
  guarded([&]() { VNR_REN(r); p = r->r->map_frame(); });
  return p;
}
int vnrAmdRendererSetOutputAsDeviceFramebuffer(vnrAmdRenderer r, int e) { return guarded([&]() { VNR_REN(r); r->r->set_device_output(e != 0); }); }
int vnrAmdRendererSetPixelRange(vnrAmdRenderer r, uint32_t lo, uint32_t hi) { return guarded([&]() { VNR_REN(r); r->r->set_pixel_range(lo, hi); }); }
int vnrAmdRendererSetPixelInterleave(vnrAmdRenderer r, uint32_t block, uint32_t parts, uint32_t part)
{
  return guarded([&]() { VNR_REN(r); r->r->set_pixel_interleave(block, parts, part); });
}
int vnrAmdRendererGetFrameStats(vnrAmdRenderer r, vnrAmdFrameStats* s)
{
  return guarded([&]() {
    VNR_REN(r);
    const FrameStats& f = r->r->stats();
    s->n_samples = f.n_samples; s->n_reference_slots = f.n_reference_slots; s->n_iterations = f.n_iterations;
    s->n_rays_hit = f.n_rays_hit; s->infer_kernel_ms = f.infer_kernel_ms; s->infer_kernel_launches = f.infer_kernel_launches; s->infer_union_ms = f.infer_union_ms;
  });
}
int vnrAmdRendererDebugQueues(vnrAmdRenderer r, const float** d_coords, const uint32_t** d_counters, float* iteration_ms, int max_iterations)
{
  return guarded([&]() {
    VNR_REN(r);
    if (d_coords) *d_coords = r->r->debug_coords();
    if (d_counters) *d_counters = r->r->debug_counters();
    const auto& v = r->r->debug_iteration_ms();
    for (int i = 0; i < max_iterations; ++i) iteration_ms[i] = i < (int)v.size() ? v[i] : 0.0f;
  });
}
int vnrAmdRendererDebugSchedule(vnrAmdRenderer r, int out[4])
{
  return guarded([&]() {
    VNR_REN(r);
    if (!out) throw std::runtime_error("null output");
    const int* v = r->r->debug_schedule();
    for (int i = 0; i < 4; ++i) out[i] = v[i];
  });
}
int vnrAmdRendererGetSchedule(vnrAmdRenderer r, vnrAmdSchedule* out)
{
  return guarded([&]() {
    VNR_REN(r);
    if (!out) throw std::runtime_error("null output");
    const int* v = r->r->debug_schedule();
    out->n_iters = v[0]; out->n_parts = v[1]; out->fused_pack = v[2]; out->decoupled = v[3];
    out->tfn_in_lds = r->r->tfn_in_lds() ? 1 : 0;
    out->tfn_lds_bytes = (int)Renderer::kTfnLdsBytes;
  });
}
int vnrAmdDebugRaySourceIndex(const uint32_t* counts, uint32_t n_in, uint32_t* src_out, uint32_t* alive_out)
{
  return guarded([&]() { debug_ray_source_index(counts, n_in, src_out, alive_out); });
}
int vnrAmdDebugEvalKernelResources(uint32_t F, uint32_t K_IN, uint32_t W, int general, int* regs, int* scratch_bytes, int* lds_bytes)
{
  return guarded([&]() { eval_kernel_resources(F, K_IN, W, general != 0, regs, scratch_bytes, lds_bytes); });
}
int vnrAmdRendererSetProfiling(vnrAmdRenderer r, int e) { return guarded([&]() { VNR_REN(r); r->r->set_profiling(e != 0); }); }
int vnrAmdRendererSetAsync(vnrAmdRenderer r, int e) { return guarded([&]() { VNR_REN(r); r->r->set_async(e != 0); }); }
int vnrAmdRendererSetInShaderKernel(vnrAmdRenderer r, int m) { return guarded([&]() { VNR_REN(r); r->r->set_in_shader_kernel(m); }); }
void vnrAmdReleaseRenderer(vnrAmdRenderer r) { delete r; }

// ------------------------------------------------------------------------------------------------ multi-GPU (dist.h)
int vnrAmdDistGetUniqueId(void* out128) { return guarded([&]() { if (!out128) throw std::runtime_error("null id buffer"); rccl_unique_id(out128); }); }
static void bind_device_to_local_rank(int local_rank)
{
  const int count = vnrAmdDeviceCount();
  if (count > 0) Runtime::get().init(local_rank % count);   // several ranks on one device: the host-staged transport's test set-up
}
int vnrAmdDistInit(int rank, int world, int local_rank, const void* unique_id, const char* transport, const char* address)
{
  return guarded([&]() {
    bind_device_to_local_rank(local_rank);
    Dist::get().init(rank, world, local_rank, unique_id, transport, address ? address : "");
  });
}
int vnrAmdDistInitFromEnv(void)
{
  return guarded([&]() {
    const char* lr = std::getenv("LOCAL_RANK");
    const char* r = std::getenv("RANK");
    bind_device_to_local_rank(lr && *lr ? std::atoi(lr) : (r && *r ? std::atoi(r) : 0));
    Dist::get().init_from_env();
  });
}
int vnrAmdDistFinalize(void) { return guarded([&]() { Dist::get().finalize(); }); }
int vnrAmdDistRank(void) { return Dist::get().rank(); }
int vnrAmdDistWorldSize(void) { return Dist::get().world(); }
const char* vnrAmdDistTransport(void) { return Dist::get().transport_name(); }
int vnrAmdDistRcclRanksSeen(void) { return Dist::get().rccl_ranks_seen(); }
int vnrAmdDistBarrier(void)
{
  return guarded([&]() {
    if (Runtime::get().ready()) VNR_HIP_CHECK(hipDeviceSynchronize());
    Dist::get().barrier();
  });
}
int vnrAmdDistAllReduceHost(double* values, int n, int op)
{
  return guarded([&]() {
    if (op < 0 || op > 3) throw std::runtime_error("unknown reduction");
    Dist::get().all_reduce_host(values, n, (DistOp)op);
  });
}
static hipStream_t dist_call_stream() { return Runtime::get().ready() ? Runtime::get().stream : nullptr; }
static void dist_call_done() { if (Runtime::get().ready()) VNR_HIP_CHECK(hipStreamSynchronize(Runtime::get().stream)); }
int vnrAmdDistAllReduce(void* buf, size_t count, int dtype, int op)
{
  return guarded([&]() {
    if (dtype < 0 || dtype > 2 || op < 0 || op > 3) throw std::runtime_error("unknown dtype / reduction");
    Dist::get().transport().all_reduce(buf, count, (DistDType)dtype, (DistOp)op, dist_call_stream());
    dist_call_done();
  });
}
int vnrAmdDistAllGather(const void* send, void* recv, size_t bytes_per_rank)
{
  return guarded([&]() { Dist::get().transport().all_gather(send, recv, bytes_per_rank, dist_call_stream()); dist_call_done(); });
}
int vnrAmdDistReduceScatter(void* buf, size_t count_per_rank, int dtype)
{
  return guarded([&]() {
    if (dtype < 0 || dtype > 2) throw std::runtime_error("unknown dtype");
    Dist::get().transport().reduce_scatter(buf, count_per_rank, (DistDType)dtype, DistOp::Sum, dist_call_stream());
    dist_call_done();
  });
}
int vnrAmdDistBroadcast(void* buf, size_t bytes, int root)
{
  return guarded([&]() { Dist::get().transport().broadcast(buf, bytes, root, dist_call_stream()); dist_call_done(); });
}
int vnrAmdDistSelfTest(double deadline_s, char* report, size_t report_size)
{
  return guarded([&]() {
    const std::string r = Dist::get().self_test(deadline_s > 0.0 ? deadline_s : 30.0);
    if (report && report_size) { std::strncpy(report, r.c_str(), report_size - 1); report[report_size - 1] = 0; }
  });
}
int vnrAmdRendererSetDistributed(vnrAmdRenderer r, int e) { return guarded([&]() { VNR_REN(r); r->r->set_distributed(e != 0); }); }
const float* vnrAmdRendererGatherFrame(vnrAmdRenderer r)
{
  const float* out = nullptr;
  guarded([&]() {
    VNR_REN(r);
    if (!r->r->distributed()) throw std::runtime_error("vnrAmdRendererGatherFrame: the renderer is not in distributed mode (vnrAmdRendererSetDistributed)");
    out = r->r->map_frame();
  });
  return out;
}
int vnrAmdRendererGetCompletedFrameStats(vnrAmdRenderer r, vnrAmdFrameStats* out)
{
  return guarded([&]() {
    VNR_REN(r);
    if (!out) throw std::runtime_error("null stats pointer");
    const FrameStats& s = r->r->completed_stats();
    out->n_samples = s.n_samples; out->n_reference_slots = s.n_reference_slots; out->n_iterations = s.n_iterations; out->n_rays_hit = s.n_rays_hit;
    out->infer_kernel_ms = s.infer_kernel_ms; out->infer_kernel_launches = s.infer_kernel_launches; out->infer_union_ms = s.infer_union_ms;
  });
}
int vnrAmdRendererRenderPipelined(vnrAmdRenderer r, const float** previous_frame)
{
  return guarded([&]() { VNR_REN(r); const float* f = r->r->render_pipelined(); if (previous_frame) *previous_frame = f; });
}
int vnrAmdRendererFlushPipeline(vnrAmdRenderer r, const float** last_frame)
{
  return guarded([&]() { VNR_REN(r); const float* f = r->r->flush_pipeline(); if (last_frame) *last_frame = f; });
}
int vnrAmdNeuralVolumeTrainDataParallel(vnrAmdVolume v, int steps, int fast_mode)
{
  return guarded([&]() { as_neural(v)->train_data_parallel((size_t)std::max(steps, 0), fast_mode != 0); });
}
int vnrAmdNeuralVolumeSetBrickImageMode(vnrAmdVolume v, int mode) { return guarded([&]() { as_neural(v)->network().brick_cache().set_mode(mode); }); }
int vnrAmdNeuralVolumeSetBrickImageBudget(vnrAmdVolume v, size_t bytes) { return guarded([&]() { as_neural(v)->network().brick_cache().set_budget(bytes); }); }
unsigned vnrAmdNeuralVolumeBrickImageLevels(vnrAmdVolume v)
{
  unsigned m = 0;
  guarded([&]() { m = as_neural(v)->network().brick_cache().levels_mask(); });
  return m;
}
int vnrAmdNeuralVolumeBrickImagePolicy(vnrAmdVolume v, uint64_t* builds, unsigned* launches_before_next_build, int* tier, uint64_t* small_builds)
{
  return guarded([&]() {
    const BrickCache& c = as_neural(v)->network().brick_cache();
    if (builds) *builds = c.policy().builds;
    if (launches_before_next_build) *launches_before_next_build = c.after_now();
    if (tier) *tier = c.policy().tier;
    if (small_builds) *small_builds = c.policy().small_builds;
  });
}
int vnrAmdNeuralVolumeGridBackwardPlan(vnrAmdVolume v, uint64_t batch, uint32_t out_u32[4], uint64_t out_u64[2])
{
  return guarded([&]() {
    const GridBackwardPlan p = as_neural(v)->network().grid_backward_plan((size_t)batch);
    if (out_u32) { out_u32[0] = p.n_levels; out_u32[1] = p.lds_levels; out_u32[2] = p.tile_entries; out_u32[3] = p.lds_blocks; }
    if (out_u64) { out_u64[0] = p.atomic_requests; out_u64[1] = p.flush_requests_at_most; }
  });
}
int vnrAmdNeuralVolumeSetDeterministicTraining(vnrAmdVolume v, int enable)
{
  return guarded([&]() { as_neural(v)->network().set_deterministic(enable != 0); });
}
int vnrAmdNeuralVolumeGetDeterministicTraining(vnrAmdVolume v, int* enabled)
{
  return guarded([&]() {
    const bool e = as_neural(v)->network().deterministic();
    if (enabled) *enabled = e ? 1 : 0;
  });
}
int vnrAmdNeuralVolumeSetTrainProfiling(vnrAmdVolume v, int e) { return guarded([&]() { as_neural(v)->network().set_train_profiling(e != 0); }); }
int vnrAmdNeuralVolumeGetTrainProfile(vnrAmdVolume v, double ms_per_step[5], int* n_steps)
{
  return guarded([&]() {
    const int n = as_neural(v)->network().train_profile(ms_per_step);
    if (n_steps) *n_steps = n;
  });
}
int vnrAmdNeuralVolumeSyncReplicas(vnrAmdVolume v) { return guarded([&]() { as_neural(v)->sync_replicas(); }); }
int vnrAmdNeuralVolumeAllReduceGradients(vnrAmdVolume v) { return guarded([&]() { as_neural(v)->all_reduce_gradients(); }); }
int vnrAmdNeuralVolumeTrainEndDataParallel(vnrAmdVolume v, int fast_mode, int sharded)
{
  return guarded([&]() { as_neural(v)->train_end_data_parallel(fast_mode != 0, sharded); });
}
int vnrAmdNeuralVolumeSetGradients(vnrAmdVolume v, const float* host, size_t count)
{
  return guarded([&]() {
    NeuralVolume* n = as_neural(v);
    n->network().set_grads_from_f32(host, count, n->stream);
    n->mark_external_gradient();
  });
}

// ------------------------------------------------------------------------------------------------ misc
void vnrAmdMemoryQuery(size_t* used_by_renderer, size_t* used_by_network)
{
  if (used_by_renderer) *used_by_renderer = Runtime::get().bytes_renderer;
  if (used_by_network) *used_by_network = Runtime::get().bytes_network;
}
void vnrAmdFreeTemporaryGPUMemory(void)
{
  guarded([&]() { Network::release_temporary_of_all(); });   // api.cpp:554-557
}

// ------------------------------------------------------------------------------------------------ building blocks
int vnrAmdSimpleVolumeTakeSamples(vnrAmdVolume v, size_t n, const float lower[3], const float upper[3], float* d_coords,
                                  float* d_values, void* stream)
{
  return guarded([&]() {
    as_simple(v)->take_samples(d_coords, d_values, n, {lower[0], lower[1], lower[2]}, {upper[0], upper[1], upper[2]}, resolve_stream(stream));
  });
}
int vnrAmdSimpleVolumeSetSamplingWeights(vnrAmdVolume v, const float* d_weights, float uniform_fraction, void* stream)
{
  return guarded([&]() {
    SimpleVolume::check_uniform_fraction(uniform_fraction);   // an argument check: before the handle, so that it needs no volume
    as_simple(v)->set_sampling_weights(d_weights, uniform_fraction, (hipStream_t)stream);
  });
}
int vnrAmdSimpleVolumeSamplingInfo(vnrAmdVolume v, int* active, uint64_t* n_cells, uint64_t* total, float* uniform_fraction)
{
  return guarded([&]() {
    const SimpleVolume* sv = as_simple(v);
    if (active) *active = sv->has_sampling_table() ? 1 : 0;
    if (n_cells) *n_cells = sv->sampling_cells();
    if (total) *total = sv->sampling_total();
    if (uniform_fraction) *uniform_fraction = sv->sampling_uniform_fraction();
  });
}
const uint64_t* vnrAmdSimpleVolumeSamplingCdf(vnrAmdVolume v)
{
  const uint64_t* p = nullptr;
  guarded([&]() { p = as_simple(v)->sampling_cdf(); });
  return p;
}
int vnrAmdSimpleVolumeTakeSamplesWeighted(vnrAmdVolume v, size_t n, float* d_coords, float* d_values, void* stream)
{
  return guarded([&]() { as_simple(v)->take_samples_weighted(d_coords, d_values, n, resolve_stream(stream)); });
}
int vnrAmdNeuralVolumeGuideSamplingByError(vnrAmdVolume v, float uniform_fraction, vnrAmdDecodeError* report)
{
  static_assert(sizeof(vnrAmdDecodeError) == sizeof(DecodeError), "vnrAmdDecodeError and DecodeError must agree");
  return guarded([&]() {
    SimpleVolume::check_uniform_fraction(uniform_fraction);
    as_neural(v)->guide_sampling_by_error(uniform_fraction, (DecodeError*)report);
  });
}
int vnrAmdSimpleVolumeTakeSamplesGrid(vnrAmdVolume v, const int origin[3], const int size[3], float* d_coords, float* d_values, void* stream)
{
  return guarded([&]() {
    SimpleVolume* sv = as_simple(v);
    const vec3i d = sv->dims();
    sv->take_samples_grid(d_coords, d_values, {origin[0], origin[1], origin[2]}, {size[0], size[1], size[2]},
                          {1.0f / (float)d.x, 1.0f / (float)d.y, 1.0f / (float)d.z}, resolve_stream(stream));
  });
}
int vnrAmdSimpleVolumeSample(vnrAmdVolume v, size_t n, const float* d_coords, float* d_values, int nodal, void* stream)
{
  return guarded([&]() { as_simple(v)->sample(d_coords, d_values, n, nodal != 0, resolve_stream(stream)); });
}
int vnrAmdNeuralVolumeUpdateMacrocell(vnrAmdVolume v, size_t n, const float* d_coords, const float* d_values, void* stream)
{
  return guarded([&]() { as_neural(v)->macrocell().update_explicit(d_coords, d_values, n, resolve_stream(stream)); });
}
int vnrAmdVolumeUpdateMaxOpacity(vnrAmdVolume v, vnrAmdTransferFunction t)
{
  return guarded([&]() {
    if (!v || !v->v) throw std::runtime_error("null volume");
    if (!t) throw std::runtime_error("null transfer function");
    v->v->set_transfer_function(t->d, Runtime::get().stream);
    VNR_HIP_CHECK(hipStreamSynchronize(Runtime::get().stream));
  });
}

}  // extern "C"
