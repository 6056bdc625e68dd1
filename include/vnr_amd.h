/* vnr_amd.h — C-ABI of the MI355X-native instantvnr hot path (libvnr_amd.so).
 *
 * This is the drop-in boundary: a C restatement of the reference's C++ API
 * (`/root/reference/api.h`, library target `instantvnr`).  Every entry point
 * cites the reference function it replaces.  The reference API passes
 * `std::shared_ptr` handles, `nlohmann::json` and gdt vectors; here handles are
 * opaque pointers (create / release), JSON documents cross as bytes (JSON text
 * or BSON, or a path to either — the reference accepts "a json that is a
 * string" as a path too: api.cpp:77-83,148-153,180-185), and vectors are plain
 * float/int arrays.  `include/vnr_api_shim.hpp` re-exposes the exact `api.h`
 * signatures on top of this header.
 *
 * Error convention: the reference throws std::runtime_error through the API
 * (api.cpp:129,138,215).  Here every function that can fail returns
 * VNR_AMD_OK / an error code (or NULL for constructors) and leaves a message
 * in vnrAmdGetLastError(); the shim turns that back into std::runtime_error.
 *
 * Threading: like the reference, not thread-safe; drive all calls of one
 * process from one thread (int_dual_volume.cpp:498-720).  One process per GPU.
 *
 * All `d_` pointers are device pointers on the current HIP device.  `stream`
 * arguments are `hipStream_t` passed as void* (NULL = the library's stream).
 */
#ifndef VNR_AMD_H
#define VNR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VNR_AMD_OK 0
#define VNR_AMD_ERROR 1

typedef struct vnrAmdVolume_t*           vnrAmdVolume;           /* api.h:28  vnrVolume   */
typedef struct vnrAmdRenderer_t*         vnrAmdRenderer;         /* api.h:29  vnrRenderer */
typedef struct vnrAmdTransferFunction_t* vnrAmdTransferFunction; /* api.h:31 */
typedef struct vnrAmdCamera_t*           vnrAmdCamera;           /* api.h:32 */

/* api.h:36-60 vnrRenderMode (same numeric values) */
enum {
  VNR_AMD_OPTIX_NO_SHADING = 0,
  VNR_AMD_RAYMARCHING_NO_SHADING_DECODING = 4,
  VNR_AMD_RAYMARCHING_NO_SHADING_SAMPLE_STREAMING = 5,
  VNR_AMD_RAYMARCHING_NO_SHADING_IN_SHADER = 6,
  VNR_AMD_RAYMARCHING_GRADIENT_SHADING_SAMPLE_STREAMING = 8,
  VNR_AMD_RAYMARCHING_SINGLE_SHADE_HEURISTIC_SAMPLE_STREAMING = 11,
  VNR_AMD_PATHTRACING_SAMPLE_STREAMING = 14,
  VNR_AMD_INVALID = 16
};

/* core/mathdef.h:51-65 ValueType (same numeric values) */
enum {
  VNR_AMD_TYPE_UINT8 = 0, VNR_AMD_TYPE_INT8, VNR_AMD_TYPE_UINT16, VNR_AMD_TYPE_INT16,
  VNR_AMD_TYPE_UINT32, VNR_AMD_TYPE_INT32, VNR_AMD_TYPE_UINT64, VNR_AMD_TYPE_INT64,
  VNR_AMD_TYPE_FLOAT, VNR_AMD_TYPE_FLOAT2, VNR_AMD_TYPE_FLOAT3, VNR_AMD_TYPE_FLOAT4, VNR_AMD_TYPE_DOUBLE
};

/* how a JSON document argument is encoded */
enum {
  VNR_AMD_JSON_TEXT = 0,      /* UTF-8 JSON text, // comments allowed (api.cpp:17-21) */
  VNR_AMD_JSON_BSON = 1,      /* BSON bytes (api.cpp:23-32) */
  VNR_AMD_JSON_TEXT_FILE = 2, /* data = path of a JSON text file */
  VNR_AMD_JSON_BSON_FILE = 3  /* data = path of a BSON file ("params.json") */
};

/* ---- library ----------------------------------------------------------- */
const char* vnrAmdGetLastError(void);
const char* vnrAmdVersion(void);
/* the build: first 12 hex digits of the md5 over every source file of the library, stamped at link time (csrc/Makefile) */
const char* vnrAmdBuildId(void);
/* selects the HIP device (reference: env VNR_CUDA_DEVICE, renderer.cpp:299-304); -1 = env VNR_AMD_DEVICE or 0 */
int  vnrAmdInit(int device);
int  vnrAmdDeviceCount(void);
/* returns 1 when libvnr_amd's HIP kernels are usable (a gfx950 device is present) */
int  vnrAmdHasDevice(void);

/* plain device-memory helpers so that hosts without a HIP binding (ctypes, cgo, JNI) can drive the API */
void* vnrAmdMalloc(size_t bytes);
int   vnrAmdFree(void* d_ptr);
int   vnrAmdMemcpyH2D(void* d_dst, const void* h_src, size_t bytes);
int   vnrAmdMemcpyD2H(void* h_dst, const void* d_src, size_t bytes);
int   vnrAmdMemset(void* d_dst, int value, size_t bytes);
int   vnrAmdSynchronize(void);
void* vnrAmdDefaultStream(void);

/* ---- JSON (api.h:90-96) -------------------------------------------------- */
/* Converts between JSON text and BSON; *out is malloc'ed, free with vnrAmdFreeHost.
 * Replaces vnrCreateJsonText/Binary, vnrLoadJsonText/Binary, vnrSaveJsonText/Binary. */
int  vnrAmdJsonConvert(const void* data, size_t size, int format_in, int format_out /* TEXT or BSON */,
                       void** out, size_t* out_size);
int  vnrAmdJsonSave(const void* data, size_t size, int format_in, const char* filename, int format_out);
void vnrAmdFreeHost(void* p);

/* ---- camera (api.h:103-110) --------------------------------------------- */
vnrAmdCamera vnrAmdCreateCamera(void);                                              /* vnrCreateCamera() */
int  vnrAmdCameraSet(vnrAmdCamera, const float from[3], const float at[3], const float up[3]); /* vnrCameraSet */
/* vnrCreateCamera(scene) / vnrCameraSet(self, scene) (api.h:104,106; serializer.cpp:178-187, 418-428): eye / center / up / fovy
 * of view.camera, eye and center moved by -dims/2.  A DIVA scene leaves the camera as it is (the reference's TODO). */
int  vnrAmdCameraSetFromScene(vnrAmdCamera, const void* scene, size_t size, int format);
int  vnrAmdCameraSetFovy(vnrAmdCamera, float fovy_degrees);                          /* Camera::fovy, instantvnr_types.h:82 */
int  vnrAmdCameraGet(vnrAmdCamera, float from[3], float at[3], float up[3], float* fovy); /* vnrCameraGetPosition/Focus/UpVec */
void vnrAmdReleaseCamera(vnrAmdCamera);

/* ---- transfer function (api.h:154-162) ----------------------------------- */
vnrAmdTransferFunction vnrAmdCreateTransferFunction(void);                           /* vnrCreateTransferFunction() */
int  vnrAmdTransferFunctionSetColor(vnrAmdTransferFunction, const float* rgb, int n);  /* ...SetColor: n x vec3f */
int  vnrAmdTransferFunctionSetAlpha(vnrAmdTransferFunction, const float* xy, int n);   /* ...SetAlpha: n x vec2f (x = position, y = alpha) */
int  vnrAmdTransferFunctionSetValueRange(vnrAmdTransferFunction, float lo, float hi); /* ...SetValueRange */
int  vnrAmdTransferFunctionGetSizes(vnrAmdTransferFunction, int* n_colors, int* n_alphas);
int  vnrAmdTransferFunctionGet(vnrAmdTransferFunction, float* rgb, float* xy, float range[2]);
void vnrAmdReleaseTransferFunction(vnrAmdTransferFunction);

/* ---- simple (ground-truth) volume (api.h:117-119) ------------------------- */
/* vnrCreateSimpleVolume(scene, "GPU"): the volume is min/max-normalised to [0,1] fp32 on load
 * (neural_sampler.cpp:223-288) and its macrocell is built (sampler.cu:5-17, macrocell.cu:221-234).
 * range_lo > range_hi means "compute min/max from the data". */
vnrAmdVolume vnrAmdCreateSimpleVolumeFromMemory(const void* host_data, const int dims[3], int value_type,
                                                float range_lo, float range_hi);
vnrAmdVolume vnrAmdCreateSimpleVolumeFromRawFile(const char* filename, const int dims[3], int value_type,
                                                 size_t offset, int big_endian, float range_lo, float range_hi);
/* seeded synthetic volume generated on the GPU (4-octave Perlin fBm, BASELINE C4/C5 stand-in) */
vnrAmdVolume vnrAmdCreateSimpleVolumePerlin(const int dims[3], uint32_t seed, int octaves, float base_frequency);
/* device pointer to the normalised fp32 voxels, x fastest */
const float* vnrAmdSimpleVolumeDeviceData(vnrAmdVolume);
/* vnrCreateSimpleVolume(scene, "OUT_OF_CORE") (api.cpp:145-158 -> neural_sampler.cpp:1224-1227, 1043-1064): the volume stays
 * in its file; a random set of n_blocks slabs is resident in HBM and n_concurrent_blocks of them are replaced per
 * training step (RandomBuffer, neural_sampler.cpp:477-668).  0 for a count = the reference's default, i.e. the
 * environment variables VNR_NUM_CONCURRENT_BLOCKS (1024) / VNR_NUM_BLOCKS (64 x) (neural_sampler.cpp:1054-1062).
 * A value range is required (range_lo < range_hi; :1069-1071).  Such a volume has no ground-truth macrocell and cannot
 * be rendered itself; it feeds vnrAmdCreateNeuralVolume, whose grid is min(1024, dims) per axis. */
vnrAmdVolume vnrAmdCreateSimpleVolumeOutOfCore(const char* filename, const int dims[3], int value_type, size_t offset,
                                               float range_lo, float range_hi, uint64_t n_concurrent_blocks, uint64_t n_blocks);
/* vnrCreateSimpleVolume(scene, mode, save_loaded_volume) (api.h:117, api.cpp:145-158): `scene` is a VIDI3D or DIVA scene
 * document (serializer.cpp:137-176, 394-447) in any of the VNR_AMD_JSON_* formats; a document that is a JSON string is the
 * path of a JSON text file.  mode: "GPU" (resident, every time step in HBM), "OUT_OF_CORE", "NOTHING" (shape only);
 * "VIRTUAL_MEMORY" and "OPENVKL*" are not implemented and fail; anything else fails with "unknown mode" like the reference.
 * save_loaded_volume writes the normalised fp32 voxels to ./reference.bin (neural_sampler.cu:101-108). */
vnrAmdVolume vnrAmdCreateSimpleVolumeFromScene(const void* scene, size_t size, int format, const char* mode, int save_loaded_volume);
int  vnrAmdSimpleVolumeGetNumberOfTimeSteps(vnrAmdVolume);            /* vnrSimpleVolumeGetNumberOfTimeSteps (api.h:119) */
int  vnrAmdSimpleVolumeSetCurrentTimeStep(vnrAmdVolume, int index);   /* vnrSimpleVolumeSetCurrentTimeStep (api.h:118) */
/* AMD extension: in-situ ground truth.  The voxels are in device memory already (a simulation's output, another kernel's result,
 * the next step of a time series): they are normalised on the GPU with the arithmetic of the host path, so the volume equals
 * vnrAmdCreateSimpleVolumeFromMemory of the same array bit for bit (voxels, data range, macrocell).
 *   d_data      typed voxels, x fastest, aligned to the value type: VNR_AMD_TYPE_UINT8 / INT8 / UINT16 / INT16 / UINT32 / INT32 /
 *               FLOAT / DOUBLE.  The 64-bit integer and the vector types are refused.  It is a pointer of the HIP runtime the
 *               library runs on: vnrAmdMalloc, or the application's own hipMalloc against the same libamdhip64.  A PyTorch tensor
 *               is not one: the PyTorch wheel's bundled second ROCm runtime cannot share the device with the library's
 *               (INTEGRATION.md §4), unless torch was imported first and the library bound to torch's runtime.
 *   strides     three element strides (sx, sy, sz), all positive, for a field with ghost layers or a sub-box of a larger array
 *               (d_data points at the first voxel of the box); NULL = dense.  sx == 1 is read 16 bytes per lane, any other sx
 *               voxel by voxel.
 *   range       range_lo > range_hi = min / max of the data (the source is then read twice, otherwise once); used_range (may be
 *               NULL) receives the range that was applied.
 *   stream      the hipStream_t the caller produced d_data on; NULL = the data is complete.  The library records an event on it and
 *               makes its own stream wait for that event; the caller's stream is never blocked or synchronised.
 * Every call returns after the ingest and the macrocell pass have completed, like the other load paths: on return the caller may
 * overwrite or free d_data.  The volume never keeps a pointer to d_data, and d_data must not overlap the volume's own voxels.
 * Errors (NULL / VNR_AMD_ERROR / -1 and a message): null data, non-positive dims, a stride <= 0, a refused value type, an
 * out-of-core or "NOTHING" volume, a neural volume, a volume whose dims are not the ones it was created with, no usable device.
 * A refused call leaves the volume as it was.
 *
 * Create: as vnrAmdCreateSimpleVolumeFromMemory (dims, transform, clip box, macrocell, data range).
 * Update: replaces the voxels of the current time step in place: same dims, vnrAmdSimpleVolumeDeviceData keeps its value.  Then
 *   the volume's macrocell is rebuilt from the new voxels alone -- it equals a fresh volume's; vnrAmdSimpleVolumeSetCurrentTimeStep
 *   only widens the cells by the step it switches to -- and, if a transfer function is set, its max opacity.  The data range becomes the new step's on a one-step volume and is extended by it otherwise.  A neural volume created
 *   on this volume goes on training from the new voxels with its current parameters and optimizer state (a warm start).  Its own
 *   online macrocell is NOT reset, exactly as at a time-step switch: it still bounds the earlier data as well, which is
 *   conservative where values left a cell and keeps tightening only through training samples; a neural volume that shares the
 *   ground truth's macrocell (online_macrocell_construction = 0) sees the recomputed one at once.  A renderer with pipelined or
 *   asynchronous frames in flight (vnrAmdRendererRenderPipelined, vnrAmdRendererSetAsync) must be flushed before the call, as
 *   before a time-step switch: frames in flight read the voxels that are being replaced.
 * Append: adds a time step (vnrAmdSimpleVolumeGetNumberOfTimeSteps / ...SetCurrentTimeStep then work on volumes built without
 *   scene files); the current step stays current; the data range is extended as by a scene's further steps.  Returns the new
 *   step's index, -1 on error. */
vnrAmdVolume vnrAmdCreateSimpleVolumeFromDevice(const void* d_data, const int dims[3], int value_type, const int64_t strides[3],
                                                float range_lo, float range_hi, void* stream, float used_range[2]);
int  vnrAmdSimpleVolumeUpdateFromDevice(vnrAmdVolume, const void* d_data, int value_type, const int64_t strides[3],
                                        float range_lo, float range_hi, void* stream, float used_range[2]);
int  vnrAmdSimpleVolumeAppendTimeStepFromDevice(vnrAmdVolume, const void* d_data, int value_type, const int64_t strides[3],
                                                float range_lo, float range_hi, void* stream, float used_range[2]);
/* the value range a scene maps its transfer function to (view.volume.scalarMappingRange[Unnormalized], serializer.cpp:212-256);
 * returns 2 and leaves `range` untouched when the scene has none (VNR_AMD_OK when it has, VNR_AMD_ERROR on a malformed scene) */
int  vnrAmdSceneGetValueRange(const void* scene, size_t size, int format, float range[2]);
typedef struct vnrAmdOutOfCoreInfo {
  int file_dims[3];            /* dims of the volume in the file */
  int block_dims[3];           /* slab proper: x-full, rows, 1 slice (RandomBuffer ctor :531-546) */
  int block_index_space[3];
  uint64_t n_blocks, n_concurrent_blocks, block_size_aligned, bytes_read;
} vnrAmdOutOfCoreInfo;
int  vnrAmdSimpleVolumeOutOfCoreInfo(vnrAmdVolume, vnrAmdOutOfCoreInfo*);
/* AMD extension: asynchronous refresh.  The reference's schedule (and the default here) replaces n_concurrent_blocks slabs per training
 * step and the step waits for them: at the default 1024 slabs that is 102 MiB of reads and PCIe per step, 3 ms against a 0.65 ms step.
 * With asynchronous refresh (also VNR_AMD_OOC_ASYNC=1) a step never waits: while a refresh is in flight batches are drawn from the slabs
 * that are not being replaced, and the next refresh starts as soon as the previous one has arrived, so slabs turn over at the rate the
 * storage delivers them.  Same slab geometry, slab choice and per-sample arithmetic; RefreshStats says how many refreshes were submitted
 * and how many steps ran beside one. */
int  vnrAmdSimpleVolumeOutOfCoreSetAsyncRefresh(vnrAmdVolume, int enable);
int  vnrAmdSimpleVolumeOutOfCoreRefreshStats(vnrAmdVolume, uint64_t* refreshes, uint64_t* steps_without_refresh);
/* the slot table the next TakeSamples call will sample from: block index (y, z) per slot, 2 ints each (AMD extension, tests) */
int  vnrAmdSimpleVolumeOutOfCoreBlocks(vnrAmdVolume, int* block_index_yz, size_t n_slots);

/* ---- neural volume (api.h:122-143) ---------------------------------------- */
/* vnrCreateNeuralVolume(config, groundtruth, online_macrocell_construction) api.cpp:174-188 */
vnrAmdVolume vnrAmdCreateNeuralVolume(const void* config, size_t size, int format, vnrAmdVolume groundtruth,
                                      int online_macrocell_construction);
/* vnrCreateNeuralVolume(config, dims) api.cpp:190-204 */
vnrAmdVolume vnrAmdCreateNeuralVolumeFromDims(const void* config, size_t size, int format, const int dims[3]);
/* vnrCreateNeuralVolume(params) api.cpp:206-220 — params.json (BSON) with volume.dims + model + parameters */
vnrAmdVolume vnrAmdCreateNeuralVolumeFromParams(const void* params, size_t size, int format);

int    vnrAmdNeuralVolumeSetModel(vnrAmdVolume, const void* config, size_t size, int format);  /* vnrNeuralVolumeSetModel */
int    vnrAmdNeuralVolumeSetParams(vnrAmdVolume, const void* params, size_t size, int format); /* vnrNeuralVolumeSetParams */
double vnrAmdNeuralVolumeGetPSNR(vnrAmdVolume, int verbose);                                   /* vnrNeuralVolumeGetPSNR */
/* vnrNeuralVolumeGetSSIM (api.h:130 -> network.cu:474-549 get_mssim): mean SSIM of the network against the reference volume at the
 * voxel centres, 7^3 uniform windows, sample covariance, K1 .01, K2 .03, data range 1; -1 on error */
double vnrAmdNeuralVolumeGetSSIM(vnrAmdVolume, int verbose);
double vnrAmdNeuralVolumeGetTestingLoss(vnrAmdVolume);                                         /* vnrNeuralVolumeGetTestingLoss */
double vnrAmdNeuralVolumeGetTrainingLoss(vnrAmdVolume);                                        /* vnrNeuralVolumeGetTrainingLoss */
int    vnrAmdNeuralVolumeGetTrainingStep(vnrAmdVolume);                                        /* vnrNeuralVolumeGetTrainingStep */
int    vnrAmdNeuralVolumeGetNumberOfBlobs(vnrAmdVolume);                                       /* vnrNeuralVolumeGetNumberOfBlobs */
int    vnrAmdNeuralVolumeTrain(vnrAmdVolume, int steps, int fast_mode);                        /* vnrNeuralVolumeTrain */
/* vnrNeuralVolumeSerializeParams(vol, filename): BSON params.json (network.cu:859-877) */
/* vnrNeuralVolumeDecodeProgressive (api.h:137, api.cpp:228-232 -> network.cu:290-326): decodes the next blob of 16 z-slices at the
 * voxel centres into the dense decoded volume that rendering modes 4 / 7 march; GetNumberOfBlobs calls = one full pass */
int    vnrAmdNeuralVolumeDecodeProgressive(vnrAmdVolume);
/* vnrNeuralVolumeDecodeInference / ...DecodeReference (api.h:139-140, api.cpp:234-244 -> network.cu:328-405): raw fp32 dump of the
 * decoded / reference volume, slice by slice, each slice padded to a multiple of 256 values.  The reference ignores the
 * file name of DecodeReference and writes "reference.bin"; this writes `filename`. */
int    vnrAmdNeuralVolumeDecodeInference(vnrAmdVolume, const char* filename);
int    vnrAmdNeuralVolumeDecodeReference(vnrAmdVolume, const char* filename);
const float* vnrAmdNeuralVolumeDecodedDeviceData(vnrAmdVolume);   /* AMD extension: the decoded volume (NULL before the first decode) */
int    vnrAmdNeuralVolumeSerializeParamsToFile(vnrAmdVolume, const char* filename);
/* vnrNeuralVolumeSerializeParams(vol, json&): BSON bytes, free with vnrAmdFreeHost */
int    vnrAmdNeuralVolumeSerializeParams(vnrAmdVolume, void** bson, size_t* size);

/* NeuralVolume::inference (core/network.cu:1043-1052): n coords [n][3] fp32 -> n fp32 values.
 * Buffers need not be padded (the reference pads n to 256 and reads/writes the pad). */
int    vnrAmdNeuralVolumeInference(vnrAmdVolume, size_t n, const float* d_coords, float* d_values, void* stream);
/* AMD extension: in-situ round trip, the other half of the in-situ ground truth above.  A trained neural volume is decoded into
 * the application's own typed device array, and the error of exactly those voxels against a field in device memory is reported,
 * both without a host round trip and without a full-size intermediate buffer.
 *   grid_dims   the virtual voxel grid the box indexes; NULL = the volume's dims.  Any positive dims: a finer grid super-samples,
 *               a coarser one is a preview.  (ErrorAgainstDevice always works on the volume's own grid.)
 *   box         box_lo / box_size, a box inside that grid; NULL / NULL = the whole grid.  Voxel (i, j, k) of the box is the
 *               network's value at ((float)(box_lo + ijk) + 0.5f) * (1.0f / (float)grid_dims) per axis, in fp32: the coordinates
 *               vnrAmdNeuralVolumeDecodeProgressive uses.  A VNR_AMD_TYPE_FLOAT decode without a range therefore equals
 *               vnrAmdNeuralVolumeInference at these coordinates bit for bit, and on the volume's own grid the decoded volume.
 *   d_out/d_ref points at the first voxel of the box in the array; value types, alignment, runtime and `strides` (elements, all
 *               positive, NULL = dense over box_size) as for d_data above.  Strides that would put two voxels of the box at one
 *               address are refused: ordered by stride, each axis longer than one voxel must step at least over the extent of
 *               the axes below it.  Where the runtime knows the allocation the pointer lies in, a box that does not fit is refused.
 *   range       the conversion of the network's output v (which is NOT clamped to [0, 1] first) to the stored voxel, step by step:
 *                 d = __fadd_rn(__fmul_rn(v, range_hi - range_lo), range_lo)   two fp32 roundings, never one fma; the width in fp32
 *                 range_lo > range_hi: d = v (FLOAT / DOUBLE only; the integer types need a range); range_lo == range_hi is refused
 *                 FLOAT stores d, DOUBLE (double)d, an integer type rint((double)d) (ties to even) saturated to the type's limits,
 *                 a NaN as 0.
 *               vnrAmdSimpleVolumeGetDataRange of the ground truth is the range that inverts the ingest.
 *   stream      the hipStream_t of the caller that may still be reading d_out's previous content / that produced d_ref; NULL =
 *               none.  The library records an event on it and makes its own stream wait; the caller's stream is never blocked or
 *               synchronised.  Both calls return after their work has completed.
 * The work runs in chunks of VNR_AMD_DECODE_CHUNK samples (read at every call; default 4194304, at most 2^28) through scratch the
 * volume keeps: 16 bytes per sample of the largest chunk so far.  The result does not depend on the chunk size.  With sx == 1 the
 * array is accessed 16 bytes per lane, cut at the 16-byte boundaries of its address, ragged row ends element by element; any
 * other sx goes voxel by voxel.  Nothing but the box's voxels is written: ghost layers keep their bytes.  A dense FLOAT decode
 * without a range is written by the evaluation kernel itself.
 *
 * ErrorAgainstDevice: per voxel e = (double)decoded - (double)ref, where decoded is the typed value DecodeToDevice would store for
 * this value type and range (quantisation included).  n_voxels = voxels of the box; max_abs = max |e| and worst = the grid index
 * of the voxel that has it (the lowest x-fastest index among equals), both exact; sum_abs, sum_sq = sums of |e| and e * e in
 * double (their last bits depend on the chunk size); psnr_db = 10 log10((range_hi - range_lo)^2 * n_voxels / sum_sq), the range
 * taken as 1 when none is given.  d_block_max (may be NULL): a float per macrocell, dims and order of vnrAmdVolumeGetMacrocell
 * (16^3 voxels, x fastest): max |e| of the cell's voxels inside the box rounded to float, 0 where the box has none.
 * NaN: the integer types never decode to one.  For FLOAT / DOUBLE a voxel where decoded or ref is a NaN makes sum_abs, sum_sq and
 * psnr_db NaN -- that is how the caller learns of it -- while max_abs, worst and the block map are those of the other voxels
 * (max_abs NaN and worst -1, -1, -1 if there is no other voxel).
 *
 * Errors (VNR_AMD_ERROR and a message; nothing has been written, the volume is as it was): a null pointer, a simple volume, a
 * neural volume without a valid network, non-positive grid dims or box sizes, a box outside the grid, box_lo without box_size,
 * a stride <= 0, overlapping strides, a refused value type, an integer type without a range, range_lo == range_hi, a pointer not
 * aligned to its type, a box beyond its allocation, a malformed VNR_AMD_DECODE_CHUNK, no usable device. */
typedef struct vnrAmdDecodeError { uint64_t n_voxels; double max_abs; int worst[3]; double sum_abs, sum_sq, psnr_db; } vnrAmdDecodeError;
int    vnrAmdNeuralVolumeDecodeToDevice(vnrAmdVolume neural, void* d_out, int value_type, const int64_t strides[3],
                                        const int box_lo[3], const int box_size[3], const int grid_dims[3],
                                        float range_lo, float range_hi, void* stream);
int    vnrAmdNeuralVolumeErrorAgainstDevice(vnrAmdVolume neural, const void* d_ref, int value_type, const int64_t strides[3],
                                            const int box_lo[3], const int box_size[3], float range_lo, float range_hi,
                                            void* stream, vnrAmdDecodeError* out, float* d_block_max);
/* AMD extension: error-bounded round trip.  BuildCorrection stores what the network missed: quantised residuals for exactly the
 * macrocells (16^3, the grid of vnrAmdVolumeGetMacrocell, ragged at the upper faces) in which some voxel of the whole-grid decode
 * misses the tolerance eps against the field d_ref; DecodeToDeviceCorrected decodes with that applied.  The pair (params.json,
 * serialised correction) is the compressed field.  The build's box is always the whole grid of the volume, DecodeToDeviceCorrected's
 * too; DecodeBoxToDeviceCorrected ("corrected decode of a box" below) takes any box of it.  Pointer, strides, alignment,
 * allocation room, stream and value range are those of DecodeToDevice, with its refusals and messages.
 *
 * Per voxel, dec is the typed value DecodeToDevice stores for this value type and range, ref the voxel of d_ref, eps a finite
 * double >= 0 in data units.  Every step is an integer operation or one IEEE double operation:
 *   kind 0, the integer types:  E = floor(min(eps, 2^40)) (no voxel of a 32-bit type can miss 2^32), s = 2 E + 1,
 *       r = (int64)ref - (int64)dec, q = floor_div(r + E, s), corrected = clamp(dec + q s, Tmin, Tmax) in int64.
 *       |corrected - ref| <= E <= eps for every voxel, and q == 0 exactly where |r| <= E.
 *   kind 1, FLOAT / DOUBLE with eps > 0:  s = 2 eps in double, r = (double)ref - (double)dec, q = rint(r / s) (one division, ties
 *       to even), corrected = (T)__dadd_rn((double)dec, __dmul_rn((double)q, s)), never an fma; a voxel with q == 0 keeps dec bit
 *       for bit.  A voxel whose r is a NaN (a NaN in ref or dec, two infinities of one sign) gets q = 0, is counted in n_nan and
 *       stays as decoded.  |corrected - ref| <= eps + 2^-50 (|ref| + |dec| + eps) + ulp_T(corrected) / 2: the roundings of r, r / s
 *       and q s can put a voxel a few last bits over eps itself, which is why max_abs_after is reported exactly.
 *   kind 2, FLOAT / DOUBLE with eps == 0, verbatim:  a voxel differs where the bit patterns of dec and ref differ; the code of
 *       every voxel of a flagged cell is ref's bit pattern and corrected = ref bit for bit, NaN payloads and -0.0 included.
 * A cell is flagged iff some voxel in it has q != 0 (kind 2: differs).  With m = max |q| over the cell its codes are 1 byte wide
 * if m <= 127, 2 if m <= 32767, 4 otherwise, little-endian signed (kind 2: sizeof(T)); m > 2^31 - 1 in any cell refuses the build.
 * The codes of a flagged cell cover all its voxels (0 within tolerance) in the order lx + cx (ly + cy lz), cx = min(16, dims.x -
 * 16 ix) and likewise cy, cz; each cell's codes are padded with zero bytes to a multiple of 16 bytes; cells in ascending index.
 *
 * Serialised form, little-endian: a header of 104 bytes, n_flagged entries {uint32 cell, uint32 width}, the payload.  Header:
 *   char[8] "VNRCORR1" | uint32 version = 1 | uint32 value_type | int32 dims[3] | uint32 n_flagged | double eps | float range_lo,
 *   range_hi | uint32 kind | uint32 reserved = 0 | uint64 step (kind 0: s; kind 1: the bits of the double s; kind 2: 0) |
 *   uint64 params_hash | uint64 n_params | uint64 payload_bytes | double max_abs_after | uint64 reserved = 0
 * params_hash: FNV-1a 64 of the bytes vnrAmdNeuralVolumeGetParamsFP16 returns at build time.  CreateCorrectionFromBytes is host
 * code (no device needed; the device copy is made at the first apply) and refuses, by name, anything but a well-formed blob:
 * magic, version, value type, positive dims, n_flagged <= cells, cells strictly ascending and in range, a width legal for kind
 * and type, kind / step / eps consistent, reserved fields zero, payload_bytes = the sum of the padded cell sizes, the exact size.
 *
 * Info: n_voxels_flagged = voxels with q != 0 (kind 2: that differ); max_abs_before / max_abs_after = max |(double)dec - (double)
 * ref| and max |(double)corrected - (double)ref| over all voxels, exact (NaN differences aside; NaN if there is no other voxel);
 * worst_after = the voxel of max_abs_after, the lowest x-fastest index among equals.  A correction loaded from bytes reports
 * max_abs_before = NaN, worst_after = -1, -1, -1, n_nan = n_voxels_flagged = 0 and max_abs_after from the header.
 * The build evaluates the network twice, chunk by chunk (VNR_AMD_DECODE_CHUNK, as above; the result does not depend on it), and
 * keeps no full-size intermediate.  The apply writes nothing but the volume's voxels: ghost layers keep their bytes.
 * verify_params != 0 hashes the volume's current parameters and refuses when hash or count differ from the correction's; with 0
 * the caller vouches that the parameters are the ones the correction was built on.
 *
 * Errors (NULL / VNR_AMD_ERROR and a message; nothing has been written): those of DecodeToDevice; eps negative, NaN or infinite;
 * a cell that needs codes wider than 32 bits; a correction whose dims differ from the volume's; a null handle; malformed bytes. */
typedef struct vnrAmdCorrection_t* vnrAmdCorrection;
typedef struct vnrAmdCorrectionInfo {
  int dims[3], value_type, kind; double eps; float range_lo, range_hi;
  uint64_t n_cells, n_flagged, n_voxels_flagged, payload_bytes, serialized_bytes, n_nan, params_hash, n_params;
  double max_abs_before, max_abs_after; int worst_after[3]; } vnrAmdCorrectionInfo;
vnrAmdCorrection vnrAmdNeuralVolumeBuildCorrection(vnrAmdVolume neural, const void* d_ref, int value_type, const int64_t strides[3],
                                                   float range_lo, float range_hi, double eps, void* stream);
int  vnrAmdCorrectionGetInfo(vnrAmdCorrection, vnrAmdCorrectionInfo*);
int  vnrAmdCorrectionSerialize(vnrAmdCorrection, void** bytes, size_t* size);          /* vnrAmdFreeHost */
vnrAmdCorrection vnrAmdCreateCorrectionFromBytes(const void* bytes, size_t size);      /* host only; uploaded at first use */
int  vnrAmdNeuralVolumeDecodeToDeviceCorrected(vnrAmdVolume neural, vnrAmdCorrection, void* d_out, const int64_t strides[3],
                                               void* stream, int verify_params);
void vnrAmdReleaseCorrection(vnrAmdCorrection);
/* AMD extension: packed corrections.  A second serialised form of the same correction, with a bit width per group of 64 codes and
 * the codes stored as bit planes; "VNRCORR1" above and everything that reads or writes it is unchanged, and either form gives the
 * other byte for byte.  Little-endian: the 104-byte header above with magic "VNRCORP1", version 1 and payload_bytes the size of the
 * packed payload (every other field as above, with its rules); the same n_flagged entries {uint32 cell, uint32 width}, width being
 * the code width of the cell in the fixed-width form; then the packed payload.
 * The codes of a flagged cell are its codes above in their order, lx + cx (ly + cy lz), cut into groups of 64 consecutive codes;
 * the last group of a cell is filled up with codes of value 0: ceil(voxels / 64) groups a cell, at most 64.  A code becomes an
 * unsigned z of up to 64 bits: kinds 0 and 1 z = (q << 1) ^ (q >> 63) of the sign-extended code q, kind 2 the stored bit pattern,
 * zero-extended.  nbits of a group is the bit length of its largest z, 0 to 64.  The packed payload is
 *   1. the group table: one byte nbits per group, all groups of all flagged cells in cell order, zero bytes up to a multiple of 8;
 *   2. the planes: group after group in that order, nbits words of uint64; bit l of word b (b = 0 the least significant plane) is
 *      bit b of the z of the group's code l.
 * payload_bytes = pad8(n_groups) + 8 * the sum of nbits.  A group of zeros costs its table byte.
 *
 * SerializePacked packs on the device, from the resident fixed-width payload (uploaded first if the correction came from bytes), on
 * the library's stream, and has synchronised when it returns; one wavefront takes one group, a plane is one ballot.  The result is
 * cached (a correction never changes); a correction read from packed bytes returns those bytes without touching the device.
 * CreateCorrectionFromPackedBytes is host code like CreateCorrectionFromBytes: the packed payload is uploaded as it is and unpacked
 * on the device by the first apply, and on the host by the first Serialize or GetInfo.  It refuses, with "malformed packed
 * correction bytes: <rule>", everything CreateCorrectionFromBytes refuses in header and entries, and: an nbits above 8 * width, a
 * group whose top plane is zero while nbits > 0 (the form is canonical), a set bit in a lane beyond the cell's voxels, nonzero table
 * padding, a size that differs from header + entries + payload_bytes, payload_bytes that differ from what the table gives.
 * Errors: a null handle, null arguments, malformed bytes; SerializePacked of a correction not read from packed bytes needs a device. */
int  vnrAmdCorrectionSerializePacked(vnrAmdCorrection, void** bytes, size_t* size);    /* vnrAmdFreeHost */
vnrAmdCorrection vnrAmdCreateCorrectionFromPackedBytes(const void* bytes, size_t size); /* host only; unpacked at first use */
/* AMD extension: corrected decode of a box, and the resident form of a correction.
 *
 * DecodeBoxToDeviceCorrected is DecodeToDeviceCorrected for a box of the volume's own grid (a correction exists at its voxel
 * centres only, so there is no grid_dims): box_lo / box_size as in DecodeToDevice, NULL / NULL = the whole grid, which stores what
 * DecodeToDeviceCorrected stores.  d_out points at the first voxel of the box, strides are in elements, NULL = dense over
 * box_size; layout, alignment, allocation room, overlap and stream rules, refusals and messages are DecodeToDevice's; value type
 * and range are the correction's.  Only the box's voxels are evaluated by the network and only they are written; a voxel's cell
 * and its index in the cell are those of its grid coordinate box_lo + ijk, so a box stores exactly the voxels the whole-grid call
 * stores there, whatever the chunk size.  A correction without flagged cells gives the plain DecodeToDevice of the box.
 *
 * SetResidentForm chooses what the apply reads on the device.  FIXED (the default of every correction however it was made): a
 * 16-byte entry per macrocell of the grid and the fixed-width payload; a correction read from packed bytes is unpacked into it
 * by its first apply.  PACKED: the packed payload as it is serialised, plus an index computed on the host from the group table:
 * 16 bytes per macrocell of the grid {the cell's first plane word, its first group} and 4 bytes per group {the group's first word
 * inside its cell (at most 63 * 64), nbits}.  The apply then gathers a voxel's code from the planes: cell -> entry, li -> group
 * li / 64 and lane li % 64, z = sum over b < nbits of ((plane word b >> lane) & 1) << b, kinds 0 and 1 q = (z >> 1) ^ -(z & 1),
 * kind 2 z is the stored bit pattern; a group with nbits == 0 reads no plane word.  No unpacked copy is made, and what is stored
 * is bit for bit what the FIXED form stores.
 * A correction that holds nothing on the device only notes the form, and its first apply uploads that form alone: PACKED set
 * before the first apply of a correction read from packed bytes never allocates the fixed-width payload on the device and never
 * runs the unpack.  A correction that is resident is converted by the call itself, on the library's stream: to PACKED it is
 * packed on the device if it has no packed form yet (cached, as by SerializePacked), the index is built and uploaded, and the
 * fixed-width payload and its table are released after the stream has drained; to FIXED the planes are unpacked on the device and
 * then released with the index.  Serialize, SerializePacked and GetInfo give the same bytes and values in either form.
 * GetResidency: form; payload_device_bytes = the payload of the resident form; index_device_bytes = the PACKED form's index, cell
 * entries included (0 in FIXED form); device_bytes = everything the correction holds on the device, FIXED's cell table included;
 * on_device = device_bytes != 0.  All are 0 before the first upload and for a correction without flagged cells.  In PACKED form
 * device_bytes = packed payload + 4 * groups + 16 * cells of the grid.
 * Errors: those of DecodeToDeviceCorrected; a null handle or result; a form other than 0 or 1 (nothing changes). */
#define VNR_AMD_CORRECTION_RESIDENT_FIXED  0
#define VNR_AMD_CORRECTION_RESIDENT_PACKED 1
typedef struct vnrAmdCorrectionResidency { int form, on_device; uint64_t device_bytes, payload_device_bytes, index_device_bytes; } vnrAmdCorrectionResidency;
int  vnrAmdCorrectionSetResidentForm(vnrAmdCorrection, int form);
int  vnrAmdCorrectionGetResidency(vnrAmdCorrection, vnrAmdCorrectionResidency*);
int  vnrAmdNeuralVolumeDecodeBoxToDeviceCorrected(vnrAmdVolume neural, vnrAmdCorrection, void* d_out, const int64_t strides[3],
                                                  const int box_lo[3], const int box_size[3], void* stream, int verify_params);
/* AMD extension: corrections to a byte budget.  CorrectionRates says what many tolerances would cost without building any of them;
 * BuildCorrectionWithinBytes uses it to build the correction of the tightest tolerance it can find whose serialised size fits.
 * Pointer, strides, alignment, allocation room, stream and value range are BuildCorrection's, with its refusals and messages.
 *
 * CorrectionRates: n_eps is 1 to 64; each eps[k] is a finite double >= 0, in any order, duplicates allowed; out: host memory, n_eps
 * entries.  Entry k holds EXACTLY what BuildCorrection(..., eps[k], ...) followed by Serialize and SerializePacked would report on
 * the same parameters and the same d_ref:
 *   kind             per entry; FLOAT / DOUBLE with eps[k] == 0 is kind 2, verbatim
 *   n_flagged        flagged cells;  n_voxels_flagged  voxels with q != 0 (kind 2: that differ)
 *   n_groups         the sum of ceil(voxels / 64) over the flagged cells
 *   payload_bytes    the sum over the flagged cells of pad16(voxels * width), width by the rule above on m = max |q| (kind 2: sizeof(T))
 *   serialized_bytes         = 104 + 8 n_flagged + payload_bytes                 (the "VNRCORR1" form)
 *   packed_payload_bytes     = pad8(n_groups) + 8 * the sum of nbits over the groups of the flagged cells
 *   packed_serialized_bytes  = 104 + 8 n_flagged + packed_payload_bytes          (the "VNRCORP1" form)
 *   refused          1 where some cell has m > 2^31 - 1, the case the build refuses; the entry's counts and sizes are then 0 and the
 *                    call itself succeeds
 * The network is evaluated once per voxel per call whatever n_eps is, chunk by chunk (VNR_AMD_DECODE_CHUNK, rounded down to whole
 * groups of 64 codes, at least one; the result does not depend on it), in the packed form's order over all cells of the grid: one
 * wavefront takes one group, forms r once and then, per tolerance, the build's own quantiser, two wave maxima and a ballot, folded
 * per cell with integer atomics.  The call stores nothing in d_ref, changes no state of the volume and keeps nothing resident but
 * the chunk scratch every round-trip call shares; its own scratch is 8 bytes per macrocell and tolerance (CorrectionRatesCoded below:
 * 4 more, 12).  Only the n_eps results cross to the host.
 * Errors: BuildCorrection's; a null eps or out; n_eps outside 1 .. 64; an eps[k] that is negative, NaN or infinite (k and the value
 * are named).  These four are found before the volume is looked at.
 *
 * BuildCorrectionWithinBytes: max_bytes bounds the serialised size in `form` (FIXED: Serialize, PACKED: SerializePacked).  The
 * search is host code in which every step is one IEEE double operation, none contracted into an fma:
 *   round 0:  t_j = ldexp(eps_hi, -j), j = 0 .. 15, one rate call.  eps_hi must be finite and > 0 and t_15 a normal number.  An entry
 *       that is `refused` does not fit.  If t_0 does not fit the call returns NULL and the message names max_bytes, eps_hi and the
 *       size at eps_hi.  J = the largest j such that every t_i, i <= J, fits; hi = t_J; J == 15 ends the search; otherwise lo = t_(J+1).
 *   rounds 1 .. rounds (0 <= rounds <= 8):  p_i = lo + (hi - lo) * (i / 16), i = 1 .. 15, evaluated as written: one rate call of 15
 *       tolerances.  I = the smallest i such that every p_i', i' >= I, fits.  No I: lo = p_15.  Otherwise hi = p_I, and lo = p_(I-1)
 *       if I > 1.
 * Then BuildCorrection(hi) runs as it always does and its result is returned.  Its size in `form` must equal the rate's figure (for
 * PACKED this runs the device pack, which stays cached for SerializePacked); a difference is an internal error that names both.
 * Sizes do not grow with the tolerance (rint, and floor_div of r + E by 2 E + 1, are monotone), so the search is a bisection; the
 * prefix / suffix wording only defines the outcome without relying on that.  The integer types need no special case: their sizes
 * depend on floor(eps) alone.
 * report: eps = hi; bytes = its size in `form`; eps_tighter / bytes_tighter = the largest tolerance probed that did not fit and its
 * size (0 where its entry was refused), NaN and 0 if there was none; rate_passes = the number of rate calls.  It is written on
 * success only.
 * Errors (NULL and a message): a null report, a form other than 0 or 1, eps_hi or rounds as above (found before the volume is looked
 * at); those of CorrectionRates and BuildCorrection; eps_hi that does not fit. */
typedef struct vnrAmdCorrectionRate {
  double eps; int kind; int refused;
  uint64_t n_flagged, n_voxels_flagged, n_groups,
           payload_bytes, serialized_bytes,                 /* the "VNRCORR1" form */
           packed_payload_bytes, packed_serialized_bytes;   /* the "VNRCORP1" form */
} vnrAmdCorrectionRate;
int vnrAmdNeuralVolumeCorrectionRates(vnrAmdVolume neural, const void* d_ref, int value_type, const int64_t strides[3],
                                      float range_lo, float range_hi, const double* eps, int n_eps, void* stream,
                                      vnrAmdCorrectionRate* out /* host, n_eps entries */);
#define VNR_AMD_CORRECTION_FORM_FIXED  0
#define VNR_AMD_CORRECTION_FORM_PACKED 1
typedef struct vnrAmdCorrectionBudget { double eps; uint64_t bytes; double eps_tighter; uint64_t bytes_tighter; int rate_passes; } vnrAmdCorrectionBudget;
vnrAmdCorrection vnrAmdNeuralVolumeBuildCorrectionWithinBytes(vnrAmdVolume neural, const void* d_ref, int value_type,
    const int64_t strides[3], float range_lo, float range_hi, uint64_t max_bytes, int form, double eps_hi, int rounds,
    void* stream, vnrAmdCorrectionBudget* report);
/* AMD extension: byte budgets in the coded form ("coded corrections" below, "VNRCORC1": the smallest form the library writes).
 * vnrAmdCorrectionRate's layout is ABI and BuildCorrectionWithinBytes refuses every form but FIXED and PACKED; both stay exactly as
 * they are, and the coded form has entry points of its own.
 *
 * CorrectionRatesCoded: the arguments, refusals and messages of CorrectionRates (the four that need no volume are found before the
 * volume is looked at).  Entry k's `rate` is CorrectionRates' entry k bit for bit; beside it, EXACTLY what BuildCorrection(..., eps[k],
 * ...) followed by SerializeCoded would give:
 *   coded_stream_words      the sum over the flagged cells of the 64-bit words of the cell's stream
 *   coded_payload_bytes     = pad8(4 n_flagged) + 8 coded_stream_words
 *   coded_serialized_bytes  = 104 + 8 n_flagged + coded_payload_bytes
 * All three are 0 where the entry is refused; an entry without a flagged cell has 0 words, 0 payload bytes and 104 serialised bytes.
 * The network is still evaluated once per voxel per call whatever n_eps is, and only the results cross to the host.  The pass is
 * CorrectionRates' with a compile-time variant of its kernel (CorrectionRates itself runs the kernel it always ran): after the
 * quantiser, per group and tolerance, with m_l = |q_l| (kind 2: ref's bit pattern; lanes beyond a ragged cell's voxels 0) and mbits
 * the bit length of the wave's largest m_l, one ballot and one popcount c for each plane b < mbits, 5 + 6 c bits for c <= 9 and 65
 * otherwise, plus (kinds 0 and 1) one sign bit per lane with q_l != 0, folded per cell and tolerance with one integer atomic; every
 * group of a flagged cell, the groups of zeros included, adds the 7 bits of its mbits; a cell's stream is that sum filled up to whole
 * words.  Scratch: CorrectionRates' 8 bytes per macrocell and tolerance, and 4 more for this call.
 *
 * BuildCorrectionCodedWithinBytes: max_bytes bounds the size of SerializeCoded.  The search is BuildCorrectionWithinBytes' search,
 * unchanged, fed with coded_serialized_bytes.  The tolerance it returns is then built by BuildCorrectionPacked, so the correction
 * comes back in the PACKED resident form and no fixed-width payload is allocated at any point; the device encode then runs once,
 * its size must equal the rate's figure (a difference is an internal error that names both) and its bytes stay cached for
 * SerializeCoded and SerializeCodedToDevice.  report is BuildCorrectionWithinBytes', with bytes in the coded form.
 * Coded sizes CAN grow with the tolerance, unlike FIXED and PACKED sizes: a lane whose magnitude falls from 4 to 3 sets two lower
 * plane bits where it cleared one, which can push a plane from a list to the dense form.  The search's prefix / suffix wording
 * defines its outcome without monotonicity: what is returned always fits max_bytes and is what that rule chooses among the
 * tolerances probed; it is not claimed to be the tightest tolerance that fits.
 * Errors (NULL and a message): a null report, eps_hi or rounds as for BuildCorrectionWithinBytes (found before the volume is looked
 * at); those of CorrectionRates and BuildCorrectionPacked; eps_hi that does not fit (max_bytes, eps_hi and the size are named). */
typedef struct vnrAmdCorrectionRateCoded {
  vnrAmdCorrectionRate rate;            /* exactly what CorrectionRates gives for this tolerance */
  uint64_t coded_stream_words,          /* sum over the flagged cells of the 64-bit words of the cell's stream */
           coded_payload_bytes,         /* pad8(4 n_flagged) + 8 coded_stream_words */
           coded_serialized_bytes;      /* 104 + 8 n_flagged + coded_payload_bytes: the size of SerializeCoded */
} vnrAmdCorrectionRateCoded;            /* 96 bytes */
int vnrAmdNeuralVolumeCorrectionRatesCoded(vnrAmdVolume neural, const void* d_ref, int value_type, const int64_t strides[3],
                                           float range_lo, float range_hi, const double* eps, int n_eps, void* stream,
                                           vnrAmdCorrectionRateCoded* out /* host, n_eps entries */);
#define VNR_AMD_CORRECTION_FORM_CODED 2  /* names the form; BuildCorrectionWithinBytes still refuses it */
vnrAmdCorrection vnrAmdNeuralVolumeBuildCorrectionCodedWithinBytes(vnrAmdVolume neural, const void* d_ref, int value_type,
    const int64_t strides[3], float range_lo, float range_hi, uint64_t max_bytes, double eps_hi, int rounds,
    void* stream, vnrAmdCorrectionBudget* report);
/* AMD extension: corrections built straight into bit planes.  BuildCorrectionPacked is BuildCorrection (arguments, validation,
 * refusals and messages, the refusal of a code wider than 32 bits included; a refused call returns NULL and keeps nothing
 * resident) and gives the SAME correction: Serialize and SerializePacked bytes, every field of GetInfo, the corrected decode of
 * the grid and of any box, and GetResidency in either form are bit for bit what BuildCorrection of the same arguments gives.
 * What differs is how it gets there.  The correction is returned in the PACKED resident form (the packed payload as serialised,
 * 16 bytes per macrocell, 4 bytes per group); no fixed-width payload is allocated on the device or the host, and no code crosses
 * to the host during the call:
 *   pass 1   chunks of whole groups of 64 codes over ALL cells of the grid, in the packed form's order (CorrectionRates' walk and
 *            chunking), the network evaluated once; one wavefront takes one group, forms dec, r, q and z as BuildCorrection does,
 *            stores the group's nbits in one byte per group of the grid, folds {max |q|, sum of nbits} per cell with integer
 *            atomics, and reduces both error reports: before max |dec - ref|, after max |corrected - ref| with its first voxel by
 *            lowest x-fastest index, the voxels with q != 0 and the NaN voxels.  (A cell that ends up not flagged has q == 0
 *            everywhere, so its corrected value is dec.)  Kind 2 records nbits of ref's bit patterns whether or not a group differs;
 *            a cell is flagged by "differs".
 *   host     the per-cell pairs alone (8 bytes per macrocell): the width rule, the refusal, the entries {cell, width}, and the
 *            exclusive sums that give each flagged cell's first group and first plane word.
 *   index    one wavefront per flagged cell copies the cell's nbits into the packed group table, scans them into the per-group
 *            index {first word inside the cell, nbits} and counts the groups with nbits > 0; a device prefix sum of the counts
 *            orders the list of those groups (never an atomic).
 *   pass 2   the network a second time for the listed groups alone, in chunks of the list: z again, one ballot per plane, lane b
 *            keeps plane b, one 8-byte store per lane.  Its cost follows what is stored, not the grid.
 * Scratch beyond the chunk scratch every round-trip call shares: 8 bytes per macrocell, 1 byte per group of the grid, 8 bytes per
 * listed group.  The result does not depend on VNR_AMD_DECODE_CHUNK.  GetInfo on such a correction moves nothing (the fixed-width
 * sizes follow from the entries); the first SerializePacked downloads table plus planes once and caches them; Serialize unpacks
 * on the host from that; SetResidentForm(FIXED) unpacks on the device.  BuildCorrectionWithinBytes is unchanged.
 *
 * SerializePackedToDevice writes the exact "VNRCORP1" bytes of SerializePacked into device memory, for GPU-aware I/O or MPI: header
 * and entries from the host, group table and planes device to device when the planes are resident (in PACKED form they are made
 * resident first; in FIXED form the device pack runs as for SerializePacked).  *size is always set; d_bytes == NULL only reports
 * it.  d_bytes follows d_out's pointer rules (allocation room is checked where the runtime knows the allocation); stream is the
 * consumer's, waited for as DecodeToDevice does; the call returns after the bytes are there.
 * Errors: a null handle or size; capacity < *size (both are named, nothing is written). */
vnrAmdCorrection vnrAmdNeuralVolumeBuildCorrectionPacked(vnrAmdVolume neural, const void* d_ref, int value_type, const int64_t strides[3],
                                                         float range_lo, float range_hi, double eps, void* stream);
int  vnrAmdCorrectionSerializePackedToDevice(vnrAmdCorrection, void* d_bytes, size_t capacity, size_t* size, void* stream);
/* AMD extension: coded corrections.  A third serialised form of the same correction, "VNRCORC1": the same codes and header fields,
 * either of the other two forms recoverable from it byte for byte.  It removes what the packed form still spends at low rates: a
 * sign bit for every code, zeros included, and 64 bits for a plane however few of them are set.  It is a serialised form only: on
 * the device a correction is resident as fixed-width codes or as bit planes, and no apply reads coded streams.
 *
 * Little-endian.  The header above with magic "VNRCORC1", version 1 and payload_bytes the size of the coded payload; the same
 * n_flagged entries {u32 cell, u32 width}; then the payload:
 *   1. the cell table: one u32 per flagged cell in entry order, the 64-bit words of that cell's stream; zero bytes up to a multiple of 8;
 *   2. the cell streams, in entry order.
 * A stream is a run of u64 words; stream bit i is bit i % 64 of word i / 64; a field of n bits is appended least significant bit
 * first; every cell's stream starts on a word and is filled up with zero bits to a whole word.  A cell's stream is the records of
 * its groups in order; the groups are the packed form's (64 consecutive codes in the order lx + cx * (ly + cy * lz), the last group
 * filled with codes of 0: ceil(voxels / 64) groups a cell).
 * Group record, kinds 0 and 1, with q_l the sign-extended code of lane l, m_l = |q_l| (0 .. 2^31) and s_l = (q_l < 0):
 *   1. mbits, 7 bits: the bit length of the largest m_l; if it is 0 the record ends here;
 *   2. for b = mbits - 1 down to 0, with P the set of lanes whose m_l has bit b and c = |P|:
 *        c <= 9: one bit 1, then c in 4 bits, then the lanes of P ascending, 6 bits each;
 *        else:   one bit 0, then 64 bits, bit l set for l in P
 *      (a list costs 5 + 6 c bits against 65, so 9 is the largest count that pays);
 *   3. for every lane with m_l != 0, ascending: one bit s_l.
 * Group record, kind 2 (verbatim patterns): m_l is the stored bit pattern, mbits is 0 .. 64, and there is no step 3.
 * The writer is canonical: what the reader accepts, the writer gives back byte for byte.
 *
 * CreateCorrectionFromCodedBytes is host only and validates everything before it allocates anything by the bytes' say; each rule is
 * refused by name under "malformed coded correction bytes: ": all header and entry rules of CreateCorrectionFromBytes; cell table
 * padding not zero; a payload shorter than the cell table; a payload size that differs from the sum the cell table gives; a record
 * that runs past its cell's words; a table entry that differs from the length its records have; stream padding not zero; mbits
 * above 8 * width; a code that does not fit the width (kinds 0 and 1: m = 2^(8 width - 1) only with the sign set, nothing larger);
 * an empty top plane; a list count above 9; a plane stored dense with 9 or fewer bits set; list lanes not strictly ascending; a bit
 * beyond the cell's voxels.  At its first use on the device the coded payload is uploaded as it is and decoded there by one kernel,
 * a cell a wave, into the packed resident form (the FIXED resident form, the default, then unpacks as for packed bytes), and the
 * coded copy on the device is released; a correction that is only serialised again, or queried, is transcoded on the host and asks
 * for no device.  GetResidency reports what it reports for the same correction read from packed bytes.
 *
 * SerializeCoded returns the bytes (vnrAmdFreeHost), cached like SerializePacked's: encoded on the device from whichever form is
 * resident, codes or planes, in two passes (the records' lengths in closed form from one ballot and popcount a plane; a device
 * scan; the cells' streams assembled in LDS and stored as whole words), no code or plane crossing to the host; a correction that
 * holds nothing on the device (read from bytes of any form and never applied, or without a flagged cell) is transcoded on the host.
 * SerializeCodedToDevice writes the same bytes into device memory, encoded straight into the destination; its arguments, its
 * size-only call (d_bytes == NULL) and its refusals are SerializePackedToDevice's.
 * Byte budgets in this form: CorrectionRatesCoded and BuildCorrectionCodedWithinBytes above.
 * Not built: there is no apply straight from coded streams; there is no prediction across voxels.
 * Errors: a null handle, result or bytes; capacity < *size (both are named, nothing is written); malformed bytes, each rule by name. */
int  vnrAmdCorrectionSerializeCoded(vnrAmdCorrection, void** bytes, size_t* size);
vnrAmdCorrection vnrAmdCreateCorrectionFromCodedBytes(const void* bytes, size_t size);
int  vnrAmdCorrectionSerializeCodedToDevice(vnrAmdCorrection, void* d_bytes, size_t capacity, size_t* size, void* stream);
/* AMD extension: random access to the corrected field.  A list of voxels or of positions instead of a box: no box around a query is
 * decoded, and the correction is read in whichever form is resident, at its resident size.  One lane takes one query.
 *
 * GatherVoxelsCorrected: d_voxels holds n triples {x, y, z} of int32, grid indices of the volume's own grid, in any order,
 * duplicates allowed; d_out receives n elements of the correction's value type, dense.  out[j] is bit for bit what
 * DecodeToDeviceCorrected stores at voxel d_voxels[j], for every value type, kind and resident form.  Only the n listed voxels are
 * evaluated, at ((float)x + 0.5f) * (1.0f / (float)dims.x) and likewise y and z (the decode's arithmetic), through the decode's
 * scratch in chunks of VNR_AMD_DECODE_CHUNK samples; the result does not depend on the chunk size.  A voxel's cell, its index in the
 * cell and its code are those of the apply ("error-bounded round trip", "resident form" above).  A correction without flagged cells
 * gives the plain typed decode of those voxels and nothing is uploaded for it; the first use of a correction read from bytes uploads
 * exactly the resident form that is set, as the apply does (PACKED set beforehand never allocates the fixed-width payload).
 * The whole list is validated on the device before any voxel is evaluated (a ballot per wavefront, an atomic minimum on the list
 * position): a voxel with a component < 0 or >= dims refuses the call with the lowest such j and its triple named, and nothing has
 * been written to d_out.
 *
 * SampleCorrected: d_coords holds n positions {x, y, z} in [0, 1] as for vnrAmdNeuralVolumeInference, d_values receives n float32 in
 * the data units of the correction's range.  The field is continuous: the converted network value plus the trilinear blend of the
 * stored residuals of the eight voxel centres around the position.  Every step is one IEEE operation:
 *   v = the value vnrAmdNeuralVolumeInference gives at the position;
 *   d = __fadd_rn(__fmul_rn(v, range_hi - range_lo), range_lo) (the subtraction in float as well), d = v when range_lo > range_hi:
 *       DecodeToDevice's conversion to FLOAT, NOT rounded to an integer value type;
 *   per axis, in fp32: t = __fsub_rn(__fmul_rn(p, (float)dim), 0.5f); if !(t >= 0) then t = 0 (a NaN coordinate lands here); if
 *       t > (float)(dim - 1) then t = (float)(dim - 1); i0 = (int)floorf(t), i1 = min(i0 + 1, dim - 1), w = __fsub_rn(t, (float)i0),
 *       which is exact;
 *   the residual of a voxel, a double: 0 in a cell that is not flagged; kind 0 (double)(clamp(q, -qmax, qmax) * s) formed in int64,
 *       qmax = 2^34 / s + 1; kind 1 __dmul_rn((double)q, s); q is read as the apply reads it, from the cell table and the
 *       fixed-width payload or from the bit planes;
 *   lerp(a, b, w) = __dadd_rn(__dmul_rn(a, __dsub_rn(1.0, (double)w)), __dmul_rn(b, (double)w)), never an fma, so that w = 0 and
 *       w = 1 give an endpoint exactly; along x for the four rows (y0 z0, y1 z0, y0 z1, y1 z1), then along y, then along z;
 *   the result is d as it is if all eight codes are 0 (-0.0 and a NaN stay), else (float)__dadd_rn((double)d, blend).
 * In the PACKED form the two x-neighbours of a row come out of one pass over their group's planes wherever both lie in one cell and
 * one group (adjacent lanes); at a cell boundary, in a row of a ragged cell that wraps a group and at the clamped upper face they are
 * read one by one.  No unpacked copy and no per-chunk copy of codes is made in either form.  d_values is written by the evaluation
 * first and corrected in place, chunk by chunk; the result does not depend on the chunk size.  A correction without flagged cells
 * gives d.  A verbatim correction (kind 2) is refused by name: its codes are bit patterns, not residuals.
 * Bounds.  The blend is a convex combination of the eight residuals.  With delta_a the distance of axis a's t from the nearest
 * integer, the sample lies within (delta_x + delta_y + delta_z) * (max - min of the eight residuals) of d + residual(voxel), apart
 * from the roundings above, where voxel is the one whose centre is nearest.  For FLOAT, d + residual(voxel) is the corrected voxel
 * before its rounding to float, so at a voxel centre the sample is the corrected voxel.  For the integer types d is not rounded to
 * the type, so at a voxel centre the field is within E + 0.5 of the original there.
 *
 * Both: stream as for DecodeToDevice (the library's stream waits for an event on the caller's; the call has completed on return);
 * verify_params as for DecodeToDeviceCorrected.  Refusals, in this order, the first four groups before any device is initialised: a
 * null correction; (SampleCorrected) a verbatim correction; a null pointer; d_voxels or d_coords not aligned to 4 bytes, d_out or
 * d_values not aligned to the value type; a null volume; dims that differ from the volume's; a malformed VNR_AMD_DECODE_CHUNK.  Then
 * n == 0 returns VNR_AMD_OK without touching a device.  Then: parameter count or hash under verify_params; a list or result that
 * does not fit the allocation it points into; a voxel outside the grid.  A refused call has written nothing. */
int  vnrAmdNeuralVolumeGatherVoxelsCorrected(vnrAmdVolume neural, vnrAmdCorrection, size_t n, const int32_t* d_voxels, void* d_out,
                                             void* stream, int verify_params);
int  vnrAmdNeuralVolumeSampleCorrected(vnrAmdVolume neural, vnrAmdCorrection, size_t n, const float* d_coords, float* d_values,
                                       void* stream, int verify_params);
/* hash-grid encode only (tcnn_impl_decoder.cu:177-230, column = level*F + f): fp16 [n][padded_width] */
int    vnrAmdNeuralVolumeEncode(vnrAmdVolume, size_t n, const float* d_coords, uint16_t* d_features, void* stream);
/* AMD extension: state of the brick image, the de-hashed inference copy of the hashed levels (csrc/grid_levels.h, csrc/brick_cache.h).  It is built
 * once the parameters have been left unchanged for VNR_AMD_BRICK_AFTER (24) inference launches and dropped when they change;
 * VNR_AMD_BRICK=0 disables it, =1 builds it at the first launch; its size is bounded (SetBrickImageBudget below).  Results do not depend on it. */
int    vnrAmdNeuralVolumeBrickImageInfo(vnrAmdVolume, int* in_use, size_t* bytes, float* build_ms);
/* AMD extension: -1 = the environment's policy, 0 = never use the image (frees it: the train-while-render configuration),
 * 1 = build it at the next launch */
int    vnrAmdNeuralVolumeSetBrickImageMode(vnrAmdVolume, int mode);
/* AMD extension: the image's budget in bytes.  0 = the default policy: 1/16 of the device's memory (18 GB on an MI355X; the image of the
 * BASELINE C4 model is 8.8 GB for a 140 MB model, 2 x the fp32 volume it represents) and never more than a quarter of the memory
 * that is free when the image is built; VNR_AMD_BRICK_MAX_GB overrides the policy for the process.  Hashed levels are taken finest
 * first while they fit (what each step buys on the bench frame: profiles/r03_brick_budget_table.json); a new budget drops the
 * image, the next launches rebuild it.  BrickImageLevels: bit l set = level l is read from the image. */
int      vnrAmdNeuralVolumeSetBrickImageBudget(vnrAmdVolume, size_t bytes);
unsigned vnrAmdNeuralVolumeBrickImageLevels(vnrAmdVolume);
/* how often the image has been built, and how many launches with unchanged parameters the next build waits for: 24 (VNR_AMD_BRICK_AFTER), doubled
 * whenever an optimizer step dropped an image that had served fewer than 64 launches -- an application that trains after every frame
 * (apps/int_dual_volume.cpp:631-672) must not pay a build per frame -- and back to 24 once an image has lived longer */
/* Two tiers: while the parameters keep changing, the first large evaluation launch (capacity >= 2^20 samples: a frame) after a change builds a SMALL
 * image (the finest levels that fit VNR_AMD_BRICK_SMALL_GB, default 0.75 GiB: 0.25 ms for the C4 model) that the frame's launches earn back;
 * tier: 0 no image, 1 small, 2 full.  Results do not depend on any of it. */
int      vnrAmdNeuralVolumeBrickImagePolicy(vnrAmdVolume, uint64_t* builds, unsigned* launches_before_next_build, int* tier, uint64_t* small_builds);
/* the layout of a training step's grid backward for `batch` samples, from the library itself (environment overrides, level masking and
 * alignment rules included): out_u32 = {active levels, levels scattered through LDS tiles, entries per tile, blocks per LDS level};
 * out_u64 = {memory-side atomic requests of the global-atomic kernel, upper bound of the LDS tiles' flush requests}: what bench.py's
 * train_roofline is priced with (no restatement of these rules outside the library) */
int      vnrAmdNeuralVolumeGridBackwardPlan(vnrAmdVolume, uint64_t batch, uint32_t out_u32[4], uint64_t out_u64[2]);
/* AMD extension: deterministic training.  On, the hash-grid part of the gradient is summed in 64-bit fixed point (exponent per call from
 * max |dL/dfeature|, one rounding per term, one fp16 rounding per entry: DESIGN.md 4.3), so the same seed, parameters and batches give the same
 * bits on every run: vnrNeuralVolumeTrain (GPU sampler; out-of-core with its synchronous refresh), TrainBegin / TrainEnd and ForwardBackward,
 * with VNR_AMD_TRAIN_OVERLAP on or off (the same bits either way), and data-parallel training over the shm transport.  Not covered: RCCL's
 * fp16 sums, VNR_AMD_OOC_ASYNC=1.  Costs an int64 image of the grid part (8 bytes per grid parameter, allocated by the first deterministic step)
 * and a slower grid backward.  A batch whose dL/dfeatures hold inf / NaN writes NaN to every grid entry of the active levels.  A runtime
 * property: params.json does not carry it.  Off by default; VNR_AMD_DETERMINISTIC=1 makes it the default of volumes created afterwards.
 * GridBackwardPlan reports the form that will run (8-byte elements, the deterministic tile size). */
int      vnrAmdNeuralVolumeSetDeterministicTraining(vnrAmdVolume, int enable);
int      vnrAmdNeuralVolumeGetDeterministicTraining(vnrAmdVolume, int* enabled);
/* AMD extension (measurement): HIP events around the kernels of the training step; GetTrainProfile averages the last <= 64 steps:
 * ms_per_step = {forward, loss + MLP backward, weight gradients, grid backward (+ the exchange's pack kernels), optimizer} */
int    vnrAmdNeuralVolumeSetTrainProfiling(vnrAmdVolume, int enable);
int    vnrAmdNeuralVolumeGetTrainProfile(vnrAmdVolume, double ms_per_step[5], int* n_steps);
int    vnrAmdNeuralVolumeGetInfo(vnrAmdVolume, int* n_levels, int* n_features_per_level, int* padded_width,
                                 int* n_neurons, int* n_hidden_layers, uint64_t* n_params);
/* AMD extension (diagnostics): the rest of what tcnn_network.h:163-221 deserialize_model builds from the model JSON: hidden / output
 * activation (0 None, 1 ReLU, 2 Exponential, 3 Sigmoid, 4 Squareplus, 5 Softplus: the set tcnn_impl.cu:405-415 dispatches), grid type
 * (0 Hash, 1 Dense, 2 Tiled: tcnn_impl_decoder.cu:68-69), interpolation (0 Linear, 1 Smoothstep, 2 Nearest: :73-94), and whether the
 * model runs on the MFMA kernels (inference / training; always 1 since round 4: every model the reference's dispatch builds does) */
int    vnrAmdNeuralVolumeGetModelKind(vnrAmdVolume, int* activation, int* output_activation, int* grid_type, int* interpolation,
                                      int* mfma_inference, int* mfma_training);
/* the hash grid's level table as the library laid it out (EXTERNAL tcnn level sizing): per level the grid resolution, the
 * entries of its table, its offset in entries and its kind (0 dense, 1 prime-XOR hash, 2 / 3 / 4 Tiled over 1 / 2 / 3 dimensions); arrays
 * of max_levels elements, any may be NULL.  Returns n_levels (-1 on error). */
int    vnrAmdNeuralVolumeLevelTable(vnrAmdVolume, int max_levels, uint32_t* resolution, uint32_t* entries, uint32_t* offset, uint32_t* kind);
/* raw tcnn-order parameter blob (MLP weights, then grid), fp16 */
int    vnrAmdNeuralVolumeGetParamsFP16(vnrAmdVolume, uint16_t* host_out, size_t count);
int    vnrAmdNeuralVolumeSetParamsFP16(vnrAmdVolume, const uint16_t* host_in, size_t count);

/* Data-parallel training hooks (new work): TrainBegin = sample + forward + backward, leaves the loss-scaled (x 128)
 * gradient of the whole parameter blob in ONE half-precision device buffer (tcnn keeps its gradients in half precision too; sum it over
 * the ranks with vnrAmdNeuralVolumeAllReduceGradients), TrainEnd = optimizer step (+ macrocell update).
 * vnrAmdNeuralVolumeTrain(steps) == steps x (Begin; End).  vnrAmdNeuralVolumeGradients returns a FLOAT COPY of that buffer for
 * inspection (device pointer, valid until the next call); changing it changes nothing. */
int    vnrAmdNeuralVolumeTrainBegin(vnrAmdVolume);
float* vnrAmdNeuralVolumeGradients(vnrAmdVolume, size_t* count);
int    vnrAmdNeuralVolumeTrainEnd(vnrAmdVolume, float grad_scale, int fast_mode);
/* forward + backward on a caller-provided batch (same kernels as TrainBegin, no sampling).  Like TrainBegin it ADDS the batch's gradients to
 * the gradient buffer, which the optimizer step (TrainEnd) clears as it consumes it: one call per TrainEnd is a training step, several calls
 * before one TrainEnd accumulate micro-batches (each scaled by 1 / its own batch size). */
int    vnrAmdNeuralVolumeForwardBackward(vnrAmdVolume, size_t n, const float* d_coords, const float* d_targets);
/* Inspection of the last ForwardBackward / TrainBegin (tests/diag/grad_hammer.py; passive: no other call depends on them).
 * TrainingBuffer: device pointer + size of 0 the fp16 gradient blob, 1 dL/dfeatures [n][padded_width] fp16, 2 the encoded features,
 * 3 the hidden activations, 4 the int64 image of the grid part that deterministic training sums into (zero between steps; 0 bytes before the
 * first deterministic step), 5 dL/d(pre-activation) of every hidden layer's output [n_hidden_layers][n][n_neurons] fp16, 6 the loss-scaled
 * dL/dy [n] fp16 after the output activation's backward, 7 the training forward's output [n] fp32.  RescatterGridGradients: clears the hash-grid part of the blob and repeats the grid backward alone on the
 * stored dL/dfeatures (same d_coords as the ForwardBackward it repeats).  GradientDistance: out4 = {sum (g - ref)^2, sum ref^2} over
 * the MLP part, then over the grid part, against an fp16 reference blob on the device, reduced on the device on the training stream. */
int    vnrAmdNeuralVolumeTrainingBuffer(vnrAmdVolume, int which, const void** d_ptr, size_t* bytes);
int    vnrAmdNeuralVolumeRescatterGridGradients(vnrAmdVolume, size_t n, const float* d_coords);
int    vnrAmdNeuralVolumeGradientDistance(vnrAmdVolume, const uint16_t* d_reference, double* out4);
int    vnrAmdNeuralVolumeSetSamplerSeed(vnrAmdVolume, uint64_t seed, uint64_t stream_id);
int    vnrAmdNeuralVolumeSetInitSeed(vnrAmdVolume, uint64_t seed); /* reference seeds with time(NULL), tcnn_network.h:209 */

/* ---- general volume (api.h:146-148) --------------------------------------- */
int  vnrAmdVolumeSetClippingBox(vnrAmdVolume, const float lower[3], const float upper[3]); /* vnrVolumeSetClippingBox */
int  vnrAmdVolumeSetScaling(vnrAmdVolume, const float scale[3]);                           /* vnrVolumeSetScaling */
/* AMD extension: the volume's object -> world map as gdt::affine3f stores it (columns vx, vy, vz, then the translation p: 12 floats).
 * The reference's vnr* API only ever scales the default map; its OVR plugin hands the renderer an arbitrary one
 * (device/device_impl.cpp:151-153, 175-184: translate(grid_origin) * scale(grid_spacing * dims)). */
int  vnrAmdVolumeSetTransform(vnrAmdVolume, const float vx_vy_vz_p[12]);
/* AMD extension: the value range of a simple volume's voxels BEFORE the normalisation to [0, 1] on load (m_value_range_unnormalized,
 * neural_sampler.cu:117-118): what maps a transfer function's range given in data units onto the normalised voxels */
int  vnrAmdSimpleVolumeGetDataRange(vnrAmdVolume, float range[2]);
int  vnrAmdVolumeGetValueRange(vnrAmdVolume, float range[2]);                              /* vnrVolumeGetValueRange */
int  vnrAmdVolumeGetDims(vnrAmdVolume, int dims[3]);
int  vnrAmdVolumeIsNetwork(vnrAmdVolume);
/* macrocell access (VolumeObject::get_macrocell_*, instantvnr_types.h:222-225); pointers are device pointers */
int  vnrAmdVolumeGetMacrocell(vnrAmdVolume, int mc_dims[3], float mc_spacings[3], const float** d_value_range,
                              const float** d_max_opacity);
void vnrAmdReleaseVolume(vnrAmdVolume);

/* ---- renderer (api.h:168-178) --------------------------------------------- */
vnrAmdRenderer vnrAmdCreateRenderer(vnrAmdVolume);                                   /* vnrCreateRenderer */
int  vnrAmdRendererSetFramebufferSize(vnrAmdRenderer, int width, int height);        /* vnrRendererSetFramebufferSize */
int  vnrAmdRendererSetTransferFunction(vnrAmdRenderer, vnrAmdTransferFunction);      /* vnrRendererSetTransferFunction */
int  vnrAmdRendererSetCamera(vnrAmdRenderer, vnrAmdCamera);                          /* vnrRendererSetCamera */
int  vnrAmdRendererSetMode(vnrAmdRenderer, int mode);                                /* vnrRendererSetMode */
int  vnrAmdRendererSetDenoiser(vnrAmdRenderer, int enable);                          /* vnrRendererSetDenoiser: accepted; 1 warns once on stderr that frames stay undenoised (OptiX's trained denoiser has no counterpart here); VNR_AMD_DENOISER_STRICT=1 refuses */
int  vnrAmdRendererSetVolumeSamplingRate(vnrAmdRenderer, float rate);                /* vnrRendererSetVolumeSamplingRate */
int  vnrAmdRendererSetVolumeDensityScale(vnrAmdRenderer, float scale);               /* vnrRendererSetVolumeDensityScale */
int  vnrAmdRendererResetAccumulation(vnrAmdRenderer);                                /* vnrRendererResetAccumulation */
int  vnrAmdRender(vnrAmdRenderer);                                                   /* vnrRender */
/* vnrRendererMapFrame: host pointer to width*height vec4f, valid until two frames later (renderer.h:84-94) */
const float* vnrAmdRendererMapFrame(vnrAmdRenderer);
/* MainRenderer::set_output_as_cuda_framebuffer (renderer.h:160): MapFrame then returns a device pointer */
int  vnrAmdRendererSetOutputAsDeviceFramebuffer(vnrAmdRenderer, int enable);
/* image-tile sharding (new work): render only pixels [pixel_lo, pixel_hi) of the full image;
 * global pixel indices (RNG seeds, accumulation) are preserved so tiles compose exactly. */
int  vnrAmdRendererSetPixelRange(vnrAmdRenderer, uint32_t pixel_lo, uint32_t pixel_hi);
/* interleaved sharding for load balance: this renderer owns the pixel blocks b (of `block_pixels` consecutive
 * pixels, e.g. 8 scanlines) with b % n_parts == part; empty-space skipping makes contiguous tiles uneven. */
int  vnrAmdRendererSetPixelInterleave(vnrAmdRenderer, uint32_t block_pixels, uint32_t n_parts, uint32_t part);

typedef struct {
  uint64_t n_samples;        /* live samples inferred in the last frame */
  uint64_t n_reference_slots;/* N_ITERS x alive rays summed over iterations: what the reference would infer */
  uint32_t n_iterations;
  uint32_t n_rays_hit;
  double   infer_kernel_ms;  /* sum over the frame of the fused encode+MLP kernel (HIP events), if profiling */
  uint64_t infer_kernel_launches;
  double   infer_union_ms;   /* length of the union of those launches' intervals: overlapping launches of the ray halves count once */
} vnrAmdFrameStats;
int  vnrAmdRendererGetFrameStats(vnrAmdRenderer, vnrAmdFrameStats*);
int  vnrAmdRendererSetProfiling(vnrAmdRenderer, int enable);
/* Asynchronous frames (new; the reference's render() synchronises once per iteration, method_raymarching.cu:923-929): with
 * a device framebuffer (SetOutputAsDeviceFramebuffer) and rendering modes 5 / 6 / 8 / 9, vnrAmdRender returns once the frame's
 * predicted iterations are enqueued and vnrAmdRendererMapFrame / GetFrameStats / the next vnrAmdRender complete it.  The caller
 * must not change the volume between Render and MapFrame.  Off by default. */
int  vnrAmdRendererSetAsync(vnrAmdRenderer, int enable);
/* Execution strategy of rendering modes 6 / 9 / 12 (ray marching) and 14 / 15 (path tracing) on a neural volume: 1 = in shader, one
 * launch per frame with the network evaluated inside the marching / tracking loop (method_raymarching.cu:981-1249,
 * method_pathtracing.cu:968-1025), 0 = sample streaming, -1 (default) = env VNR_AMD_IN_SHADER or, without it, the faster one for the
 * mode as measured: ray marching streams (in shader is 2 x slower on a whole frame), path tracing runs in shader
 * (1.25 x faster).  Same frames either way: bit for bit for path tracing, up to the streaming path's resume rounding for ray marching. */
int  vnrAmdRendererSetInShaderKernel(vnrAmdRenderer, int mode);
/* diagnostics: device pointers to the compacted sample queue ([n][3] fp32) and the counter block, plus the
 * per-iteration duration (ms) of the sample-evaluation kernel in the last profiled frame */
int  vnrAmdRendererDebugQueues(vnrAmdRenderer, const float** d_coords, const uint32_t** d_counters, float* iteration_ms, int max_iterations);
/* diagnostics: the schedule the last sample-streaming frame ran with: out = {samples per ray and iteration (N_ITERS, method_raymarching.cu:30-40),
 * ray parts, 1 = done inside the evaluation kernel: the survivors of an iteration are numbered (dense ray -> list slot) by that kernel's
 * prologue, for parts of every size; 0 = by a kernel of its own behind the evaluation (volumes without a network, 128-neuron models),
 * 1 = decoupled walk / evaluate / compose loop}.  Tests use it to know WHICH path they compared with the oracle (a rank's small share runs
 * another schedule than a whole frame). */
int  vnrAmdRendererDebugSchedule(vnrAmdRenderer, int out[4]);
/* The same report by name, with where the last frame's compose kernels read the transfer function: the streaming loops (coupled and
 * decoupled) keep the colour and the opacity table in LDS while the pair fits tfn_lds_bytes (16 bytes per colour, 4 per opacity: 1228
 * entries each for tables of equal length) and read them from global memory above that; the same lookup either way.  tfn_in_lds is
 * decided by the transfer function of the frame rendered last, whatever its rendering mode (the other modes always read global memory). */
typedef struct vnrAmdSchedule {
  int n_iters;        /* samples per ray and iteration */
  int n_parts;        /* ray parts */
  int fused_pack;     /* 1 = survivors numbered inside the evaluation kernel */
  int decoupled;      /* 1 = decoupled walk / evaluate / compose loop */
  int tfn_in_lds;     /* 1 = both transfer function tables in LDS, 0 = read from global memory */
  int tfn_lds_bytes;  /* the budget that decides it */
} vnrAmdSchedule;
int  vnrAmdRendererGetSchedule(vnrAmdRenderer, vnrAmdSchedule*);
/* diagnostics: the numbering of an iteration's surviving rays on its own (pack_rays.h), as the kernel behind the evaluation runs it.
 * n_in > 0: rays the march consumed; counts[g], g < ceil(n_in / 64): what it leaves per 64-ray group, survivors in the low byte (the
 * bytes above it belong to the frame statistics).  Host arrays in and out: src_out (room for n_in entries) receives the list slot
 * 64 g + l of the dense rays 0 .. alive, alive_out the published number of them. */
int  vnrAmdDebugRaySourceIndex(const uint32_t* counts, uint32_t n_in, uint32_t* src_out, uint32_t* alive_out);
/* diagnostics: what the evaluation kernel the dispatcher launches for inference was compiled to, by model shape: F features per level, K_IN padded
 * encoding width, W neurons, general != 0 for a model outside the common kind (rarer grid types, interpolations, activations).  regs: vector
 * registers per lane (96 or fewer let five waves share a SIMD), scratch_bytes: private memory per lane (0 = nothing spilled), lds_bytes: static
 * LDS of a block (the weight image is dynamic LDS and not counted).  Any output may be NULL. */
int  vnrAmdDebugEvalKernelResources(uint32_t F, uint32_t K_IN, uint32_t W, int general, int* regs, int* scratch_bytes, int* lds_bytes);
void vnrAmdReleaseRenderer(vnrAmdRenderer);

/* ---- multi-GPU: one process per GPU (new work; the reference is single-GPU, its only device-selection code is
 * renderer.cpp:299-304 and it has no collective) ------------------------------------------------------------------------------
 * Transports: "rccl" (librccl.so of the ROCm the process runs on, opened with dlopen here; device pointers straight into
 * ncclAllGather / ncclAllReduce on HIP streams) and "shm" (host-staged through one shared-memory segment of the node: several
 * ranks on one GPU, or none; tests).  NULL / "" = env VNR_AMD_DIST_TRANSPORT, default "rccl".
 * InitFromEnv reads the torchrun contract (RANK, LOCAL_RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT), binds the process to
 * device LOCAL_RANK (modulo the device count) and meets the other ranks on a control socket of its own: an abstract unix
 * socket named after MASTER_PORT when MASTER_ADDR is this host, tcp MASTER_ADDR:MASTER_PORT+1 otherwise
 * (VNR_AMD_DIST_ADDR = "unix:<name>" | "tcp:<host>:<port>" overrides).  Init is the explicit form for an application with its
 * own rendezvous: unique_id = the 128 bytes of vnrAmdDistGetUniqueId from one rank (NULL: exchanged over `address`). */
int  vnrAmdDistGetUniqueId(void* out128);
int  vnrAmdDistInit(int rank, int world_size, int local_rank, const void* unique_id, const char* transport, const char* address);
int  vnrAmdDistInitFromEnv(void);
int  vnrAmdDistFinalize(void);
int  vnrAmdDistRank(void);
int  vnrAmdDistWorldSize(void);
const char* vnrAmdDistTransport(void);
int  vnrAmdDistRcclRanksSeen(void);   /* ncclCommCount of the communicator; 0 when the transport is not RCCL */
int  vnrAmdDistBarrier(void);                                      /* device synchronize + host barrier */
/* host values over the control plane (the bench's MAX / SUM over ranks); op: 0 sum, 1 max, 2 min, 3 mean */
int  vnrAmdDistAllReduceHost(double* values, int n, int op);
/* the transport's collectives on caller buffers (device pointers; host pointers on the shm transport), blocking.
 * dtype: 0 f32, 1 f16, 2 u8.  AllGather: rank r's bytes land at recv + r * bytes_per_rank (send may be that address). */
int  vnrAmdDistAllReduce(void* buf, size_t count, int dtype, int op);
int  vnrAmdDistAllGather(const void* send, void* recv, size_t bytes_per_rank);
int  vnrAmdDistReduceScatter(void* buf, size_t count_per_rank, int dtype);
int  vnrAmdDistBroadcast(void* buf, size_t bytes, int root);
/* First-contact self-test: every collective the sharded paths use (in-place all-gather of a frame share, reduce-scatter(Avg) fp16 on a
 * slice length that divides nothing + all-gather of the slices, broadcast, all-reduce(Sum) fp16) once on patterned buffers whose
 * result each rank computes by itself.  A collective that does not complete within deadline_s (the stream is polled from the host) or
 * returns other values fails with its name in vnrAmdGetLastError; the process should then EXIT (a hung collective cannot be
 * cancelled).  report (optional): a one-line summary. */
int  vnrAmdDistSelfTest(double deadline_s, char* report, size_t report_size);
/* Image tiles: the rank renders the 8-scanline tile rows r with r % world == rank into its slot of a [world][share] buffer;
 * vnrAmdRendererMapFrame (= vnrAmdRendererGatherFrame) all-gathers in place, de-interleaves and returns the WHOLE frame on
 * every rank, bit-identical to the unsharded frame rendered with the same batch size (VNR_RM_N_ITERS): a share of at most 262 144
 * pixels marches 32 samples per ray and iteration instead of 24 unless VNR_RM_N_ITERS pins it, and the batch size moves the last bit
 * of a few samples (0.2 % of the pixels, <= 4e-5; the same holds in the reference for its N_ITERS).  RenderPipelined: enqueue frame k, gather frame k - 1 meanwhile on the
 * communication stream, complete frame k, return the assembled frame k - 1 (NULL the first time); FlushPipeline returns the
 * frame still in flight.  The head of frame k (ray generation, first batch of samples) is enqueued before the host has seen
 * frame k - 1 complete, so the GPU does not idle during the host's turn-around; a renderer that is not distributed pipelines the
 * same way. */
int  vnrAmdRendererSetDistributed(vnrAmdRenderer, int enable);
const float* vnrAmdRendererGatherFrame(vnrAmdRenderer);
int  vnrAmdRendererRenderPipelined(vnrAmdRenderer, const float** previous_frame);
/* statistics of the frame COMPLETED last (vnrAmdRendererGetFrameStats completes a pending frame first, which ends the overlap) */
int  vnrAmdRendererGetCompletedFrameStats(vnrAmdRenderer, vnrAmdFrameStats*);
int  vnrAmdRendererFlushPipeline(vnrAmdRenderer, const float** last_frame);
/* Data-parallel training: `steps` steps, each equal to ONE step on the concatenated batch of all ranks (Adam on the MEAN of the
 * ranks' gradients).  Gradients travel as fp16 (2 B x n_params per step), range by range (the MLP, then the hash-grid levels from
 * the finest to the coarsest in buckets) while the backward pass of the coarser levels and the update of earlier ranges run; no host
 * synchronisation inside a step on the rccl transport.  The optimizer is SHARDED by default: a range is reduce-scattered (ncclAvg),
 * the rank updates its 1/world of the range and the fp16 parameters are all-gathered in place: the bytes of an all-reduce on the
 * wire, 1/world of the optimizer sweep per rank (VNR_AMD_DP_SHARDED=0: all-reduce + the whole update on every rank; the same bits
 * wherever the reduction gives the same bits).  A call first asks over the control plane whether any rank's parameters changed
 * outside an optimizer step since the last synchronisation (first call, SetParams, SetModel, a loaded params.json) and if so makes
 * the replicas identical (SyncReplicas: rank 0's parameters, optimizer state, step count and learning rate; with a sharded
 * optimizer state the ranks' slices of it are all-gathered instead).  Every rank draws its own sample stream.
 * After sharded steps a rank's optimizer state of the OTHER ranks' slices is stale: vnrAmdNeuralVolumeTrain / TrainEnd on such a
 * volume fail until vnrAmdNeuralVolumeSyncReplicas has been called on every rank. */
int  vnrAmdNeuralVolumeTrainDataParallel(vnrAmdVolume, int steps, int fast_mode);
int  vnrAmdNeuralVolumeSyncReplicas(vnrAmdVolume);
/* for the TrainBegin / TrainEnd form: sums the gradient buffer over the ranks, in place (fp16 payload); follow with
 * vnrAmdNeuralVolumeTrainEnd(v, 1.0f / world, fast_mode) */
int  vnrAmdNeuralVolumeAllReduceGradients(vnrAmdVolume);
/* ... or exchange + update of the pending step in one call, nothing overlapped: sharded = 1 reduce-scatter / 1/world Adam /
 * all-gather, 0 all-reduce + full Adam, -1 the process default */
int  vnrAmdNeuralVolumeTrainEndDataParallel(vnrAmdVolume, int fast_mode, int sharded);
/* tests: replaces the gradient buffer by `count` host floats (rounded to its half precision) and marks a step as pending */
int  vnrAmdNeuralVolumeSetGradients(vnrAmdVolume, const float* host, size_t count);

/* ---- isosurface (core/marching_cube.cuh:6-8; apps/batch_isosurface.cpp:70-76) --------------------------------- */
/* vnrMarchingCube(volume, isovalue, &ptr, &size, cuda): marching cubes over the dual grid of the volume's dims voxels (a neural volume is
 * evaluated at the grid nodes index / dims, core/marching_cube.cu:117-122); *xyz = 3 floats per vertex, 3 vertices per triangle, in voxel
 * units (+ 0.5, :245).  on_device = 0: a malloc'ed host array (vnrAmdFreeHost; the reference hands out new[]), 1: a device array
 * (vnrAmdFree).  Same surface rules as the reference (classification <=, the vertex rule with its 0.001 guard); the case table is this
 * library's own derivation (tools/gen_mc_table.py), so triangle order and the cut of ambiguous faces may differ from the reference's.
 * vnrSaveTriangles(filename, ptr, size): Wavefront OBJ with one "v" line per vertex and one "f" triple per triangle. */
int  vnrAmdMarchingCube(vnrAmdVolume, float isovalue, float** xyz, size_t* n_vertices, int on_device);
int  vnrAmdSaveTriangles(const char* filename, const float* xyz, size_t n_vertices);

/* ---- misc (api.h:185-188) -------------------------------------------------- */
void vnrAmdMemoryQuery(size_t* used_by_renderer, size_t* used_by_network); /* vnrMemoryQuery */
void vnrAmdFreeTemporaryGPUMemory(void);                                   /* vnrFreeTemporaryGPUMemory */

/* ---- hot-path building blocks exposed for parity tests and benches ---------- */
/* StaticSampler::sample (neural_sampler.cu:130-164): n uniform coords in [lower,upper] + cell-centred trilinear values */
int  vnrAmdSimpleVolumeTakeSamples(vnrAmdVolume, size_t n, const float lower[3], const float upper[3],
                                   float* d_coords, float* d_values, void* stream);
/* AMD extension: error-guided training batches.  A simple volume with resident voxels may carry a SAMPLING TABLE: one weight per
 * 16^3 macrocell, from which training batches are drawn instead of uniformly over the volume.  The layout of d_weights is the
 * one of d_block_max of vnrAmdNeuralVolumeErrorAgainstDevice (dims and order of vnrAmdVolumeGetMacrocell: x fastest, ragged last
 * cells), so an error map goes in unchanged: "where the error is" becomes "where to train more".
 *   d_weights         one float per macrocell, a pointer of the library's HIP runtime (as d_data of the ingest); NULL removes the table.
 *   uniform_fraction  in [0, 1]: the share of every batch that is still drawn uniformly over the whole volume.
 *   stream            as for the ingest: the hipStream_t d_weights was produced on (NULL = complete); the library records an event
 *                     on it and makes its own stream wait; the caller's stream is never blocked.
 * The call returns after the table is complete (the caller may overwrite or free d_weights).  The table is built into new memory,
 * the call waits for the draws in flight that may still read the old one, and swaps only on success: a refused call leaves the
 * old table in force.  The table belongs to the volume: it survives vnrAmdSimpleVolumeSetCurrentTimeStep and
 * vnrAmdSimpleVolumeUpdateFromDevice (same dims; a stale map is still a valid weighting) and is released with the volume.
 *
 * The table, all of it exact (integers, or one rounding each in double):
 *   validation   wmax = the unsigned maximum over the float BITS of the entries without a sign bit (for non-negative floats that
 *                is their maximum); an entry that is a NaN, an infinity or negative refuses the call, and so does wmax == 0
 *                (-0.0f counts as 0).
 *   quantisation q[c] = (uint64) rint(((double)w[c] / (double)wmax) * 16777216.0), ties to even; w[c] > 0 with q[c] == 0 gets
 *                q[c] = 1: a cell with any error is never starved, a cell with weight 0 is reached through the uniform share only.
 *   CDF          cdf[c] = q[0] + ... + q[c], uint64, in cell order (a device scan; integer sums do not depend on how they are
 *                parallelised); total = cdf[n_cells - 1] <= n_cells * 2^24.
 *   threshold    T = (uint64) rint((double)uniform_fraction * 4294967296.0).
 * The draw.  TakeSamplesWeighted continues the volume's pcg32 stream, the seed / sequence / offset vnrAmdSimpleVolumeTakeSamples
 * uses (vnrAmdNeuralVolumeSetSamplerSeed).  Sample e of a call consumes exactly six draws, stream positions offset + 6e .. 6e + 5,
 * and the call advances the offset by 6n whichever branch a sample takes:
 *   draw 0       s = next_uint; the sample is uniform iff (uint64)s < T.
 *   draws 1, 2   r = ((uint64)next_uint << 32) | next_uint, k = the high 64 bits of r * total (__umul64hi); the cell is the first c
 *                with cdf[c] > k (an upper bound; cells with q = 0 are never chosen).  Always made, ignored in the uniform branch.
 *   draws 3 - 5  ux, uy, uz = next_float = uint_as_float((next_uint >> 9) | 0x3f800000) - 1.0f.
 *   uniform      p = (ux, uy, uz): what TakeSamples computes for the unit box.
 *   weighted     per axis, with lo = 16 * c_axis and size = min(16, dims - lo):
 *                  p = fminf(__fmul_rn(__fadd_rn((float)lo, __fmul_rn(u, (float)size)), 1.0f / (float)dims), 0x1.fffffep-1f)
 *                three fp32 roundings, never an fma; the reciprocal in fp32, as the decode's coordinates; the clamp keeps p < 1 like
 *                the uniform stream.  A sample may land on its cell's upper face by rounding; that is harmless.
 *   value        the cell-centred trilinear lookup of TakeSamples at p.
 * d_coords [n][3] and d_values [n] are device arrays; `stream` of TakeSamplesWeighted is the stream the kernel runs on (NULL = the
 * library's), as for TakeSamples.  The search of the CDF first looks through a strided top of it staged in LDS; VNR_AMD_GUIDED_LDS=0
 * (read when weights are set) searches global memory alone.  Same bits either way.
 *
 * Training: while the ground truth of a neural volume has a table, vnrAmdNeuralVolumeTrain, ...TrainBegin and
 * ...TrainDataParallel draw their batches from it (6 draws per sample); vnrAmdNeuralVolumeGetTrainingLoss then reports the loss
 * of guided batches.  GetTestingLoss, GetPSNR, GetSSIM, the decode paths and TakeSamples stay uniform and consume the stream as
 * before (3 draws per sample).  Setting weights is the opt-in: without a table every path runs the code it ran before.  The online
 * macrocell update takes a guided batch as it takes any batch, and deterministic training composes: a batch is a pure function of
 * seed, offset and table.  Data-parallel: every rank draws from its own volume's table with its own sequence; the ranks must
 * install the same weights (not checked).
 *
 * SamplingInfo (any output may be NULL): active = 1 with a table; n_cells, total, uniform_fraction of the table (0 without).
 * SamplingCdf: the device pointer of the CDF (n_cells uint64), NULL when there is no table or on error.
 *
 * GuideSamplingByError closes the loop in one call, for a neural volume whose ground truth is resident in the library: the error
 * pass of ErrorAgainstDevice against the ground truth's current float voxels (vnrAmdSimpleVolumeDeviceData, VNR_AMD_TYPE_FLOAT,
 * the whole volume, no range), then its per-macrocell maxima as the ground truth's weights.  It equals the two public calls made
 * by hand, bit for bit: same report (may be NULL), same CDF.
 *
 * Errors (VNR_AMD_ERROR and a message; the previous table stays in force): uniform_fraction a NaN or outside [0, 1], a null
 * volume, a neural volume (Set / Info / Cdf / TakeSamplesWeighted) or a simple one (GuideSamplingByError), an out-of-core or
 * "NOTHING" volume (no resident voxels), weights with a NaN, an infinity or a negative value, all-zero weights (for
 * GuideSamplingByError: a perfect fit), TakeSamplesWeighted without a table, no resident ground truth, no usable device. */
int  vnrAmdSimpleVolumeSetSamplingWeights(vnrAmdVolume simple, const float* d_weights, float uniform_fraction, void* stream);
int  vnrAmdSimpleVolumeSamplingInfo(vnrAmdVolume simple, int* active, uint64_t* n_cells, uint64_t* total, float* uniform_fraction);
const uint64_t* vnrAmdSimpleVolumeSamplingCdf(vnrAmdVolume simple);
int  vnrAmdSimpleVolumeTakeSamplesWeighted(vnrAmdVolume simple, size_t n, float* d_coords, float* d_values, void* stream);
int  vnrAmdNeuralVolumeGuideSamplingByError(vnrAmdVolume neural, float uniform_fraction, vnrAmdDecodeError* report);
/* SamplerAPI::sample_grid (neural_sampler.cu:166-198; out-of-core: sample_streaming_grid, neural_sampler.cpp:967-1035):
 * voxel-centre coordinates of the block [origin, origin + size) of the volume's grid and the ground truth there */
int  vnrAmdSimpleVolumeTakeSamplesGrid(vnrAmdVolume, const int origin[3], const int size[3], float* d_coords, float* d_values,
                                       void* stream);
/* trilinear lookup of given coords; nodal = 1 is the renderer's sampleVolume (raytracing.h:105-110),
 * nodal = 0 the sampler's tex3D (neural_sampler.cu:182-185) */
int  vnrAmdSimpleVolumeSample(vnrAmdVolume, size_t n, const float* d_coords, float* d_values, int nodal, void* stream);
/* MacroCell::update_explicit (macrocell.cu:236-241) on a neural volume's own macrocell */
int  vnrAmdNeuralVolumeUpdateMacrocell(vnrAmdVolume, size_t n, const float* d_coords, const float* d_values, void* stream);
/* MacroCell::update_max_opacity (macrocell.cu:243-253) with an explicit TFN */
int  vnrAmdVolumeUpdateMaxOpacity(vnrAmdVolume, vnrAmdTransferFunction);

#ifdef __cplusplus
}
#endif
#endif
