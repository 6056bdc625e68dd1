#!/usr/bin/env python3
"""In-situ training of a time series: the example and the measuring tool of the device ingest (include/vnr_amd.h, "in-situ ground truth").

A short seeded series (instantvnr_amd/synthetic.py: a vortex field, advected along x and fading from step to step) stands for a
simulation whose output lives in device memory: every step is put into a vnrAmdMalloc buffer.  The volume is created from the first
step (vnrAmdCreateSimpleVolumeFromDevice) and a neural volume on it; for every further step the voxels are replaced in place
(vnrAmdSimpleVolumeUpdateFromDevice), the network trains --steps-per-frame steps from where it stands, and the step's PSNR and the
ingest time are printed.

  --size N               voxels per axis                                                      [64]
  --dtype T              uint8 | int8 | uint16 | int16 | uint32 | int32 | float32 | float64     [uint8]
  --frames K             time steps of the series                                              [4]
  --steps-per-frame S    training steps per time step (0: ingest only)                         [100]
  --ghost G              G ghost layers on every side of the source array (strided ingest)      [0]
  --range-from-data      min / max of every step instead of the type's range (reads the source twice)
  --repeat R             time every ingest R times, report the fastest and the median          [5]
  --compare-host         also time vnrAmdCreateSimpleVolumeFromMemory on the same array (the path a host-resident field takes)
  --round-trip           after each step's training: the error of the decoded voxels against the step's own device array, in data units
                         (vnrAmdNeuralVolumeErrorAgainstDevice), and a decode into a device array of the source's type and ghost
                         layers (vnrAmdNeuralVolumeDecodeToDevice); both timed, beside vnrAmdNeuralVolumeInference on the same
                         number of ready-made coordinates
  --error-bound EPS      after each step's training: a correction for the tolerance EPS (data units, >= 0) against the step's own
                         device array (vnrAmdNeuralVolumeBuildCorrection) and a decode with it applied into a device array of the
                         source's type and ghost layers (vnrAmdNeuralVolumeDecodeToDeviceCorrected).  Per step: the raw bytes, the
                         params.json bytes plus the correction's bytes and the ratio, the flagged cells, the largest error before
                         and after; both calls timed, beside ErrorAgainstDevice and DecodeToDevice on the same arrays
  --packed               with --error-bound: the packed form of each step's correction as well (vnrAmdCorrectionSerializePacked,
                         vnrAmdCreateCorrectionFromPackedBytes).  Per step: the packed bytes, the fixed-width bytes over them, the
                         compressed bytes and the ratio with the packed form, the time of the device pack and of the first corrected
                         decode of a correction read from the packed bytes (upload, unpack on the device, apply)
  --direct               with --error-bound: the correction built straight into the bit planes on the device
                         (vnrAmdNeuralVolumeBuildCorrectionPacked) beside vnrAmdNeuralVolumeBuildCorrection followed by
                         vnrAmdCorrectionSerializePacked, alternating in one process, max(--repeat, 10) samples each after a warm-up.
                         Per step: min, median and max of both and of the direct build plus the one download of its bytes, the bytes each path
                         leaves on the device, and whether both gave the same bytes and report (checked here)
  --coded                with --error-bound: the coded form ("VNRCORC1": sparse bit planes as lists of lanes, signs for the non-zero
                         codes alone) of the correction built straight into the bit planes.  Per step: the packed bytes, the coded
                         bytes, bits a voxel of a flagged cell in both forms and the compressed ratio with each; min, median and max of
                         vnrAmdCorrectionSerializeCodedToDevice and vnrAmdCorrectionSerializePackedToDevice of that correction
                         (alternating, max(--repeat, 10) samples each after one warm-up each); the first corrected decode of a
                         correction read from the coded bytes beside one read from the packed bytes; and whether the correction
                         read back from the coded bytes serialises to the original's packed bytes
  --resident FORM        with --error-bound: fixed | packed, the resident form of each step's correction, set before the corrected
                         decode (vnrAmdCorrectionSetResidentForm); packed keeps the bit planes and an index on the device and no
                         fixed-width payload.  Per step: the form and the bytes the correction holds on the device     [fixed]
  --roi x0,y0,z0,sx,sy,sz  with --error-bound: additionally decode that box of the grid corrected into a dense device array
                         (vnrAmdNeuralVolumeDecodeBoxToDeviceCorrected), check it on the host against the step's own array (every
                         voxel within max_abs_after) and against the same box cut out of the whole-grid corrected decode (equal
                         bytes), and time it beside the plain vnrAmdNeuralVolumeDecodeToDevice of the box
  --probe N              with --error-bound: after the build draw N seeded voxels and N seeded points.  The voxels go through
                         vnrAmdNeuralVolumeGatherVoxelsCorrected: the largest |gather - original| on the host beside the correction's
                         max_abs_after, and whether the values are the whole-grid corrected decode's at those voxels; the points
                         through vnrAmdNeuralVolumeSampleCorrected (not for EPS = 0 on a float type: a verbatim correction has no
                         residuals).  Both calls timed, in the form --resident sets
  --byte-budget BYTES    after each step's training: the correction of the tightest tolerance the search finds whose serialised
                         size is at most BYTES (vnrAmdNeuralVolumeBuildCorrectionWithinBytes).  eps_hi is the step's max_abs from
                         the error report (vnrAmdNeuralVolumeErrorAgainstDevice), at which nothing is flagged.  Per step: the chosen
                         eps and its bytes, the tolerance just below that did not fit and its bytes, the compressed bytes (params.json
                         plus the correction) and the ratio, max_abs_after, the rate passes; the whole call timed, beside one rate call
                         of 16 tolerances (vnrAmdNeuralVolumeCorrectionRates)
  --budget-form FORM     with --byte-budget: fixed | packed | coded, the serialised form BYTES bounds             [packed]
                         coded: vnrAmdNeuralVolumeBuildCorrectionCodedWithinBytes, whose correction is built straight into the bit
                         planes and stored as to_coded_bytes(); the rate call timed is vnrAmdNeuralVolumeCorrectionRatesCoded, beside
                         the plain one, and the packed size at the chosen tolerance is reported next to the coded one
  --budget-rounds N      with --byte-budget: refinement rounds after the ladder eps_hi * 2^-j, 0 .. 8             [2]
  --guided               error-guided batches instead of the series (vnrAmdNeuralVolumeGuideSamplingByError): ONE static field, the
                         synthetic blob field with plateaus at both ends, trained --steps-per-frame steps in all, twice with the same
                         seeds: once with the error map re-installed as sampling weights every --refresh-every steps, once with
                         uniform batches.  After each refresh: the maximum error and the PSNR of both
  --uniform-fraction F   the share of a guided batch that stays uniform                         [0.25]
  --refresh-every N      steps between two error reports / weight maps                          [100]
  --seed N                                                                                     [1]

Times are host clocks around calls that end in a device synchronise.  "update" is the whole vnrAmdSimpleVolumeUpdateFromDevice call
(ingest kernels + macrocell pass); "macrocell" is the macrocell pass alone (vnrAmdSimpleVolumeSetCurrentTimeStep on the current step);
"ingest" is their difference, and the GB/s are the bytes the ingest must move (source bytes once or twice + 4 bytes written per voxel)
over it.  Kernel times proper: run this under rocprofv3 --kernel-trace --stats (the kernels are ingest_minmax_kernel,
ingest_minmax_final_kernel, ingest_convert_kernel).

The --round-trip times are host clocks as well, each around one call that returns after its work has completed: "decode" and
"error" are the whole calls (coordinate kernel + evaluation + store or reduce kernel per chunk of VNR_AMD_DECODE_CHUNK samples),
"inference" is one vnrAmdNeuralVolumeInference call + synchronise over the same voxel centres as ready-made coordinates, so
"decode - inference" is a difference of wall times.  Each is run once to warm up, then --repeat times.  The kernels are decode_coords_kernel, decode_store_kernel,
decode_error_kernel and worst_final_kernel<double>.

The --error-bound times are host clocks around whole calls in the same way: "build" evaluates the network twice and brings the codes
to the host, "apply" evaluates it once.  The kernels are correction_measure_kernel, correction_encode_kernel and
correction_apply_kernel.

The --packed times are host clocks around whole calls too.  "pack" is one vnrAmdCorrectionSerializePacked call on the correction the
build returned, whose codes are resident: two kernels, the cells' offsets through the host between them, the packed bytes brought to
the host and copied out (the result is cached, so it is one measurement a step, after a warm-up on a copy of the correction).
"packed_first_apply" is the first vnrAmdNeuralVolumeDecodeToDeviceCorrected of a correction just read from the packed bytes: the
upload of the packed payload, the unpack kernel and the apply; each repeat reads the bytes anew (the host's validation is outside the
clock).  The kernels are correction_pack_measure_kernel, correction_pack_planes_kernel and correction_unpack_kernel.  With
--resident packed the form is set on the fresh correction first: the upload of the packed payload and of the index, and the apply
that reads the planes (correction_apply_planes_kernel); no unpack.

The --coded times are host clocks around whole calls: "serialize_coded_to_device" is pass 1 (correction_code_measure_kernel), the
device scan of the cells' words, one count to the host and pass 2 (correction_code_write_kernel) straight into the destination, from
the resident planes; "serialize_packed_to_device" copies the resident table and planes device to device.  "coded_first_apply" is the
first vnrAmdNeuralVolumeDecodeToDeviceCorrected of a correction just read from the coded bytes (the upload of the coded payload and of
the index, correction_code_decode_kernel, in the FIXED resident form the unpack kernel, and the apply), "packed_first_apply_again" the
same of one just read from the packed bytes, alternating; the host's validation is outside both.

The --direct times are host clocks around whole calls: "build_pack" is BuildCorrection plus SerializePacked on its result (two
evaluations of the whole grid, the fixed-width codes to the host, the device pack, the packed bytes to the host), "direct" is
BuildCorrectionPacked alone (one evaluation of the whole grid, one of the groups that store planes; table and planes stay on the
device), "direct_and_bytes" adds the SerializePacked that downloads them.  The kernels are correction_direct_measure_kernel,
correction_direct_index_kernel, correction_direct_list_kernel and correction_direct_planes_kernel.

The --roi times are host clocks around whole calls as well, each warmed up once: "roi_apply" evaluates the network for the box's
voxels alone and applies the correction in the resident form, "roi_plain_decode" is DecodeToDevice of the same box.

The --probe times are host clocks around whole calls, each warmed up once: "probe_gather" validates the list, evaluates the network
for the listed voxels alone and applies the correction to them (correction_voxels_check_kernel, correction_voxel_coords_kernel,
correction_gather_kernel), "probe_sample" evaluates the network at the points and blends the stored residuals of the eight voxel
centres around each (correction_sample_kernel).

The --byte-budget times are host clocks around whole calls, each warmed up once: "budget_ms" is the whole
vnrAmdNeuralVolumeBuildCorrectionWithinBytes (1 + rounds rate passes at most, one build, for the packed form the device pack),
"rate_pass_ms" one vnrAmdNeuralVolumeCorrectionRates call over the ladder's 16 tolerances: one evaluation of the network.  The
kernels are correction_rate_coords_kernel, correction_rate_kernel and correction_rate_final_kernel.  With --budget-form coded the call
is vnrAmdNeuralVolumeBuildCorrectionCodedWithinBytes (the coded rate passes, the direct build, the device encode), "rate_pass_ms" is
one vnrAmdNeuralVolumeCorrectionRatesCoded call (correction_rate_coded_kernel, correction_rate_final_coded_kernel) and
"plain_rate_pass_ms" one vnrAmdNeuralVolumeCorrectionRates call, alternating."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instantvnr_amd import api, synthetic as syn  # noqa: E402

FULL_SCALE = {"uint8": 255.0, "int8": 127.0, "uint16": 65535.0, "int16": 32767.0, "uint32": 4294967040.0, "int32": 2147483520.0,
              "float32": 1.0, "float64": 1.0}


def series(size, frames, dtype, seed):
    """frames arrays [z, y, x] of `dtype`: a seeded vortex field moving along x and fading"""
    b = min(size, 64)
    base = syn.vortex_volume(b, seed=seed)
    if size != b:
        idx = np.arange(size) * b // size
        base = base[np.ix_(idx, idx, idx)]
    scale = np.float32(FULL_SCALE[np.dtype(dtype).name])
    for t in range(frames):
        f = np.roll(base, t * max(1, size // 16), axis=2) * np.float32(1.0 - 0.4 * t / max(1, frames))
        yield np.ascontiguousarray((f * scale).astype(dtype))


def with_ghost_layers(a, g):
    """-> (padded array, element offset of the first voxel, strides) for g ghost layers per side"""
    if g == 0:
        return a, 0, None
    p = np.zeros(tuple(s + 2 * g for s in a.shape), a.dtype)
    p[g:-g, g:-g, g:-g] = a
    sy, sz = p.shape[2], p.shape[2] * p.shape[1]
    return p, g + g * sy + g * sz, (1, sy, sz)


def timed(fn, repeat, warmup=0):
    out, times = None, []
    for _ in range(warmup):
        fn()
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, min(times), statistics.median(times)


def round_trip(neural, ptr, dtype, strides, dims, ghost, value_range, repeat, coords):
    """-> the --round-trip columns of one step.  `ptr` is the step's own device array (the reference of the error report)."""
    n = dims[0] * dims[1] * dims[2]
    rep, best, median = timed(lambda: api.vnrNeuralVolumeErrorAgainstDevice(neural, ptr, dtype, strides, None, value_range), repeat, 1)
    row = {"max_abs_error": rep["max_abs"], "worst_voxel": list(rep["worst"]), "mean_abs_error": rep["mean_abs"],
           "psnr_data_units_db": round(rep["psnr_db"], 3), "error_ms": round(best, 4), "error_median_ms": round(median, 4)}
    padded = tuple(d + 2 * ghost for d in dims)
    out = api.DeviceArray((padded[2], padded[1], padded[0]), dtype)     # the array a consumer would hand over, ghost layers included
    first = (ghost + ghost * padded[0] + ghost * padded[0] * padded[1]) * dtype.itemsize
    _, best, median = timed(lambda: api.vnrNeuralVolumeDecodeToDevice(neural, out.ptr + first, dtype, strides, None, None, value_range), repeat, 1)
    out.free()
    row.update(decode_ms=round(best, 4), decode_median_ms=round(median, 4))
    values = api.DeviceArray((n,), np.float32)

    def inference():
        api.check(api.lib().vnrAmdNeuralVolumeInference(neural.h, n, coords.ptr, values.ptr, None))
        api.check(api.lib().vnrAmdSynchronize())
    _, best, median = timed(inference, repeat, 1)
    values.free()
    row.update(inference_ms=round(best, 4), inference_median_ms=round(median, 4), samples=n,
               decode_chunk=int(os.environ.get("VNR_AMD_DECODE_CHUNK", 1 << 22)))
    return row


def error_bound(neural, ptr, dtype, strides, dims, ghost, value_range, eps, repeat, packed=False, resident="fixed", roi=None, step=None, probe=0, seed=1):
    """-> the --error-bound columns of one step.  `ptr` is the step's own device array (the reference of the correction), `step`
    the same voxels on the host (for --roi and --probe)."""
    def build():
        c = api.vnrNeuralVolumeBuildCorrection(neural, ptr, dtype, eps, strides, value_range)
        held.append(c)
        while len(held) > 1:
            held.pop(0).release()
        return c
    held = []
    corr, best, median = timed(build, repeat, 1)
    info = corr.info()
    raw = dims[0] * dims[1] * dims[2] * dtype.itemsize
    n_params = len(api.vnrNeuralVolumeSerializeParams(neural))
    row = {"eps": eps, "raw_bytes": raw, "params_bytes": n_params, "correction_bytes": info["serialized_bytes"],
           "compressed_bytes": n_params + info["serialized_bytes"], "ratio": round(raw / (n_params + info["serialized_bytes"]), 3),
           "flagged_cells": info["n_flagged"], "cells": info["n_cells"], "voxels_over": info["n_voxels_flagged"],
           "max_abs_before": info["max_abs_before"], "max_abs_after": info["max_abs_after"], "build_ms": round(best, 4), "build_median_ms": round(median, 4)}
    padded = tuple(d + 2 * ghost for d in dims)
    out = api.DeviceArray((padded[2], padded[1], padded[0]), dtype)
    first = (ghost + ghost * padded[0] + ghost * padded[0] * padded[1]) * dtype.itemsize
    corr.set_resident_form(resident)      # (the build left the fixed-width codes resident: packed converts them here, once)
    _, best, median = timed(lambda: api.vnrNeuralVolumeDecodeToDeviceCorrected(neural, corr, out.ptr + first, strides), repeat, 1)
    row.update(apply_ms=round(best, 4), apply_median_ms=round(median, 4), resident=resident, device_bytes=corr.residency()["device_bytes"])
    if roi is not None:
        lo, size = roi
        whole = out.numpy()[ghost:ghost + dims[2], ghost:ghost + dims[1], ghost:ghost + dims[0]]
        cut = tuple(slice(lo[a], lo[a] + size[a]) for a in (2, 1, 0))
        box = api.DeviceArray((size[2], size[1], size[0]), dtype)
        _, best, median = timed(lambda: api.vnrNeuralVolumeDecodeToDeviceCorrected(neural, corr, box, box=roi), repeat, 1)
        got = box.numpy()
        worst = float(np.abs(got.astype(np.float64) - step[cut].astype(np.float64)).max())
        row.update(roi=list(lo) + list(size), roi_apply_ms=round(best, 4), roi_apply_median_ms=round(median, 4), roi_max_abs_error=worst,
                   roi_within_bound=bool(worst <= info["max_abs_after"]), roi_equals_whole_grid=bool(np.array_equal(got.view(np.uint8), np.ascontiguousarray(whole[cut]).view(np.uint8))))
        _, best, median = timed(lambda: api.vnrNeuralVolumeDecodeToDevice(neural, box, dtype, None, roi, None, value_range), repeat, 1)
        row.update(roi_plain_decode_ms=round(best, 4), roi_plain_decode_median_ms=round(median, 4))
        box.free()
    if probe:
        rng = np.random.default_rng(seed)
        voxels = np.stack([rng.integers(0, dims[a], probe) for a in range(3)], axis=1).astype(np.int32)
        d_voxels, d_got = api.DeviceArray.from_numpy(voxels), api.DeviceArray((probe,), dtype)
        _, best, median = timed(lambda: api.vnrNeuralVolumeGatherVoxelsCorrected(neural, corr, d_voxels, d_got, verify_params=False), repeat, 1)
        got = d_got.numpy()
        at = (voxels[:, 2], voxels[:, 1], voxels[:, 0])
        whole = out.numpy()[ghost:ghost + dims[2], ghost:ghost + dims[1], ghost:ghost + dims[0]]
        row.update(probe=probe, probe_gather_ms=round(best, 4), probe_gather_median_ms=round(median, 4),
                   probe_max_abs_error=float(np.abs(got.astype(np.float64) - step[at].astype(np.float64)).max()),
                   probe_equals_whole_grid=bool(np.array_equal(got.view(np.uint8), np.ascontiguousarray(whole[at]).view(np.uint8))))
        d_voxels.free(); d_got.free()
        if info["kind"] != 2:
            d_points, d_values = api.DeviceArray.from_numpy(rng.uniform(0.0, 1.0, (probe, 3)).astype(np.float32)), api.DeviceArray((probe,), np.float32)
            _, best, median = timed(lambda: api.vnrNeuralVolumeSampleCorrected(neural, corr, d_points, d_values, verify_params=False), repeat, 1)
            row.update(probe_sample_ms=round(best, 4), probe_sample_median_ms=round(median, 4))
            d_points.free(); d_values.free()
    _, best, median = timed(lambda: api.vnrNeuralVolumeDecodeToDevice(neural, out.ptr + first, dtype, strides, None, None, value_range), repeat, 1)
    row.update(plain_decode_ms=round(best, 4), plain_decode_median_ms=round(median, 4))
    _, best, median = timed(lambda: api.vnrNeuralVolumeErrorAgainstDevice(neural, ptr, dtype, strides, None, value_range), repeat, 1)
    row.update(error_report_ms=round(best, 4), error_report_median_ms=round(median, 4))
    if packed:
        fixed = corr.to_bytes()
        warm = api.Correction.from_bytes(fixed)
        warm.to_packed_bytes()
        warm.release()
        blob, best, _ = timed(corr.to_packed_bytes, 1)
        row.update(packed_correction_bytes=len(blob), fixed_over_packed=round(len(fixed) / len(blob), 3), packed_compressed_bytes=n_params + len(blob),
                   packed_ratio=round(raw / (n_params + len(blob)), 3), pack_ms=round(best, 4))
        times = []
        for _ in range(repeat):
            fresh = api.Correction.from_packed_bytes(blob)
            fresh.set_resident_form(resident)
            times.append(timed(lambda: api.vnrNeuralVolumeDecodeToDeviceCorrected(neural, fresh, out.ptr + first, strides), 1)[1])
            last = fresh.to_bytes() == fixed if len(times) == repeat else None
            fresh.release()
        row.update(packed_first_apply_ms=round(min(times), 4), packed_first_apply_median_ms=round(statistics.median(times), 4), packed_unpacks_to_fixed=last)
    out.free()
    corr.release()
    return row


def direct_build(neural, ptr, dtype, strides, value_range, eps, repeat):
    """-> the --direct columns of one step: vnrAmdNeuralVolumeBuildCorrectionPacked beside vnrAmdNeuralVolumeBuildCorrection followed by
    vnrAmdCorrectionSerializePacked, alternating in this process, max(repeat, 10) samples each after one warm-up each; min and max"""
    def two_calls():
        t0 = time.perf_counter()
        c = api.vnrNeuralVolumeBuildCorrection(neural, ptr, dtype, eps, strides, value_range)
        blob = c.to_packed_bytes()
        return c, blob, (time.perf_counter() - t0) * 1e3, None

    def direct():
        t0 = time.perf_counter()
        c = api.vnrNeuralVolumeBuildCorrectionPacked(neural, ptr, dtype, eps, strides, value_range)
        t1 = time.perf_counter()
        residency = c.residency()                     # (as the call leaves it: before the bytes are asked for)
        t2 = time.perf_counter()
        blob = c.to_packed_bytes()                    # the one download of table plus planes
        return c, blob, (t1 - t0) * 1e3, (t1 - t0 + time.perf_counter() - t2) * 1e3, residency

    times = {"build_pack": [], "direct": [], "direct_and_bytes": []}
    equal, row = True, {}
    for k in range(1 + max(repeat, 10)):
        c2, blob2, ms2, _ = two_calls()
        c1, blob1, ms1, ms1b, residency = direct()
        if k:      # (k == 0 warms both up)
            times["build_pack"].append(ms2); times["direct"].append(ms1); times["direct_and_bytes"].append(ms1b)
        equal = equal and blob1 == blob2
        if k == 0:     # once a step: the fixed-width bytes and the report as well
            equal = equal and c1.to_bytes() == c2.to_bytes() and repr(c1.info()) == repr(c2.info())
            row.update(direct_device_bytes=residency["device_bytes"], build_pack_device_bytes=c2.residency()["device_bytes"],
                       direct_packed_bytes=len(blob1))
        c1.release(); c2.release()
    for name, t in times.items():
        row[name + "_min_ms"], row[name + "_median_ms"], row[name + "_max_ms"] = round(min(t), 4), round(statistics.median(t), 4), round(max(t), 4)
    row.update(direct_samples=len(times["direct"]), direct_equals_build_pack=equal)
    return row


def coded_form(neural, ptr, dtype, strides, dims, ghost, value_range, eps, repeat, resident):
    """-> the --coded columns of one step: the coded form beside the packed form of the correction that
    vnrAmdNeuralVolumeBuildCorrectionPacked leaves resident as bit planes"""
    corr = api.vnrNeuralVolumeBuildCorrectionPacked(neural, ptr, dtype, eps, strides, value_range)
    raw = dims[0] * dims[1] * dims[2] * dtype.itemsize
    n_params = len(api.vnrNeuralVolumeSerializeParams(neural))
    sizes = {"packed": corr.to_packed_device(), "coded": corr.to_coded_device()}
    bufs = {k: api.DeviceArray((max(v, 1),), np.uint8) for k, v in sizes.items()}
    write = {"packed": corr.to_packed_device, "coded": corr.to_coded_device}
    times = {"packed": [], "coded": []}
    for k in range(1 + max(repeat, 10)):      # (k == 0 warms both up)
        for form in ("coded", "packed"):
            t0 = time.perf_counter()
            written = write[form](bufs[form])
            if k:
                times[form].append((time.perf_counter() - t0) * 1e3)
            assert written == sizes[form]
    coded = bufs["coded"].numpy()[:sizes["coded"]].tobytes()
    packed = bufs["packed"].numpy()[:sizes["packed"]].tobytes()
    for b in bufs.values():
        b.free()
    n_flagged = int(np.frombuffer(coded, "<u4", 1, 28)[0])
    cells = np.frombuffer(coded, "<u4", 2 * n_flagged, 104)[0::2].astype(np.int64)
    m = [-(-d // 16) for d in dims]
    extent = lambda d, i: np.minimum(16, d - 16 * i)
    voxels = int((extent(dims[0], cells % m[0]) * extent(dims[1], cells // m[0] % m[1]) * extent(dims[2], cells // (m[0] * m[1]))).sum())
    head = 104 + 8 * n_flagged
    row = {"coded_flagged_cells": n_flagged, "coded_flagged_voxels": voxels, "packed_form_bytes": len(packed), "coded_form_bytes": len(coded),
           "packed_bits_per_flagged_voxel": round(8 * (len(packed) - head) / max(voxels, 1), 4),
           "coded_bits_per_flagged_voxel": round(8 * (len(coded) - head) / max(voxels, 1), 4),
           "packed_form_ratio": round(raw / (n_params + len(packed)), 3), "coded_form_ratio": round(raw / (n_params + len(coded)), 3)}
    for form, t in times.items():
        row.update({f"serialize_{form}_to_device_min_ms": round(min(t), 4), f"serialize_{form}_to_device_median_ms": round(statistics.median(t), 4),
                    f"serialize_{form}_to_device_max_ms": round(max(t), 4)})
    row["serialize_samples"] = len(times["coded"])
    same = packed == corr.to_packed_bytes() and coded == corr.to_coded_bytes()
    # the first corrected decode of a correction read from either form
    padded = tuple(d + 2 * ghost for d in dims)
    out = api.DeviceArray((padded[2], padded[1], padded[0]), dtype)
    first = (ghost + ghost * padded[0] + ghost * padded[0] * padded[1]) * dtype.itemsize
    applies = {"coded": [], "packed": []}
    stored = {}
    for k in range(1 + repeat):
        for form, read, blob in (("coded", api.Correction.from_coded_bytes, coded), ("packed", api.Correction.from_packed_bytes, packed)):
            fresh = read(blob)
            fresh.set_resident_form(resident)
            ms = timed(lambda: api.vnrNeuralVolumeDecodeToDeviceCorrected(neural, fresh, out.ptr + first, strides), 1)[1]
            if k:
                applies[form].append(ms)
            else:
                stored[form] = out.numpy().tobytes()
                if form == "coded":
                    same = same and fresh.to_packed_bytes() == packed
            fresh.release()
    out.free()
    corr.release()
    row.update(coded_first_apply_ms=round(min(applies["coded"]), 4), coded_first_apply_median_ms=round(statistics.median(applies["coded"]), 4),
               packed_first_apply_again_ms=round(min(applies["packed"]), 4), packed_first_apply_again_median_ms=round(statistics.median(applies["packed"]), 4),
               coded_reads_back_to_packed=bool(same), coded_decodes_like_packed=stored["coded"] == stored["packed"])
    return row


def byte_budget(neural, ptr, dtype, strides, dims, value_range, max_bytes, form, rounds, repeat):
    """-> the --byte-budget columns of one step.  `ptr` is the step's own device array (the reference of the correction)."""
    eps_hi = api.vnrNeuralVolumeErrorAgainstDevice(neural, ptr, dtype, strides, None, value_range)["max_abs"]
    raw = dims[0] * dims[1] * dims[2] * dtype.itemsize
    n_params = len(api.vnrNeuralVolumeSerializeParams(neural))
    row = {"byte_budget": max_bytes, "budget_form": form, "budget_rounds": rounds, "eps_hi": eps_hi, "raw_bytes": raw, "params_bytes": n_params}
    if not eps_hi > 0:      # the decode is exact already: there is no ladder below 0
        return row
    held = []

    def build():
        c, rep = api.vnrNeuralVolumeBuildCorrectionWithinBytes(neural, ptr, dtype, max_bytes, eps_hi, form, rounds, strides, value_range)
        held.append(c)
        while len(held) > 1:
            held.pop(0).release()
        return c, rep
    try:
        (corr, rep), best, median = timed(build, repeat, 1)
    except api.VnrAmdError as e:      # not even eps_hi fits
        row["budget_refused"] = str(e)
        return row
    blob = corr.to_coded_bytes() if form == "coded" else (corr.to_packed_bytes() if form == "packed" else corr.to_bytes())      # what is stored
    row.update(budget_eps=rep["eps"], budget_bytes=rep["bytes"], serialized_equals_report=len(blob) == rep["bytes"], eps_tighter=rep["eps_tighter"],
               bytes_tighter=rep["bytes_tighter"], rate_passes=rep["rate_passes"], compressed_bytes=n_params + rep["bytes"],
               ratio=round(raw / (n_params + rep["bytes"]), 3), max_abs_after=corr.info()["max_abs_after"], budget_ms=round(best, 4),
               budget_median_ms=round(median, 4))
    corr.release()
    ladder = [eps_hi * 2.0 ** -j for j in range(16)]
    if form == "coded":      # the coded rate call beside the plain one, alternating; and what the packed form needs at the chosen tolerance
        at = api.vnrNeuralVolumeCorrectionRates(neural, ptr, dtype, [rep["eps"]], strides, value_range, coded=True)[0]
        row.update(rate_equals_report=at["coded_serialized_bytes"] == rep["bytes"], packed_bytes_at_budget_eps=at["packed_serialized_bytes"])
        samples = {True: [], False: []}
        for i in range(2 * (max(repeat, 10) + 1)):
            coded = i % 2 == 0
            t0 = time.perf_counter()
            api.vnrNeuralVolumeCorrectionRates(neural, ptr, dtype, ladder, strides, value_range, coded=coded)
            if i >= 2:      # (one warm-up each)
                samples[coded].append((time.perf_counter() - t0) * 1e3)
        row.update(rate_pass_ms=round(min(samples[True]), 4), rate_pass_median_ms=round(statistics.median(samples[True]), 4),
                   plain_rate_pass_ms=round(min(samples[False]), 4), plain_rate_pass_median_ms=round(statistics.median(samples[False]), 4))
        return row
    _, best, median = timed(lambda: api.vnrNeuralVolumeCorrectionRates(neural, ptr, dtype, ladder, strides, value_range), repeat, 1)
    row.update(rate_pass_ms=round(best, 4), rate_pass_median_ms=round(median, 4))
    return row


def guided(a):
    """the --guided run: the same field, model and seeds trained with error-guided and with uniform batches, side by side"""
    dims = (a.size,) * 3
    f = syn.analytic_volume(a.size)
    f = (f - f.min()) / (f.max() - f.min())
    field = api.DeviceArray.from_numpy(np.clip(np.float32(1.6) * f - np.float32(0.3), 0, 1).astype(np.float32))
    before = os.environ.get("VNR_AMD_INIT_SEED")
    os.environ["VNR_AMD_INIT_SEED"] = str(1000 + a.seed)      # both models start from the same parameters
    runs = {}
    for name in ("guided", "uniform"):
        volume, _ = api.vnrCreateSimpleVolumeFromDevice(field.ptr, dims, np.float32, None, (0.0, 1.0))
        neural = api.vnrCreateNeuralVolume(syn.model_config(n_levels=8, n_features=8, log2_hashmap_size=15, base_resolution=16), volume)
        api.check(api.lib().vnrAmdNeuralVolumeSetSamplerSeed(neural.h, a.seed, 1))
        runs[name] = (volume, neural)
    if before is None:
        os.environ.pop("VNR_AMD_INIT_SEED", None)
    else:
        os.environ["VNR_AMD_INIT_SEED"] = before
    print(f"library build {api.lib().vnrAmdBuildId().decode()}; --guided: {a.size}^3 float32 blob field, {a.steps_per_frame} steps, "
          f"refresh every {a.refresh_every}, uniform fraction {a.uniform_fraction}")
    done = 0
    while done < a.steps_per_frame:
        steps = min(a.refresh_every, a.steps_per_frame - done)
        row = {"steps": done + steps}
        for name, (volume, neural) in runs.items():
            t0 = time.perf_counter()
            api.vnrNeuralVolumeTrain(neural, steps, True)
            api.check(api.lib().vnrAmdSynchronize())
            row[name + "_train_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            t0 = time.perf_counter()
            if name == "guided":     # the report and the new weight map in one call
                rep = api.neural_volume_guide_sampling_by_error(neural, a.uniform_fraction)
            else:
                rep = api.vnrNeuralVolumeErrorAgainstDevice(neural, api.lib().vnrAmdSimpleVolumeDeviceData(volume.h), np.float32)
            row[name + "_report_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            row[name + "_max_abs_error"] = rep["max_abs"]
            row[name + "_psnr_db"] = round(rep["psnr_db"], 3)
        done += steps
        print(json.dumps(row))
    field.free()
    return 0


def main(argv=None):
    p = argparse.ArgumentParser(description="in-situ training of a time series from device memory")
    p.add_argument("--size", type=int, default=64)
    p.add_argument("--dtype", default="uint8", choices=sorted(FULL_SCALE))
    p.add_argument("--frames", type=int, default=4)
    p.add_argument("--steps-per-frame", type=int, default=100)
    p.add_argument("--ghost", type=int, default=0)
    p.add_argument("--range-from-data", action="store_true")
    p.add_argument("--repeat", type=int, default=5)
    p.add_argument("--compare-host", action="store_true")
    p.add_argument("--round-trip", action="store_true")
    p.add_argument("--error-bound", type=float, default=None, metavar="EPS")
    p.add_argument("--packed", action="store_true")
    p.add_argument("--direct", action="store_true")
    p.add_argument("--coded", action="store_true")
    p.add_argument("--resident", default="fixed", choices=["fixed", "packed"])
    p.add_argument("--roi", default=None, metavar="x0,y0,z0,sx,sy,sz")
    p.add_argument("--probe", type=int, default=0, metavar="N")
    p.add_argument("--byte-budget", type=int, default=None, metavar="BYTES")
    p.add_argument("--budget-form", default="packed", choices=["fixed", "packed", "coded"])
    p.add_argument("--budget-rounds", type=int, default=2, metavar="N")
    p.add_argument("--guided", action="store_true")
    p.add_argument("--uniform-fraction", type=float, default=0.25)
    p.add_argument("--refresh-every", type=int, default=100)
    p.add_argument("--seed", type=int, default=1)
    a = p.parse_args(argv)
    if a.guided and (a.steps_per_frame <= 0 or a.refresh_every <= 0 or not 0.0 <= a.uniform_fraction <= 1.0):
        p.error("--guided needs --steps-per-frame > 0, --refresh-every > 0 and --uniform-fraction in [0, 1]")
    if a.round_trip and not a.steps_per_frame:
        p.error("--round-trip needs a trained network: --steps-per-frame > 0")
    if a.error_bound is not None and (not a.steps_per_frame or not a.error_bound >= 0.0 or a.error_bound == float("inf")):
        p.error("--error-bound needs a trained network (--steps-per-frame > 0) and a finite EPS >= 0")
    if (a.packed or a.direct or a.coded) and a.error_bound is None:
        p.error("--packed, --direct and --coded need --error-bound EPS")
    if a.byte_budget is not None and (not a.steps_per_frame or a.byte_budget < 0 or not 0 <= a.budget_rounds <= 8):
        p.error("--byte-budget needs a trained network (--steps-per-frame > 0), BYTES >= 0 and --budget-rounds 0 .. 8")
    roi = None
    if a.roi is not None or a.resident != "fixed" or a.probe:
        if a.error_bound is None or a.probe < 0:
            p.error("--resident, --roi and --probe N (N > 0) need --error-bound EPS")
    if a.roi is not None:
        try:
            v = [int(x) for x in a.roi.split(",")]
        except ValueError:
            v = []
        if len(v) != 6 or min(v[:3]) < 0 or min(v[3:]) <= 0 or any(v[k] + v[3 + k] > a.size for k in range(3)):
            p.error(f"--roi needs x0,y0,z0,sx,sy,sz: a box with positive sizes inside the {a.size}^3 grid")
        roi = (tuple(v[:3]), tuple(v[3:]))

    api._lib.require_device()
    api.check(api.lib().vnrAmdInit(-1))
    if a.guided:
        return guided(a)
    dtype = np.dtype(a.dtype)
    dims = (a.size,) * 3
    n = a.size ** 3
    value_range = None if a.range_from_data else (0.0, FULL_SCALE[a.dtype])
    passes = 2 if a.range_from_data else 1
    bytes_read, bytes_written = passes * n * dtype.itemsize, 4 * n
    print(f"library build {api.lib().vnrAmdBuildId().decode()}; {a.size}^3 {a.dtype}, ghost {a.ghost}, range "
          f"{'from the data' if a.range_from_data else value_range}, ingest reads {bytes_read} B and writes {bytes_written} B")

    volume = neural = coords = None
    if a.round_trip:     # ready-made coordinates for the plain inference: the voxel centres, x fastest (12 bytes per voxel)
        c = (np.arange(a.size, dtype=np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(a.size))
        host = np.empty((a.size, a.size, a.size, 3), np.float32)
        host[..., 0], host[..., 1], host[..., 2] = c[None, None, :], c[None, :, None], c[:, None, None]
        coords = api.DeviceArray.from_numpy(host.reshape(-1, 3))
        del host
    for t, step in enumerate(series(a.size, a.frames, dtype, a.seed)):
        source, offset, strides = with_ghost_layers(step, a.ghost)
        d = api.DeviceArray.from_numpy(source)              # the "simulation output": typed voxels in device memory
        ptr = d.ptr + offset * dtype.itemsize
        row = {"step": t}
        if volume is None:
            (volume, used), row["create_ms"], _ = timed(lambda: api.vnrCreateSimpleVolumeFromDevice(ptr, dims, dtype, strides, value_range), 1)
            if a.steps_per_frame:
                neural = api.vnrCreateNeuralVolume(syn.model_config(n_levels=8, n_features=8, log2_hashmap_size=15, base_resolution=16), volume)
        else:
            (_, used), best, median = timed(lambda: api.vnrSimpleVolumeUpdateFromDevice(volume, ptr, dtype, strides, value_range), a.repeat)
            _, mc_best, mc_median = timed(lambda: api.vnrSimpleVolumeSetCurrentTimeStep(volume, 0), a.repeat)
            ingest = max(best - mc_best, 1e-6)
            row.update(update_ms=round(best, 4), update_median_ms=round(median, 4), macrocell_ms=round(mc_best, 4),
                       macrocell_median_ms=round(mc_median, 4), ingest_ms=round(ingest, 4),
                       ingest_GBps=round((bytes_read + bytes_written) / ingest / 1e6, 1))
        row["used_range"] = used
        if a.compare_host:
            host, row["host_create_ms"], row["host_create_median_ms"] = timed(lambda: api.vnrCreateSimpleVolume(step, value_range=value_range),
                                                                               1 if t == 0 else min(a.repeat, 3))
            host.release()
        if neural is not None:
            t0 = time.perf_counter()
            api.vnrNeuralVolumeTrain(neural, a.steps_per_frame, True)
            row["train_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            row["psnr"] = round(api.vnrNeuralVolumeGetPSNR(neural), 3)
            if a.round_trip:     # in data units: the range that was applied inverts the ingest
                row.update(round_trip(neural, ptr, dtype, strides, dims, a.ghost, used, a.repeat, coords))
            if a.error_bound is not None:
                row.update(error_bound(neural, ptr, dtype, strides, dims, a.ghost, used, a.error_bound, a.repeat, a.packed, a.resident, roi, step, a.probe, a.seed))
                if a.direct:
                    row.update(direct_build(neural, ptr, dtype, strides, used, a.error_bound, a.repeat))
                if a.coded:
                    row.update(coded_form(neural, ptr, dtype, strides, dims, a.ghost, used, a.error_bound, a.repeat, a.resident))
            if a.byte_budget is not None:
                row.update(byte_budget(neural, ptr, dtype, strides, dims, used, a.byte_budget, a.budget_form, a.budget_rounds, a.repeat))
        d.free()
        for k in ("create_ms", "host_create_ms", "host_create_median_ms"):
            if k in row:
                row[k] = round(row[k], 4)
        print(json.dumps(row))
    return 0


if __name__ == "__main__":
    sys.exit(main())
