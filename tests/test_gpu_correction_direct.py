"""Corrections built straight into bit planes (include/vnr_amd.h, "corrections built straight into bit planes"; the direct build of
csrc/correction.hip, its host step csrc/correction_direct.cpp) against the numpy restatements tests/error_bound_ref.py,
tests/correction_pack_ref.py and tests/correction_index_ref.py, and against vnrNeuralVolumeBuildCorrection of the same arguments.
Codes, counts and sizes are integers, the reports are single double operations and maxima: every comparison has tolerance ZERO.

The setup is the one of tests/test_gpu_correction_rate.py, restated: the trained (40, 24, 20) volume (ragged upper faces, clean cells,
codes of 1, 2 and 4 bytes) and a (21, 10, 3) one whose cells have 480 and 150 voxels (cx = 5: groups that straddle rows, short last
groups), and references that are the decoded field perturbed."""
import functools
import math
import os
import sys

import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correction_index_ref as cir  # noqa: E402
import correction_pack_ref as cpr  # noqa: E402
import error_bound_ref as ebr  # noqa: E402

pytestmark = pytest.mark.gpu

DIMS = (40, 24, 20)
TAIL_DIMS = (21, 10, 3)
ALL_DIMS = [DIMS, TAIL_DIMS]
DIMS_IDS = ["40x24x20", "21x10x3"]
# (dtype, eps): kind 1, kind 0 of a narrow and of a wide type, kind 2 with 64-bit patterns
TYPES = [(np.float32, 1e-3), (np.int16, 2), (np.uint32, 1), (np.float64, 0)]
TYPE_IDS = [t.__name__ for t, _ in TYPES]
RANGES = {np.int16: (-30000.0, 30000.0), np.uint32: (0.0, 4.0e9), np.float32: (-3.5, 12.25), np.float64: (-1.0e3, 2.5e3)}
LAYOUTS = ("dense", "gather", "ghost")
# (lower, size): aligned to nothing; the ragged upper faces only.  On the small volume: straddles the ragged cell of cx = 5
BOXES = {DIMS: [((3, 5, 1), (30, 13, 11)), ((32, 0, 16), (8, 24, 4))], TAIL_DIMS: [((2, 1, 0), (18, 8, 3))]}


def ground_truth(dims):
    z0, y0 = (40 - dims[2]) // 2, (40 - dims[1]) // 2
    a = syn.analytic_volume(40)[z0:z0 + dims[2], y0:y0 + dims[1], :dims[0]]
    a = (a - a.min()) / (a.max() - a.min())
    return np.clip(np.float32(1.6) * a - np.float32(0.3), 0, 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def trained(dims):
    """-> (simple volume, neural volume) with fixed seeds, 400 steps (10 for the small one); shared and left unchanged"""
    before = {k: os.environ.get(k) for k in ("VNR_AMD_INIT_SEED", "VNR_AMD_DECODE_CHUNK")}
    os.environ["VNR_AMD_INIT_SEED"] = "4711"
    os.environ.pop("VNR_AMD_DECODE_CHUNK", None)
    try:
        sv = api.vnrCreateSimpleVolume(ground_truth(dims), value_range=(0.0, 1.0))
        cfg = syn.model_config(n_levels=4, n_features=2, log2_hashmap_size=12, base_resolution=4, n_neurons=16, n_hidden_layers=1)
        nv = api.vnrCreateNeuralVolume(cfg, sv)
        api.check(api.lib().vnrAmdNeuralVolumeSetSamplerSeed(nv.h, 99, 7))
        api.vnrNeuralVolumeTrain(nv, 400 if dims == DIMS else 10, True)
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return sv, nv


def sentinel(dtype):
    return np.frombuffer(b"\xa5" * np.dtype(dtype).itemsize, dtype)[0]


def layout(kind, size):
    """-> (elements of the array, element offset of the first voxel, strides or None)"""
    bx, by, bz = size
    if kind == "dense":
        return bx * by * bz, 0, None
    if kind == "gather":                                    # sx = 2: one voxel at a time
        sy, sz = 2 * bx + 3, (2 * bx + 3) * (by + 1)
        return sz * (bz + 1), 1 + sy, (2, sy, sz)
    sy, sz = bx + 5, (bx + 5) * (by + 3)
    return sz * (bz + 2), 2 + sy + sz, (1, sy, sz)


def box_view(flat, offset, strides, size):
    bx, by, bz = size
    sx, sy, sz = strides or (1, bx, bx * by)
    it = flat.dtype.itemsize
    return np.lib.stride_tricks.as_strided(flat[offset:], shape=(bz, by, bx), strides=(sz * it, sy * it, sx * it))


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def box_slice(a, box):
    (x, y, z), (sx, sy, sz) = box
    return a[z:z + sz, y:y + sy, x:x + sx]


@functools.lru_cache(maxsize=None)
def decoded(dtype, dims):
    """what vnrAmdNeuralVolumeDecodeToDevice stores, [z, y, x]; computed once, read only"""
    d = api.DeviceArray((dims[0] * dims[1] * dims[2],), dtype)
    api.vnrNeuralVolumeDecodeToDevice(trained(dims)[1], d, dtype, value_range=RANGES[dtype])
    out = d.numpy().reshape(dims[::-1])
    d.free()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def params_id(dims):
    p = api.neural_get_params_fp16(trained(dims)[1])
    return ebr.fnv1a64(np.ascontiguousarray(p).tobytes()), int(p.size)


@functools.lru_cache(maxsize=None)
def reference(dtype, eps, dims):
    """the decoded field perturbed: codes of a few -3 .. 3 among zeros where x < 16 (none at all from z = 16 on: clean cells),
    thousands where 16 <= x < 32, millions (a 16-bit type: hundreds) beyond; eps == 0: +0.0 in the slice z = 0 from x = 16 on"""
    dec = decoded(dtype, dims)
    rng = np.random.default_rng(dims[0] + np.dtype(dtype).itemsize)
    wide = np.dtype(dtype).itemsize > 2
    x = np.arange(dims[0])
    scale = np.where(x < 16, 1.0, np.where(x < 32, 6000.0 if wide else 1000.0, 3.0e6 if wide else 300.0))
    q = np.rint(rng.normal(0.0, 1.0, dec.shape) * scale).astype(np.int64)
    q[:, :, :16] *= rng.uniform(size=dec.shape)[:, :, :16] < 0.03
    q[16:, :, :16] = 0
    q[0, 0, 0] = -1
    if np.dtype(dtype).kind == "f":
        ref = (dec.astype(np.float64) + q * (2.0 * eps if eps > 0 else 1.0e-3)).astype(dtype)
        if eps == 0:
            ref[0, :, 16:] = 0.0
    else:
        info = np.iinfo(dtype)
        ref = np.clip(dec.astype(np.int64) + q * (2 * int(eps) + 1), info.min, info.max).astype(dtype)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def top_error(dtype, eps, dims):
    return float(np.abs(reference(dtype, eps, dims).astype(np.float64) - decoded(dtype, dims).astype(np.float64)).max())


@functools.lru_cache(maxsize=None)
def expected(dtype, eps, dims, build_eps=None):
    """-> (fixed-width blob of numpy's build of reference() at build_eps (None: eps), its packed form, the corrected array by
    error_bound_ref.apply); computed once, read only"""
    h, n = params_id(dims)
    dec = decoded(dtype, dims)
    blob = ebr.build(dec.copy(), reference(dtype, eps, dims).copy(), eps if build_eps is None else build_eps, RANGES[dtype], params_hash=h, n_params=n)["bytes"]
    corrected = ebr.apply(dec.copy(), blob)
    corrected.setflags(write=False)
    return blob, cpr.pack(blob), corrected


def device_reference(ref, kind):
    """-> (device array, its host copy, address of the first voxel, strides): ref [z, y, x] in an array of sentinels"""
    dims = ref.shape[::-1]
    n, offset, strides = layout(kind, dims)
    host = np.full(n, sentinel(ref.dtype), ref.dtype)
    box_view(host, offset, strides, dims)[...] = ref
    d = api.DeviceArray.from_numpy(host)
    return d, host, d.ptr + offset * host.dtype.itemsize, strides


def build_both(dtype, eps, dims, kind="ghost", ref=None, build_eps=None, direct_only=False):
    """-> (the direct build, vnrNeuralVolumeBuildCorrection of the same arguments) against reference() in layout `kind`; the bytes of
    the reference array, ghost layers included, are unchanged by either"""
    nv = trained(dims)[1]
    e = eps if build_eps is None else build_eps
    d, host, ptr, strides = device_reference(reference(dtype, eps, dims) if ref is None else ref, kind)
    try:
        direct = api.vnrNeuralVolumeBuildCorrectionPacked(nv, ptr, dtype, e, strides, RANGES[dtype])
        assert np.array_equal(d.numpy().view(np.uint8), host.view(np.uint8)), "the direct build wrote into the reference array"
        two = None if direct_only else api.vnrNeuralVolumeBuildCorrection(nv, ptr, dtype, e, strides, RANGES[dtype])
        return direct, two
    finally:
        d.free()


def same_info(a, b):
    """field by field; a NaN equals a NaN"""
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, float) and math.isnan(x):
            assert isinstance(y, float) and math.isnan(y), (k, x, y)
        else:
            assert x == y, (k, x, y)
    return True


def packed_residency(packed, dims):
    payload = cpr.split(packed, b"VNRCORP1")[0][15]
    n_groups = len(cir.index(packed)["group_word"])
    n_cells = int(np.prod([-(-d // 16) for d in dims]))
    return {"form": "packed", "on_device": True, "payload_device_bytes": payload, "index_device_bytes": 4 * n_groups + 16 * n_cells,
            "device_bytes": payload + 4 * n_groups + 16 * n_cells}


def device_apply(corr, dtype, kind, dims, box=None):
    """one corrected decode of `box` (None: the whole grid) into an array of sentinels -> (the whole destination after the call, the
    same as it was before, offset, strides)"""
    size = box[1] if box else dims
    n, offset, strides = layout(kind, size)
    before = np.full(n, sentinel(dtype), dtype)
    d = api.DeviceArray.from_numpy(before)
    try:
        api.vnrNeuralVolumeDecodeToDeviceCorrected(trained(dims)[1], corr, d.ptr + offset * before.dtype.itemsize, strides, box=box)
        return d.numpy(), before, offset, strides
    finally:
        d.free()


def check_box(corr, dtype, eps, kind, dims, box):
    """the decode of `box` equals the slice of error_bound_ref.apply, and the ghost layers keep their sentinel"""
    got, expect, offset, strides = device_apply(corr, dtype, kind, dims, box)
    size = box[1] if box else dims
    want = expected(dtype, eps, dims)[2]
    box_view(expect, offset, strides, size)[...] = box_slice(want, box) if box else want
    assert same_bytes(got, expect), (dtype, kind, box, corr.residency())
    return got


# ------------------------------------------------------------------------------------------------ 0. the inputs
def test_the_inputs_have_every_case_the_direct_build_can_meet():
    widths, wide_groups = set(), 0
    for dtype, eps in TYPES:
        blob, packed, _ = expected(dtype, eps, DIMS)
        f, cells, _ = cpr.split(blob, b"VNRCORR1")
        ix = cir.index(packed)
        widths.update((f[10], w) for _, w in cells)
        assert 0 < len(cells) < 12, dtype                                                              # unflagged cells
        assert list(ix["nbits"]).count(0) > 0, dtype                                                   # a flagged cell with a group of zeros
        wide_groups += int((ix["nbits"] >= 17).sum())
        # the small volume: both cells flagged, and a short last group whose last valid lane holds a nonzero code
        blob, packed, _ = expected(dtype, eps, TAIL_DIMS)
        f, cells, _ = cpr.split(blob, b"VNRCORR1")
        voxels = [cpr.cell_voxels(TAIL_DIMS, c) for c, _ in cells]
        assert voxels == [480, 150] and all(v % 64 for v in voxels)
        ix = cir.index(packed)
        assert any(cir.code_at(ix, i, v - 1) != 0 for i, v in enumerate(voxels)), dtype
    assert widths >= {(1, 1), (1, 2), (1, 4), (0, 1), (0, 2), (0, 4), (2, 8)}, widths
    assert wide_groups > 0
    # float64, eps 0: ref's +0.0 slice gives z == 0 where the voxel differs, and groups of nbits 0 inside flagged cells
    dec, ref = decoded(np.float64, DIMS), reference(np.float64, 0, DIMS)
    assert ((ebr.bits(ref) == 0) & (ebr.bits(dec) != 0)).any()


# ------------------------------------------------------------------------------------------------ 1. bytes, info, residency
@pytest.mark.parametrize("dims", ALL_DIMS, ids=DIMS_IDS)
@pytest.mark.parametrize("dtype,eps", TYPES, ids=TYPE_IDS)
def test_bytes_info_and_residency_equal_numpy_and_the_build(dtype, eps, dims, monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    blob, packed, _ = expected(dtype, eps, dims)
    for kind in LAYOUTS:
        direct, two = build_both(dtype, eps, dims, kind)
        want_residency = packed_residency(packed, dims)
        assert direct.residency() == want_residency, kind                   # directly after the call
        info = direct.info()
        assert direct.residency() == want_residency                         # info() moves nothing
        assert same_info(info, two.info()), kind
        assert info["n_flagged"] > 0 and info["payload_bytes"] == cpr.split(blob, b"VNRCORR1")[0][15] and info["serialized_bytes"] == len(blob)
        assert direct.to_packed_bytes() == packed == two.to_packed_bytes(), kind
        assert direct.to_bytes() == blob == two.to_bytes(), kind
        assert direct.residency() == want_residency and same_info(direct.info(), info)
        direct.release(); two.release()


# ------------------------------------------------------------------------------------------------ 2. the corrected decode
@pytest.mark.parametrize("dims", ALL_DIMS, ids=DIMS_IDS)
@pytest.mark.parametrize("dtype,eps", TYPES, ids=TYPE_IDS)
def test_corrected_decode_of_grid_and_boxes_equals_numpy_and_the_build(dtype, eps, dims, monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    direct, two = build_both(dtype, eps, dims)
    for kind in ("dense", "ghost"):
        for box in [None] + BOXES[dims]:
            got = check_box(direct, dtype, eps, kind, dims, box)            # reads the index the device built
            assert same_bytes(got, device_apply(two, dtype, kind, dims, box)[0]), (kind, box)
    assert direct.residency() == packed_residency(expected(dtype, eps, dims)[1], dims)
    assert not same_bytes(expected(dtype, eps, dims)[2], decoded(dtype, dims))
    direct.release(); two.release()


# ------------------------------------------------------------------------------------------------ 3. chunks
@pytest.mark.parametrize("dims", ALL_DIMS, ids=DIMS_IDS)
@pytest.mark.parametrize("dtype,eps", TYPES, ids=TYPE_IDS)
def test_the_direct_build_does_not_depend_on_the_chunk_size(dtype, eps, dims, monkeypatch):
    blob, packed, _ = expected(dtype, eps, dims)
    infos = []
    for chunk in (None, 64, 4160):                              # the default; one group a chunk; a chunk that ends inside a cell
        if chunk is None:
            monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
        else:
            monkeypatch.setenv("VNR_AMD_DECODE_CHUNK", str(chunk))
        direct, _ = build_both(dtype, eps, dims, direct_only=True)
        infos.append(direct.info())
        assert direct.to_packed_bytes() == packed and direct.to_bytes() == blob, chunk
        assert same_info(infos[-1], infos[0]), chunk
        direct.release()


# ------------------------------------------------------------------------------------------------ 4. form changes
@pytest.mark.parametrize("dtype,eps", TYPES, ids=TYPE_IDS)
def test_form_changes_of_a_direct_build_keep_results_and_bytes(dtype, eps, monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    blob, packed, _ = expected(dtype, eps, DIMS)
    direct, _ = build_both(dtype, eps, DIMS, direct_only=True)
    first = check_box(direct, dtype, eps, "ghost", DIMS, None)
    direct.set_resident_form("fixed")                            # unpacks on the device; the planes are released
    fixed_bytes = cpr.split(blob, b"VNRCORR1")[0][15]
    assert direct.residency() == {"form": "fixed", "on_device": True, "payload_device_bytes": fixed_bytes, "index_device_bytes": 0,
                                  "device_bytes": fixed_bytes + 16 * 12}
    assert same_bytes(check_box(direct, dtype, eps, "ghost", DIMS, None), first)
    assert same_bytes(check_box(direct, dtype, eps, "dense", DIMS, BOXES[DIMS][0]), box_slice(expected(dtype, eps, DIMS)[2], BOXES[DIMS][0]).ravel())
    direct.set_resident_form("packed")
    assert direct.residency() == packed_residency(packed, DIMS)
    assert same_bytes(check_box(direct, dtype, eps, "ghost", DIMS, None), first)
    assert direct.to_packed_bytes() == packed and direct.to_bytes() == blob
    direct.release()


# ------------------------------------------------------------------------------------------------ 5. special cases
@pytest.mark.parametrize("dtype,eps", TYPES, ids=TYPE_IDS)
def test_a_tolerance_above_the_largest_error_gives_an_empty_correction(dtype, eps, monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    loose = 2.0 * top_error(dtype, eps, DIMS) + 1.0
    blob, packed, corrected = expected(dtype, eps, DIMS, loose)
    assert cpr.split(blob, b"VNRCORR1")[1] == [] and same_bytes(corrected, decoded(dtype, DIMS))
    direct, two = build_both(dtype, eps, DIMS, build_eps=loose)
    r = direct.residency()
    assert (r["on_device"], r["device_bytes"], r["payload_device_bytes"], r["index_device_bytes"]) == (False, 0, 0, 0)
    assert same_info(direct.info(), two.info()) and direct.info()["n_flagged"] == 0
    assert direct.to_bytes() == blob == two.to_bytes() and direct.to_packed_bytes() == packed == two.to_packed_bytes()
    got, expect, offset, strides = device_apply(direct, dtype, "ghost", DIMS)
    box_view(expect, offset, strides, DIMS)[...] = decoded(dtype, DIMS)       # the plain decode
    assert same_bytes(got, expect)
    assert direct.to_packed_device() == len(packed) == 104
    direct.release(); two.release()


def test_an_all_nan_reference_gives_nan_reports_as_the_build_does(monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    dtype, eps = TYPES[0]
    ref = np.full(DIMS[::-1], np.nan, dtype)
    direct, two = build_both(dtype, eps, DIMS, ref=ref)
    info = direct.info()
    assert same_info(info, two.info())
    assert math.isnan(info["max_abs_before"]) and math.isnan(info["max_abs_after"]) and info["n_nan"] == DIMS[0] * DIMS[1] * DIMS[2]
    assert info["n_flagged"] == 0 and info["worst_after"] == (-1, -1, -1)
    assert direct.to_bytes() == two.to_bytes() and direct.to_packed_bytes() == two.to_packed_bytes()
    direct.release(); two.release()


@pytest.mark.parametrize("dtype,eps", [TYPES[0], TYPES[3]], ids=[TYPE_IDS[0], TYPE_IDS[3]])
def test_a_code_of_2_to_the_32_is_refused_with_the_builds_message(dtype, eps, monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    nv = trained(DIMS)[1]
    tight = math.ldexp(top_error(dtype, eps, DIMS), -33)          # the largest residual quantises to 2^32
    d, host, ptr, strides = device_reference(reference(dtype, eps, DIMS), "ghost")
    try:
        with pytest.raises(api.VnrAmdError) as by_direct:
            api.vnrNeuralVolumeBuildCorrectionPacked(nv, ptr, dtype, tight, strides, RANGES[dtype])
        with pytest.raises(api.VnrAmdError) as by_build:
            api.vnrNeuralVolumeBuildCorrection(nv, ptr, dtype, tight, strides, RANGES[dtype])
        assert str(by_direct.value) == str(by_build.value) and "codes wider than 32 bits" in str(by_direct.value)
        ok = api.vnrNeuralVolumeBuildCorrectionPacked(nv, ptr, dtype, eps, strides, RANGES[dtype])      # a valid call after it
        assert ok.to_packed_bytes() == expected(dtype, eps, DIMS)[1]
        ok.release()
        assert np.array_equal(d.numpy().view(np.uint8), host.view(np.uint8))
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------ 6. the packed bytes in device memory
@pytest.mark.parametrize("dims", ALL_DIMS, ids=DIMS_IDS)
@pytest.mark.parametrize("dtype,eps", TYPES, ids=TYPE_IDS)
def test_to_packed_device_writes_the_packed_bytes(dtype, eps, dims, monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    packed = expected(dtype, eps, dims)[1]
    direct, two = build_both(dtype, eps, dims)
    for corr in (direct, two):                                  # planes resident: device to device; FIXED form: the device pack first
        assert corr.to_packed_device() == len(packed)            # None gives the size
        fill = np.full(len(packed) + 24, 0xa5, np.uint8)
        d = api.DeviceArray.from_numpy(fill)
        try:
            with pytest.raises(api.VnrAmdError) as short:
                corr.to_packed_device((d.ptr, len(packed) - 1))
            assert "capacity" in str(short.value) and str(len(packed)) in str(short.value)
            assert np.array_equal(d.numpy(), fill)               # nothing was written
            assert corr.to_packed_device(d) == len(packed)
            got = d.numpy()
            assert got[:len(packed)].tobytes() == packed and np.array_equal(got[len(packed):], fill[len(packed):])
        finally:
            d.free()
        assert corr.to_packed_bytes() == packed
    assert direct.residency() == packed_residency(packed, dims)
    direct.release(); two.release()
