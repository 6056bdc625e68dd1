"""The corrected decode of a box and the packed resident form (include/vnr_amd.h, "corrected decode of a box, and the resident form
of a correction"; correction_apply_planes_kernel and the box offset of correction_apply_kernel, csrc/correction.hip) against the
numpy restatements tests/error_bound_ref.py, tests/correction_pack_ref.py and tests/correction_index_ref.py.  Bits are moved and
the arithmetic of the header is applied: every comparison has tolerance ZERO.

The setup is the one of tests/test_gpu_correction_pack.py, restated: the trained (40, 24, 20) volume and a (21, 10, 3) one whose
cells have 480 and 150 voxels (cx = 5: groups that straddle rows, 16-byte pieces that straddle groups), references that are the
decoded field perturbed so that codes of 1, 2 and 4 bytes, 64-bit patterns and groups of zeros occur, and, as in
correction_pack_cases.fields, no residual at all where x < 16 and z >= 16: clean cells.  expected = error_bound_ref.apply of the
whole decoded grid; a box's result is its slice."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correction_index_ref as cir  # noqa: E402
import correction_pack_cases as cases  # noqa: E402
import correction_pack_ref as cpr  # noqa: E402
import error_bound_ref as ebr  # noqa: E402

pytestmark = pytest.mark.gpu

DIMS = (40, 24, 20)
TAIL_DIMS = (21, 10, 3)
# (dtype, eps): kind 1, kind 0 of a narrow and of a wide type, kind 2 with 64-bit patterns
APPLY_TYPES = [(np.float32, 1e-3), (np.int16, 2), (np.uint32, 1), (np.float64, 0)]
TYPE_IDS = [f"{t.__name__}-{e}" for t, e in APPLY_TYPES]
RANGES = {np.int16: (-30000.0, 30000.0), np.uint32: (0.0, 4.0e9), np.float32: (-3.5, 12.25), np.float64: (-1.0e3, 2.5e3)}
FORMS = ["fixed", "packed"]
CLEAN_BOX = ((0, 0, 16), (16, 24, 4))          # x < 16, z >= 16: cells 6 and 9 of the 3 x 2 x 2
# (lower, size) on DIMS: aligned to no cell and to no 16-byte piece; inside one cell; one voxel, the ragged corner cell; the ragged
# upper faces only; no flagged cell
BOXES = [((3, 5, 1), (30, 13, 11)), ((17, 2, 3), (9, 7, 5)), ((39, 23, 19), (1, 1, 1)), ((32, 0, 16), (8, 24, 4)), CLEAN_BOX]
TAIL_BOX = ((2, 1, 0), (18, 8, 3))
CHUNK_BOX = BOXES[0]


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
    """the decoded field perturbed like correction_pack_cases.fields: codes of a few -3 .. 3 among zeros where x < 16 (none at all
    from z = 16 on: clean cells), thousands where 16 <= x < 32, millions (a 16-bit type: hundreds) beyond; verbatim: +0.0, the code
    of value 0, in the slice z = 0 from x = 16 on"""
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
def expected(dtype, eps, dims):
    """-> (fixed-width blob of numpy's build against reference(), its packed form, the corrected array by error_bound_ref.apply)"""
    h, n = params_id(dims)
    dec = decoded(dtype, dims)
    blob = ebr.build(dec.copy(), reference(dtype, eps, dims).copy(), eps, RANGES[dtype], params_hash=h, n_params=n)["bytes"]
    corrected = ebr.apply(dec.copy(), blob)
    corrected.setflags(write=False)
    return blob, cpr.pack(blob), corrected


def packed_payload_bytes(packed):
    return cpr.split(packed, b"VNRCORP1")[0][15]


def fixed_payload_bytes(blob):
    return cpr.split(blob, b"VNRCORR1")[0][15]


@functools.lru_cache(maxsize=None)
def correction(dtype, eps, dims, form):
    """a correction read from packed bytes with `form` set before its first apply; shared, its form is left as it is"""
    c = api.Correction.from_packed_bytes(expected(dtype, eps, dims)[1])
    c.set_resident_form(form)
    return c


def device_apply(corr, dtype, kind, dims, box=None, verify=False):
    """one corrected decode of `box` (None: the whole grid, through vnrAmdNeuralVolumeDecodeToDeviceCorrected) into an array of
    sentinels -> (the whole destination after the call, the same as it was before, offset, strides)"""
    size = box[1] if box else dims
    n, offset, strides = layout(kind, size)
    before = np.full(n, sentinel(dtype), dtype)
    d = api.DeviceArray.from_numpy(before)
    try:
        api.vnrNeuralVolumeDecodeToDeviceCorrected(trained(dims)[1], corr, d.ptr + offset * before.dtype.itemsize, strides, verify_params=verify, box=box)
        return d.numpy(), before, offset, strides
    finally:
        d.free()


def check_box(corr, dtype, eps, kind, dims, box):
    """the decode of `box` equals the slice of expected, and no byte around it has changed"""
    got, expect, offset, strides = device_apply(corr, dtype, kind, dims, box)
    size = box[1] if box else dims
    box_view(expect, offset, strides, size)[...] = box_slice(expected(dtype, eps, dims)[2], box) if box else expected(dtype, eps, dims)[2]
    assert same_bytes(got, expect), (dtype, kind, box, corr.residency())
    return got


# ------------------------------------------------------------------------------------------------ 4. planes against fixed-width, whole grid
@pytest.mark.parametrize("kind", ["dense", "ghost"])
@pytest.mark.parametrize("dims", [DIMS, TAIL_DIMS], ids=["40x24x20", "21x10x3"])
@pytest.mark.parametrize("dtype,eps", APPLY_TYPES, ids=TYPE_IDS)
def test_apply_from_the_planes_equals_numpy_and_touches_nothing_else(dtype, eps, dims, kind):
    blob, packed, corrected = expected(dtype, eps, dims)
    corr = api.Correction.from_packed_bytes(packed)
    corr.set_resident_form("packed")                          # before the first apply: the fixed-width payload never reaches the device
    assert corr.residency() == {"form": "packed", "on_device": False, "device_bytes": 0, "payload_device_bytes": 0, "index_device_bytes": 0}
    check_box(corr, dtype, eps, kind, dims, None)
    assert not same_bytes(corrected, decoded(dtype, dims))
    r = corr.residency()
    n_groups = len(cir.index(packed)["group_word"])
    n_cells = int(np.prod([-(-d // 16) for d in dims]))
    assert r["form"] == "packed" and r["on_device"] and r["payload_device_bytes"] == packed_payload_bytes(packed)
    assert r["index_device_bytes"] == 4 * n_groups + 16 * n_cells and r["device_bytes"] == r["payload_device_bytes"] + r["index_device_bytes"]
    check_box(corr, dtype, eps, kind, dims, None)           # (resident now)
    assert corr.to_bytes() == blob and corr.to_packed_bytes() == packed
    corr.release()


def test_the_references_give_every_width_zero_groups_and_clean_cells():
    widths = set()
    for dtype, eps in APPLY_TYPES:
        blob, packed, _ = expected(dtype, eps, DIMS)
        f, cells, _ = cpr.split(blob, b"VNRCORR1")
        widths.update((f[10], w) for _, w in cells)
        assert list(cir.index(packed)["nbits"]).count(0) > 0, dtype
        assert [c for c, _ in cells] == [c for c in range(12) if c not in (6, 9)], (dtype, cells)      # CLEAN_BOX holds no flagged cell
        f, cells, _ = cpr.split(expected(dtype, eps, TAIL_DIMS)[0], b"VNRCORR1")
        assert [cpr.cell_voxels(TAIL_DIMS, c) for c, _ in cells] == [480, 150]                        # cx = 16 and cx = 5
    assert widths >= {(1, 1), (1, 2), (1, 4), (0, 1), (0, 2), (0, 4), (2, 8)}, widths


# ------------------------------------------------------------------------------------------------ 5. boxes
@pytest.mark.parametrize("box", BOXES, ids=["unaligned", "one-cell", "corner-voxel", "ragged-faces", "clean"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype,eps", APPLY_TYPES, ids=TYPE_IDS)
def test_box_equals_the_slice_of_the_whole_grid(dtype, eps, form, box):
    corr = correction(dtype, eps, DIMS, form)
    for kind in ("dense", "ghost", "gather"):
        got = check_box(corr, dtype, eps, kind, DIMS, box)
    assert corr.residency()["form"] == form
    if box == CLEAN_BOX:                                      # no flagged cell: the plain decode of the box
        n, offset, strides = layout("gather", box[1])
        d = api.DeviceArray.from_numpy(np.full(n, sentinel(dtype), dtype))
        api.vnrNeuralVolumeDecodeToDevice(trained(DIMS)[1], d.ptr + offset * np.dtype(dtype).itemsize, dtype, strides, box, None, RANGES[dtype])
        assert same_bytes(d.numpy(), got)
        d.free()
    else:
        assert not same_bytes(box_slice(expected(dtype, eps, DIMS)[2], box), box_slice(decoded(dtype, DIMS), box))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype,eps", APPLY_TYPES, ids=TYPE_IDS)
def test_box_of_the_volume_with_ragged_rows(dtype, eps, form):
    corr = correction(dtype, eps, TAIL_DIMS, form)
    for kind in ("dense", "ghost", "gather"):
        check_box(corr, dtype, eps, kind, TAIL_DIMS, TAIL_BOX)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype,eps", APPLY_TYPES, ids=TYPE_IDS)
def test_no_box_is_the_whole_grid_in_both_calls(dtype, eps, form):
    corr = correction(dtype, eps, DIMS, form)
    want = check_box(corr, dtype, eps, "ghost", DIMS, None)                 # vnrAmdNeuralVolumeDecodeToDeviceCorrected
    n, offset, strides = layout("ghost", DIMS)
    d = api.DeviceArray.from_numpy(np.full(n, sentinel(dtype), dtype))
    st = api.lib().vnrAmdNeuralVolumeDecodeBoxToDeviceCorrected(trained(DIMS)[1].h, corr.h, C.c_void_p(d.ptr + offset * np.dtype(dtype).itemsize),
                                                                (C.c_int64 * 3)(*strides), None, None, None, 1)
    assert st == 0, api._lib.last_error()
    assert same_bytes(d.numpy(), want)
    d.free()
    whole = ((0, 0, 0), DIMS)
    assert same_bytes(check_box(corr, dtype, eps, "ghost", DIMS, whole), want)


# ------------------------------------------------------------------------------------------------ 6. chunks
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype,eps", APPLY_TYPES, ids=TYPE_IDS)
def test_box_does_not_depend_on_the_chunk_size(dtype, eps, form, monkeypatch):
    corr = correction(dtype, eps, DIMS, form)
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    want = {kind: check_box(corr, dtype, eps, kind, DIMS, CHUNK_BOX) for kind in ("dense", "ghost")}
    assert int(np.prod(CHUNK_BOX[1])) == 4290
    for chunk in (1000, 4097):                                # chunk ends inside rows and inside groups
        monkeypatch.setenv("VNR_AMD_DECODE_CHUNK", str(chunk))
        for kind in ("dense", "ghost"):
            assert same_bytes(check_box(corr, dtype, eps, kind, DIMS, CHUNK_BOX), want[kind])


# ------------------------------------------------------------------------------------------------ 7. form changes
@pytest.mark.parametrize("dtype,eps", APPLY_TYPES, ids=TYPE_IDS)
def test_form_changes_of_a_built_correction_keep_results_and_bytes(dtype, eps):
    blob, packed, _ = expected(dtype, eps, DIMS)
    d = api.DeviceArray.from_numpy(np.ascontiguousarray(reference(dtype, eps, DIMS)).ravel())
    try:
        built = api.vnrNeuralVolumeBuildCorrection(trained(DIMS)[1], d, dtype, eps, None, RANGES[dtype])
    finally:
        d.free()
    fixed = {"form": "fixed", "on_device": True, "payload_device_bytes": fixed_payload_bytes(blob), "index_device_bytes": 0,
             "device_bytes": fixed_payload_bytes(blob) + 16 * 12}
    assert built.residency() == fixed                        # (the build leaves its codes resident)
    results = []
    for form in ("packed", "fixed", "packed"):
        built.set_resident_form(form)                        # converts at once: packed on the device / unpacked on the device
        r = built.residency()
        if form == "fixed":
            assert r == fixed
        else:
            assert r["form"] == "packed" and r["payload_device_bytes"] == packed_payload_bytes(packed) and r["index_device_bytes"] > 0
            assert r["device_bytes"] == r["payload_device_bytes"] + r["index_device_bytes"]
        results.append(check_box(built, dtype, eps, "ghost", DIMS, None))
        results.append(check_box(built, dtype, eps, "ghost", DIMS, BOXES[0]))
        assert built.residency() == r
        assert built.to_bytes() == blob and built.to_packed_bytes() == packed
    assert same_bytes(results[0], results[2]) and same_bytes(results[0], results[4])
    assert same_bytes(results[1], results[3]) and same_bytes(results[1], results[5])
    built.release()


def test_form_set_on_a_correction_from_fixed_width_bytes():
    dtype, eps = APPLY_TYPES[1]
    blob, packed, _ = expected(dtype, eps, DIMS)
    c = api.Correction.from_bytes(blob)
    c.set_resident_form("packed")                             # nothing resident yet: the first apply packs on the device
    assert not c.residency()["on_device"]
    check_box(c, dtype, eps, "dense", DIMS, BOXES[0])
    r = c.residency()
    assert r["payload_device_bytes"] == packed_payload_bytes(packed) and r["device_bytes"] == r["payload_device_bytes"] + r["index_device_bytes"]
    assert c.to_packed_bytes() == packed and c.to_bytes() == blob
    c.release()


# ------------------------------------------------------------------------------------------------ 8. residency
def test_packed_residency_stays_under_its_cap_and_below_the_fixed_width_payload():
    out = cases.many_cells()
    packed = cpr.pack(out["bytes"])
    payload, fixed_bytes = packed_payload_bytes(packed), fixed_payload_bytes(out["bytes"])
    n_groups, n_cells = len(cir.index(packed)["group_word"]), 8 * 8 * 5
    cap = payload + 4 * n_groups + 32 * n_cells
    print("packed payload", payload, "groups", n_groups, "cells", n_cells, "cap", cap, "fixed-width payload", fixed_bytes)
    # the precondition, from the reference's bytes: the cap is 946 008 bytes, 0.72 (0.7203) of the fixed-width payload
    assert (payload, n_groups, fixed_bytes) == (876616, 14788, 1313280) and cap == 946008 and round(cap / fixed_bytes, 2) == 0.72
    dims = (128, 120, 70)
    cfg = syn.model_config(n_levels=4, n_features=2, log2_hashmap_size=12, base_resolution=4, n_neurons=16, n_hidden_layers=1)
    nv = api.vnrCreateNeuralVolume(cfg, dims)                 # the parameters need not match: verify_params = 0, the voxels are not read
    d = api.DeviceArray((dims[0] * dims[1] * dims[2],), np.int16)
    corr = api.Correction.from_packed_bytes(packed)
    corr.set_resident_form("packed")
    assert corr.residency() == {"form": "packed", "on_device": False, "device_bytes": 0, "payload_device_bytes": 0, "index_device_bytes": 0}
    api.vnrNeuralVolumeDecodeToDeviceCorrected(nv, corr, d)
    r = corr.residency()
    print(r)
    assert r["on_device"] and r["form"] == "packed" and 0 < r["device_bytes"] <= cap
    assert r["payload_device_bytes"] == payload and r["index_device_bytes"] <= 4 * n_groups + 32 * n_cells
    other = api.Correction.from_packed_bytes(packed)          # the default form
    assert other.residency() == {"form": "fixed", "on_device": False, "device_bytes": 0, "payload_device_bytes": 0, "index_device_bytes": 0}
    api.vnrNeuralVolumeDecodeToDeviceCorrected(nv, other, d)
    f = other.residency()
    print(f)
    assert f["on_device"] and f["form"] == "fixed" and f["device_bytes"] >= fixed_bytes and f["payload_device_bytes"] == fixed_bytes and f["index_device_bytes"] == 0
    d.free(); corr.release(); other.release(); nv.release()


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_give_a_message_and_write_nothing():
    L = api.lib()
    dtype, eps = APPLY_TYPES[0]
    nv = trained(DIMS)[1]
    corr = api.Correction.from_packed_bytes(expected(dtype, eps, DIMS)[1])
    before = np.full(DIMS[0] * DIMS[1] * DIMS[2], sentinel(dtype), dtype)
    d = api.DeviceArray.from_numpy(before)
    i3, s3 = (lambda *v: (C.c_int * 3)(*v)), (lambda *v: (C.c_int64 * 3)(*v))

    def refused(word, strides, lo, size, volume=nv.h, handle=corr.h):
        st = L.vnrAmdNeuralVolumeDecodeBoxToDeviceCorrected(volume, handle, C.c_void_p(d.ptr), strides, lo, size, None, 0)
        msg = api._lib.last_error()
        assert st != 0 and word in msg, (word, msg)
        assert same_bytes(d.numpy(), before)

    for form in FORMS:
        corr.set_resident_form(form)
        refused("outside the grid", None, i3(30, 0, 0), i3(11, 4, 4))
        refused("outside the grid", None, i3(0, -1, 0), i3(4, 4, 4))
        refused("outside the grid", None, i3(0, 0, 20), i3(1, 1, 1))
        refused("both or neither", None, i3(0, 0, 0), None)
        refused("both or neither", None, None, i3(4, 4, 4))
        refused("box sizes must be positive", None, i3(0, 0, 0), i3(4, 0, 4))
        refused("box sizes must be positive", None, i3(0, 0, 0), i3(4, 4, -2))
        refused("overlap", s3(1, 7, 80), i3(0, 0, 0), i3(8, 8, 8))
        refused("strides must be positive", s3(1, 0, 80), i3(0, 0, 0), i3(8, 8, 8))
        refused("null correction", None, i3(0, 0, 0), i3(4, 4, 4), handle=None)
        refused("null volume", None, i3(0, 0, 0), i3(4, 4, 4), volume=None)
        st = L.vnrAmdNeuralVolumeDecodeBoxToDeviceCorrected(nv.h, corr.h, None, None, i3(0, 0, 0), i3(4, 4, 4), None, 0)
        assert st != 0 and "null device data" in api._lib.last_error()
        assert not corr.residency()["on_device"]              # a refused call uploads nothing
    # the form itself
    for bad in (2, -1, 7):
        assert L.vnrAmdCorrectionSetResidentForm(corr.h, bad) != 0 and "unknown resident form" in api._lib.last_error()
        assert corr.residency()["form"] == "packed"
    assert L.vnrAmdCorrectionSetResidentForm(None, 1) != 0 and "null correction" in api._lib.last_error()
    r = api._lib.CorrectionResidency()
    assert L.vnrAmdCorrectionGetResidency(None, C.byref(r)) != 0 and "null correction" in api._lib.last_error()
    assert L.vnrAmdCorrectionGetResidency(corr.h, None) != 0 and "null result" in api._lib.last_error()
    with pytest.raises(api.VnrAmdError, match="resident form must be"):
        corr.set_resident_form("planes")
    with pytest.raises(api.VnrAmdError, match="box must be"):
        api.vnrNeuralVolumeDecodeToDeviceCorrected(nv, corr, d, box=((0, 0, 0), (4, 0, 4)))
    assert same_bytes(d.numpy(), before)
    d.free(); corr.release()
