"""Coded corrections on the device (include/vnr_amd.h, "coded corrections"; csrc/correction_code.hip): the device encode behind
vnrAmdCorrectionSerializeCoded and vnrAmdCorrectionSerializeCodedToDevice, from the resident fixed-width codes and from the resident
bit planes, and the device decode behind the first apply of a correction read from coded bytes, against the numpy restatement
tests/correction_coded_ref.py.  Bits are moved, nothing is computed: every comparison has tolerance ZERO.

The encode needs no network: the blobs of tests/correction_coded_cases.py are loaded with from_bytes (the device pack then leaves the
fixed-width codes resident) or with from_packed_bytes (in the packed resident form, whose planes SerializePackedToDevice makes
resident).  The decode is checked through the apply: on the (40, 24, 20) and (21, 10, 3) volumes of tests/test_gpu_correction_pack.py
(model, training, references and layouts restated), and, for the longest streams, many cells and the crafted blobs, on barely trained
networks of the blobs' own dims, against the same correction read from its fixed-width bytes."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correction_coded_cases as ccc  # noqa: E402
import correction_coded_ref as ccr  # noqa: E402
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
BLOBS = ccc.all_blobs()
NAMES = [b[0] for b in BLOBS]


@functools.lru_cache(maxsize=None)
def coded_of(name):
    return ccr.encode(dict(BLOBS)[name])


def ground_truth(dims):
    z0, y0 = (40 - dims[2]) // 2, (40 - dims[1]) // 2
    a = syn.analytic_volume(40)[z0:z0 + dims[2], y0:y0 + dims[1], :dims[0]]
    a = (a - a.min()) / (a.max() - a.min())
    return np.clip(np.float32(1.6) * a - np.float32(0.3), 0, 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def trained(dims):
    """-> (simple volume, neural volume) with fixed seeds, 400 steps (10 for every other one); shared and left unchanged.  (40, 24, 20)
    and (21, 10, 3) are the volumes of test_gpu_correction_pack.py; any other dims get seeded noise as ground truth"""
    before = {k: os.environ.get(k) for k in ("VNR_AMD_INIT_SEED", "VNR_AMD_DECODE_CHUNK")}
    os.environ["VNR_AMD_INIT_SEED"] = "4711"
    os.environ.pop("VNR_AMD_DECODE_CHUNK", None)
    try:
        truth = ground_truth(dims) if dims in (DIMS, TAIL_DIMS) else np.random.default_rng(3).uniform(0, 1, dims[::-1]).astype(np.float32)
        sv = api.vnrCreateSimpleVolume(truth, value_range=(0.0, 1.0))
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
    sy, sz = bx + 5, (bx + 5) * (by + 3)
    return sz * (bz + 2), 2 + sy + sz, (1, sy, sz)


def box_view(flat, offset, strides, size):
    bx, by, bz = size
    sx, sy, sz = strides or (1, bx, bx * by)
    it = flat.dtype.itemsize
    return np.lib.stride_tricks.as_strided(flat[offset:], shape=(bz, by, bx), strides=(sz * it, sy * it, sx * it))


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


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
    """the decoded field perturbed like correction_pack_cases.fields: codes of a few -3 .. 3 among zeros where x < 16, thousands where
    16 <= x < 32, millions (a 16-bit type: hundreds) beyond; verbatim: +0.0, the code of value 0, in the slice z = 0 from x = 16 on"""
    dec = decoded(dtype, dims)
    rng = np.random.default_rng(dims[0] + np.dtype(dtype).itemsize)
    wide = np.dtype(dtype).itemsize > 2
    x = np.arange(dims[0])
    scale = np.where(x < 16, 1.0, np.where(x < 32, 6000.0 if wide else 1000.0, 3.0e6 if wide else 300.0))
    q = np.rint(rng.normal(0.0, 1.0, dec.shape) * scale).astype(np.int64)
    q[:, :, :16] *= rng.uniform(size=dec.shape)[:, :, :16] < 0.03
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
    """-> (fixed-width blob of numpy's build against reference(), its packed form, its coded form, the corrected array by error_bound_ref.apply)"""
    h, n = params_id(dims)
    dec = decoded(dtype, dims)
    blob = ebr.build(dec.copy(), reference(dtype, eps, dims).copy(), eps, RANGES[dtype], params_hash=h, n_params=n)["bytes"]
    corrected = ebr.apply(dec.copy(), blob)
    corrected.setflags(write=False)
    return blob, cpr.pack(blob), ccr.encode(blob), corrected


def device_apply(corr, dtype, kind, dims, box=None):
    """-> (the whole destination after the call, the same as it was before, offset, strides); box = (lower, size): that box alone"""
    size = dims if box is None else box[1]
    n, offset, strides = layout(kind, size)
    before = np.full(n, sentinel(dtype), dtype)
    d = api.DeviceArray.from_numpy(before)
    try:
        api.vnrNeuralVolumeDecodeToDeviceCorrected(trained(dims)[1], corr, d.ptr + offset * before.dtype.itemsize, strides, box=box)
        return d.numpy(), before, offset, strides
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------ the device encode, no network
def encode_on_device(c, want):
    """SerializeCodedToDevice first (it encodes straight into the destination and caches nothing), then SerializeCoded"""
    assert c.residency()["on_device"]
    size = c.to_coded_device()
    assert size == len(want)
    fill = np.full(size + 24, 0xa5, np.uint8)
    d = api.DeviceArray.from_numpy(fill)
    try:
        with pytest.raises(api.VnrAmdError, match=f"capacity \\({size - 1} bytes\\) is smaller than the coded correction \\({size} bytes\\)"):
            c.to_coded_device((d.ptr, size - 1))
        assert np.array_equal(d.numpy(), fill)                       # refused: nothing written
        assert c.to_coded_device((d.ptr, size + 24)) == size
        got = d.numpy()
        assert got[:size].tobytes() == want and np.array_equal(got[size:], fill[size:])
    finally:
        d.free()
    assert c.to_coded_bytes() == want
    assert c.to_coded_bytes() == want and c.to_coded_device() == size      # (cached)


@pytest.mark.parametrize("name,v1", BLOBS, ids=NAMES)
def test_device_encode_from_resident_codes_equals_numpy_byte_for_byte(name, v1):
    c = api.Correction.from_bytes(v1)
    assert c.to_packed_bytes() == cpr.pack(v1)                       # the device pack: the fixed-width codes are resident from here on
    assert c.residency()["form"] == "fixed"
    encode_on_device(c, coded_of(name))
    assert c.to_bytes() == v1                                        # (the correction itself is as it was)
    c.release()


@pytest.mark.parametrize("name,v1", BLOBS, ids=NAMES)
def test_device_encode_from_resident_planes_equals_numpy_byte_for_byte(name, v1):
    packed = cpr.pack(v1)
    c = api.Correction.from_packed_bytes(packed)
    c.set_resident_form("packed")
    d = api.DeviceArray((len(packed),), np.uint8)
    try:
        assert c.to_packed_device(d) == len(packed)                  # in the packed resident form this makes the planes resident
    finally:
        d.free()
    r = c.residency()
    assert r["form"] == "packed" and r["on_device"] and r["index_device_bytes"] > 0
    encode_on_device(c, coded_of(name))
    assert c.residency() == r and c.to_packed_bytes() == packed
    c.release()


def test_the_blobs_hold_the_longest_streams_and_many_cells():
    for verbatim, name in ((False, "longest-w4"), (True, "longest-f64")):
        f, cells, payload = ccr.split(coded_of(name))
        assert np.frombuffer(payload, "<u4", 1)[0] == ccc.LONGEST_WORDS[verbatim]
    assert ccc.LONGEST_WORDS[True] == 7 + 64 * 65                    # kCodedMaxCellWords: what the kernels stage in LDS
    f, cells, payload = ccr.split(coded_of("many-cells"))
    assert 250 <= len(cells) <= 320                                  # more than one block of the scan


# ------------------------------------------------------------------------------------------------ after the direct build
@pytest.mark.parametrize("dims", [DIMS, TAIL_DIMS], ids=["40x24x20", "21x10x3"])
@pytest.mark.parametrize("dtype,eps", APPLY_TYPES, ids=TYPE_IDS)
def test_direct_build_codes_to_what_numpy_codes_from_the_two_call_build(dtype, eps, dims):
    d = api.DeviceArray.from_numpy(np.ascontiguousarray(reference(dtype, eps, dims)).ravel())
    try:
        direct = api.vnrNeuralVolumeBuildCorrectionPacked(trained(dims)[1], d, dtype, eps, None, RANGES[dtype])
        built = api.vnrNeuralVolumeBuildCorrection(trained(dims)[1], d, dtype, eps, None, RANGES[dtype])
    finally:
        d.free()
    want = ccr.encode(built.to_bytes())
    assert direct.residency()["form"] == "packed"
    encode_on_device(direct, want)                                   # from the planes the build left resident
    assert built.residency()["form"] == "fixed"
    encode_on_device(built, want)                                    # from the codes the two-call build left resident
    assert want == expected(dtype, eps, dims)[2]
    direct.release(); built.release()


# ------------------------------------------------------------------------------------------------ the device decode, through the apply
@pytest.mark.parametrize("resident", ["fixed", "packed"])
@pytest.mark.parametrize("kind", ["dense", "ghost"])
@pytest.mark.parametrize("dims", [DIMS, TAIL_DIMS], ids=["40x24x20", "21x10x3"])
@pytest.mark.parametrize("dtype,eps", APPLY_TYPES, ids=TYPE_IDS)
def test_apply_from_coded_bytes_equals_the_fixed_width_form_and_touches_nothing_else(dtype, eps, dims, kind, resident):
    blob, packed, coded, corrected = expected(dtype, eps, dims)
    fixed, twin, corr = api.Correction.from_bytes(blob), api.Correction.from_packed_bytes(packed), api.Correction.from_coded_bytes(coded)
    for c in (fixed, twin, corr):
        c.set_resident_form(resident)
    box = ((3, 1, 1), (dims[0] - 4, dims[1] - 3, dims[2] - 1))      # aligned to nothing
    results = {}
    for name, c in (("coded", corr), ("fixed", fixed), ("packed", twin)):   # upload, decode on the device, (unpack,) apply
        whole, expect, offset, strides = device_apply(c, dtype, kind, dims)
        part, expect_box, box_offset, box_strides = device_apply(c, dtype, kind, dims, box)
        results[name] = (whole, part)
    box_view(expect, offset, strides, dims)[...] = corrected
    cut = tuple(slice(lo, lo + n) for lo, n in zip(box[0][::-1], box[1][::-1]))
    box_view(expect_box, box_offset, box_strides, box[1])[...] = corrected[cut]
    for name, (whole, part) in results.items():
        assert same_bytes(whole, expect) and same_bytes(part, expect_box), name     # the ghost layers keep their sentinel
    assert not same_bytes(corrected, decoded(dtype, dims))
    assert corr.residency() == twin.residency() and corr.residency()["on_device"] and corr.residency()["form"] == resident
    assert corr.to_packed_bytes() == packed == twin.to_packed_bytes() and corr.to_bytes() == blob == twin.to_bytes()
    assert corr.to_coded_bytes() == coded and twin.to_coded_bytes() == coded
    assert corr.residency() == twin.residency()
    for c in (fixed, twin, corr):
        c.release()


NETWORK_FREE = ["longest-w4", "longest-f64", "many-cells", "plane-counts", "pattern64", "int32-1-17x16x33", "gaussian"]


@pytest.mark.parametrize("resident", ["fixed", "packed"])
@pytest.mark.parametrize("name", NETWORK_FREE)
def test_device_decode_of_the_longest_streams_many_cells_and_crafted_blobs(name, resident):
    """a barely trained network of the blob's dims: the apply of the correction read from coded bytes stores what the apply of the
    one read from fixed-width bytes stores, and the planes the device decoded (downloaded by to_packed_bytes in the packed resident
    form) are numpy's"""
    v1 = dict(BLOBS)[name]
    f = cpr.split(v1, b"VNRCORR1")[0]
    dims, dtype = tuple(f[3:6]), ebr.DTYPES[f[2]].type
    corr, fixed = api.Correction.from_coded_bytes(coded_of(name)), api.Correction.from_bytes(v1)
    corr.set_resident_form(resident); fixed.set_resident_form(resident)
    n = dims[0] * dims[1] * dims[2]
    outs = []
    for c in (corr, fixed):
        d = api.DeviceArray.from_numpy(np.full(n, sentinel(dtype), dtype))
        try:
            api.vnrNeuralVolumeDecodeToDeviceCorrected(trained(dims)[1], c, d)
            outs.append(d.numpy())
        finally:
            d.free()
    assert same_bytes(outs[0], outs[1])
    plain = api.DeviceArray((n,), dtype)
    api.vnrNeuralVolumeDecodeToDevice(trained(dims)[1], plain, dtype, value_range=(f[8], f[9]))
    assert not same_bytes(outs[0], plain.numpy())                    # (the correction did something)
    plain.free()
    assert corr.residency() == fixed.residency() and corr.residency()["on_device"]
    assert corr.to_packed_bytes() == cpr.pack(v1) and corr.to_bytes() == v1 and corr.to_coded_bytes() == coded_of(name)
    corr.release(); fixed.release()


# ------------------------------------------------------------------------------------------------ refusals
def test_null_arguments_and_other_dims_are_refused():
    L = api.lib()
    n = C.c_size_t()
    assert L.vnrAmdCorrectionSerializeCodedToDevice(None, None, 0, C.byref(n), None) != 0 and "null correction" in api._lib.last_error()
    c = api.Correction.from_coded_bytes(coded_of("float32-0.001-17x16x33"))
    assert L.vnrAmdCorrectionSerializeCodedToDevice(c.h, None, 0, None, None) != 0 and "null result" in api._lib.last_error()
    before = np.full(DIMS[0] * DIMS[1] * DIMS[2], sentinel(np.float32), np.float32)     # (17, 16, 33) against the volume's (40, 24, 20)
    d = api.DeviceArray.from_numpy(before)
    st = L.vnrAmdNeuralVolumeDecodeToDeviceCorrected(trained(DIMS)[1].h, c.h, C.c_void_p(d.ptr), None, None, 0)
    assert st != 0 and "differ from the volume's" in api._lib.last_error()
    assert same_bytes(d.numpy(), before) and not c.residency()["on_device"]
    with pytest.raises(api.VnrAmdError, match="malformed coded correction bytes"):
        api.Correction.from_coded_bytes(coded_of("float32-0.001-17x16x33")[:-3])
    d.free(); c.release()
