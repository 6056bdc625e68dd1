"""Packed corrections on the device (include/vnr_amd.h, "packed corrections"; csrc/correction_pack.hip): the device pack behind
vnrAmdCorrectionSerializePacked and the device unpack behind the first apply of a correction read from packed bytes, against the
numpy restatement tests/correction_pack_ref.py.  Bits are moved, nothing is computed: every comparison has tolerance ZERO.

The pack needs no network: fixed-width blobs built by numpy (tests/correction_pack_cases.py: every kind and code width, groups of
zeros, cells of 480, 256, 150, 30 and 16 voxels, blobs crafted for nbits 0, 1, 8 * width and 64, one blob of about 300 flagged cells)
are loaded with from_bytes and packed.  The unpack is checked through the apply, on the (40, 24, 20) volume of
tests/test_gpu_error_bounded.py (model, training and layouts restated) and on a (21, 10, 3) one whose cells have 480 and 150 voxels:
references are the decoded field perturbed so that codes of 1, 2 and 4 bytes and groups of zeros occur."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correction_pack_cases as cases  # noqa: E402
import correction_pack_ref as cpr  # noqa: E402
import error_bound_ref as ebr  # noqa: E402

pytestmark = pytest.mark.gpu

DIMS = (40, 24, 20)
TAIL_DIMS = (21, 10, 3)
# (dtype, eps): kind 1, kind 0 of a narrow and of a wide type, kind 2 with 64-bit patterns
APPLY_TYPES = [(np.float32, 1e-3), (np.int16, 2), (np.uint32, 1), (np.float64, 0)]
RANGES = {np.int16: (-30000.0, 30000.0), np.uint32: (0.0, 4.0e9), np.float32: (-3.5, 12.25), np.float64: (-1.0e3, 2.5e3)}


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
    """-> (fixed-width blob of numpy's build against reference(), its packed form, the corrected array by error_bound_ref.apply)"""
    h, n = params_id(dims)
    dec = decoded(dtype, dims)
    blob = ebr.build(dec.copy(), reference(dtype, eps, dims).copy(), eps, RANGES[dtype], params_hash=h, n_params=n)["bytes"]
    corrected = ebr.apply(dec.copy(), blob)
    corrected.setflags(write=False)
    return blob, cpr.pack(blob), corrected


def device_apply(corr, dtype, kind, dims, verify=False):
    """-> (the whole destination after the call, the same as it was before, offset, strides)"""
    n, offset, strides = layout(kind, dims)
    before = np.full(n, sentinel(dtype), dtype)
    d = api.DeviceArray.from_numpy(before)
    try:
        api.vnrNeuralVolumeDecodeToDeviceCorrected(trained(dims)[1], corr, d.ptr + offset * before.dtype.itemsize, strides, verify_params=verify)
        return d.numpy(), before, offset, strides
    finally:
        d.free()


def nbits_of(packed):
    f, cells, payload = cpr.split(packed, b"VNRCORP1")
    return list(payload[:sum(-(-cpr.cell_voxels(f[3:6], c) // 64) for c, _ in cells)])


# ------------------------------------------------------------------------------------------------ the device pack, no network
def pack_blobs():
    out = [(i, lambda c=c: cases.case(*c)["bytes"]) for i, c in zip(cases.IDS, cases.CASES)]
    out += [(f"crafted-{t.__name__}-{e}-w{w}", lambda k=(t, e, w): cases.crafted(*k)[0]) for t, e, w in cases.CRAFTED]
    return out + [("many-cells", lambda: cases.many_cells()["bytes"])]


@pytest.mark.parametrize("name,make", pack_blobs(), ids=[b[0] for b in pack_blobs()])
def test_device_pack_equals_numpy_byte_for_byte(name, make):
    v1 = make()
    want = cpr.pack(v1)
    c = api.Correction.from_bytes(v1)
    got = c.to_packed_bytes()
    print(name, "fixed-width", len(v1), "packed", len(got), "numpy", len(want))
    assert got == want
    assert c.to_packed_bytes() == want and c.to_bytes() == v1       # (cached; the correction itself is as it was)
    c.release()


def test_many_cells_cross_the_blocks_of_the_offset_scan():
    out = cases.many_cells()
    assert 250 <= out["n_flagged"] <= 320 and {w for _, w in out["cells"]} == {1, 2}
    nbits = nbits_of(cpr.pack(out["bytes"]))
    assert len(nbits) > 12000 and nbits.count(0) > 100 and sum(nbits) > 2 ** 16


# ------------------------------------------------------------------------------------------------ the device unpack, through the apply
@pytest.mark.parametrize("kind", ["dense", "ghost"])
@pytest.mark.parametrize("dims", [DIMS, TAIL_DIMS], ids=["40x24x20", "21x10x3"])
@pytest.mark.parametrize("dtype,eps", APPLY_TYPES, ids=[f"{t.__name__}-{e}" for t, e in APPLY_TYPES])
def test_apply_from_packed_bytes_equals_numpy_and_touches_nothing_else(dtype, eps, dims, kind):
    blob, packed, corrected = expected(dtype, eps, dims)
    corr = api.Correction.from_packed_bytes(packed)
    got, expect, offset, strides = device_apply(corr, dtype, kind, dims)      # upload, unpack on the device, apply
    box_view(expect, offset, strides, dims)[...] = corrected
    assert same_bytes(got, expect)
    assert not same_bytes(corrected, decoded(dtype, dims))
    again, _, _, _ = device_apply(corr, dtype, kind, dims)                    # (resident now)
    assert same_bytes(again, expect)
    assert corr.to_bytes() == blob and corr.to_packed_bytes() == packed
    corr.release()


def test_the_references_give_every_width_zero_groups_and_partly_filled_groups():
    widths, zero_groups = set(), 0
    for dtype, eps in APPLY_TYPES:
        blob, packed, _ = expected(dtype, eps, DIMS)
        widths.update((cpr.split(blob, b"VNRCORR1")[0][10], w) for _, w in cpr.split(blob, b"VNRCORR1")[1])
        assert nbits_of(packed).count(0) > 0, dtype
        zero_groups += nbits_of(packed).count(0)
    assert widths >= {(1, 1), (1, 2), (1, 4), (0, 1), (0, 2), (0, 4), (2, 8)}, widths
    print("groups of zeros:", zero_groups)
    for dtype, eps in APPLY_TYPES:
        f, cells, _ = cpr.split(expected(dtype, eps, TAIL_DIMS)[0], b"VNRCORR1")
        assert [cpr.cell_voxels(TAIL_DIMS, c) for c, _ in cells] == [480, 150]      # 7.5 and 2.34 groups


# ------------------------------------------------------------------------------------------------ a correction the device built
@pytest.mark.parametrize("dtype,eps", APPLY_TYPES, ids=[f"{t.__name__}-{e}" for t, e in APPLY_TYPES])
def test_built_correction_packs_to_what_numpy_packs_and_reads_back(dtype, eps):
    blob, packed, corrected = expected(dtype, eps, DIMS)
    d = api.DeviceArray.from_numpy(np.ascontiguousarray(reference(dtype, eps, DIMS)).ravel())
    try:
        built = api.vnrNeuralVolumeBuildCorrection(trained(DIMS)[1], d, dtype, eps, None, RANGES[dtype])
    finally:
        d.free()
    assert built.to_bytes() == blob
    assert built.to_packed_bytes() == cpr.pack(built.to_bytes()) == packed
    first, expect, offset, strides = device_apply(built, dtype, "ghost", DIMS, verify=True)
    back = api.Correction.from_packed_bytes(built.to_packed_bytes())
    second, _, _, _ = device_apply(back, dtype, "ghost", DIMS, verify=True)
    box_view(expect, offset, strides, DIMS)[...] = corrected
    assert same_bytes(first, expect) and same_bytes(second, expect)
    built.release(); back.release()


# ------------------------------------------------------------------------------------------------ refusals
def test_null_arguments_and_other_dims_are_refused():
    L = api.lib()
    out, n = C.c_void_p(), C.c_size_t()
    assert L.vnrAmdCorrectionSerializePacked(None, C.byref(out), C.byref(n)) != 0 and "null correction" in api._lib.last_error()
    h = L.vnrAmdCreateCorrectionFromPackedBytes(None, 200)
    assert not h and "null bytes" in api._lib.last_error()
    c = api.Correction.from_bytes(cases.case(np.float32, 1e-3, (17, 16, 33))["bytes"])
    assert L.vnrAmdCorrectionSerializePacked(c.h, None, C.byref(n)) != 0 and "null result" in api._lib.last_error()
    assert L.vnrAmdCorrectionSerializePacked(c.h, C.byref(out), None) != 0 and "null result" in api._lib.last_error()
    other = api.Correction.from_packed_bytes(c.to_packed_bytes())         # (17, 16, 33) against the volume's (40, 24, 20)
    before = np.full(DIMS[0] * DIMS[1] * DIMS[2], sentinel(np.float32), np.float32)
    d = api.DeviceArray.from_numpy(before)
    st = L.vnrAmdNeuralVolumeDecodeToDeviceCorrected(trained(DIMS)[1].h, other.h, C.c_void_p(d.ptr), None, None, 0)
    assert st != 0 and "differ from the volume's" in api._lib.last_error()
    assert same_bytes(d.numpy(), before)
    with pytest.raises(api.VnrAmdError, match="malformed packed correction bytes"):
        api.Correction.from_packed_bytes(c.to_packed_bytes()[:-3])
    d.free(); c.release(); other.release()
