"""Error-bounded round trip on the device (include/vnr_amd.h, "error-bounded round trip"; csrc/correction.hip):
vnrAmdNeuralVolumeBuildCorrection and vnrAmdNeuralVolumeDecodeToDeviceCorrected against the numpy restatement tests/error_bound_ref.py.

The arithmetic is integer or single IEEE double operations, so every comparison has tolerance ZERO: the serialised bytes, the
corrected array and every number of the report equal numpy's.  numpy's `dec` is what vnrAmdNeuralVolumeDecodeToDevice stores, `ref`
the ground truth converted to the type (perturbed where a case says so).  The tolerance of a case comes from the data: strictly
between two adjacent distinct entries of the error report's block map (some cells flagged, some not), or a fraction of the largest
error (code widths).

Volume, model, training, chunk setting and array layouts are those of tests/test_gpu_device_decode.py, restated: (40, 24, 20) has 12
ragged macrocells; VNR_AMD_DECODE_CHUNK = 7001 gives 3 chunks, none ending at the end of a row."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import error_bound_ref as ebr  # noqa: E402

pytestmark = pytest.mark.gpu

DIMS = (40, 24, 20)
N = DIMS[0] * DIMS[1] * DIMS[2]
N_CELLS = 12
CHUNK = "7001"
TYPES = [np.uint8, np.int16, np.uint32, np.float32, np.float64]
RANGES = {np.uint8: (0.0, 255.0), np.int16: (-30000.0, 30000.0), np.uint32: (0.0, 4.0e9), np.float32: (-3.5, 12.25), np.float64: (-1.0e3, 2.5e3)}
LAYOUTS = ["dense", "ghost", "sx2"]


def ground_truth():
    z0, y0 = (40 - DIMS[2]) // 2, (40 - DIMS[1]) // 2
    a = syn.analytic_volume(40)[z0:z0 + DIMS[2], y0:y0 + DIMS[1], :DIMS[0]]
    a = (a - a.min()) / (a.max() - a.min())
    return np.clip(np.float32(1.6) * a - np.float32(0.3), 0, 1).astype(np.float32)


def train(steps):
    before = {k: os.environ.get(k) for k in ("VNR_AMD_INIT_SEED", "VNR_AMD_DECODE_CHUNK")}
    os.environ["VNR_AMD_INIT_SEED"] = "4711"
    os.environ.pop("VNR_AMD_DECODE_CHUNK", None)
    try:
        sv = api.vnrCreateSimpleVolume(ground_truth(), value_range=(0.0, 1.0))
        cfg = syn.model_config(n_levels=4, n_features=2, log2_hashmap_size=12, base_resolution=4, n_neurons=16, n_hidden_layers=1)
        nv = api.vnrCreateNeuralVolume(cfg, sv)
        api.check(api.lib().vnrAmdNeuralVolumeSetSamplerSeed(nv.h, 99, 7))
        api.vnrNeuralVolumeTrain(nv, steps, True)
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return sv, nv


@functools.lru_cache(maxsize=None)
def trained():
    """-> (simple volume, neural volume): trained 400 steps with fixed seeds; shared and left unchanged"""
    return train(400)


def convert(v, dtype, value_range):
    """the header's conversion, step by step"""
    d = np.asarray(v, np.float32)
    lo, hi = np.float32(value_range[0]), np.float32(value_range[1])
    d = (d * np.float32(hi - lo)).astype(np.float32) + lo
    if np.issubdtype(dtype, np.floating):
        return d.astype(dtype)
    r = np.rint(d.astype(np.float64))
    info = np.iinfo(dtype)
    return np.clip(r, float(info.min), float(info.max)).astype(dtype)


def sentinel(dtype):
    return np.frombuffer(b"\xa5" * np.dtype(dtype).itemsize, dtype)[0]


def layout(kind, size=DIMS):
    """-> (elements of the array, element offset of the first voxel, strides or None)"""
    bx, by, bz = size
    if kind == "dense":
        return bx * by * bz, 0, None
    if kind == "ghost":
        sy, sz = bx + 5, (bx + 5) * (by + 3)
        return sz * (bz + 2), 2 + sy + sz, (1, sy, sz)
    sy, sz = 2 * bx + 3, (2 * bx + 3) * (by + 1)
    return sz * (bz + 1), 1, (2, sy, sz)


def box_view(flat, offset, strides, size=DIMS):
    bx, by, bz = size
    sx, sy, sz = strides or (1, bx, bx * by)
    it = flat.dtype.itemsize
    return np.lib.stride_tricks.as_strided(flat[offset:], shape=(bz, by, bx), strides=(sz * it, sy * it, sx * it))


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@functools.lru_cache(maxsize=None)
def decoded(dtype):
    """what vnrAmdNeuralVolumeDecodeToDevice stores, [z, y, x]; computed once, read only"""
    d = api.DeviceArray((N,), dtype)
    api.vnrNeuralVolumeDecodeToDevice(trained()[1], d, dtype, value_range=RANGES[dtype])
    out = d.numpy().reshape(DIMS[::-1])
    d.free()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def field(dtype):
    out = convert(ground_truth(), dtype, RANGES[dtype])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def params_id():
    p = api.neural_get_params_fp16(trained()[1])
    return ebr.fnv1a64(np.ascontiguousarray(p).tobytes()), int(p.size)


@functools.lru_cache(maxsize=None)
def block_map(dtype):
    d = api.DeviceArray.from_numpy(field(dtype).ravel())
    out = api.vnrNeuralVolumeErrorAgainstDevice(trained()[1], d, dtype, value_range=RANGES[dtype], block_map=True)
    d.free()
    return out


@functools.lru_cache(maxsize=None)
def mixed_eps(dtype):
    """strictly between two adjacent distinct entries of the error report's block map, the middle pair"""
    v = np.unique(block_map(dtype)["block_max"].astype(np.float64))
    print(np.dtype(dtype).name, "block maxima", v)
    if len(v) < 2:
        pytest.fail(f"the block map of {np.dtype(dtype).name} has no two distinct entries: {v}")
    k = (len(v) - 1) // 2
    return float((v[k] + v[k + 1]) / 2)


@functools.lru_cache(maxsize=None)
def expected(dtype, eps, plant=None):
    """numpy's build for ref = the field (plant: ((z, y, x), value) pairs written into it first) -> (ref, dict of error_bound_ref.build)"""
    ref = field(dtype).copy()
    for at, value in plant or ():
        ref[at] = value
    h, n = params_id()
    return ref, ebr.build(decoded(dtype).copy(), ref, eps, RANGES[dtype], params_hash=h, n_params=n)


def device_build(ref, dtype, kind, eps):
    n, offset, strides = layout(kind)
    flat = np.full(n, sentinel(dtype), dtype)
    box_view(flat, offset, strides)[...] = ref
    d = api.DeviceArray.from_numpy(flat)
    try:
        return api.vnrNeuralVolumeBuildCorrection(trained()[1], d.ptr + offset * flat.dtype.itemsize, dtype, eps, strides, RANGES[dtype])
    finally:
        d.free()


def device_apply(corr, dtype, kind, volume=None, verify=False):
    """-> (the whole destination after the call, the same as it was before, offset, strides)"""
    n, offset, strides = layout(kind)
    before = np.full(n, sentinel(dtype), dtype)
    d = api.DeviceArray.from_numpy(before)
    try:
        api.vnrNeuralVolumeDecodeToDeviceCorrected(volume or trained()[1], corr, d.ptr + offset * before.dtype.itemsize, strides, verify_params=verify)
        return d.numpy(), before, offset, strides
    finally:
        d.free()


def set_chunk(monkeypatch, chunk):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    if chunk:
        monkeypatch.setenv("VNR_AMD_DECODE_CHUNK", chunk)


def check_report(info, want):
    for k in ("n_flagged", "n_voxels_flagged", "n_nan", "payload_bytes", "kind"):
        assert info[k] == want[k], (k, info[k], want[k])
    for k in ("max_abs_before", "max_abs_after"):
        assert info[k] == want[k] or (np.isnan(info[k]) and np.isnan(want[k])), (k, info[k], want[k])
    assert info["worst_after"] == want["worst_after"]
    assert info["serialized_bytes"] == len(want["bytes"]) and info["n_cells"] == N_CELLS and info["dims"] == DIMS


def check_bound(corrected, ref, dec, eps):
    if corrected.dtype.kind != "f":
        assert int(np.abs(corrected.astype(np.int64) - ref.astype(np.int64)).max()) <= int(np.floor(eps))
    elif eps > 0:
        ok = ~np.isnan(ref.astype(np.float64) - dec.astype(np.float64))
        err = np.abs(corrected.astype(np.float64) - ref.astype(np.float64))
        assert (err[ok] <= ebr.float_bound(corrected, ref, dec, eps)[ok]).all()
    else:
        assert same_bytes(corrected, ref)


# ------------------------------------------------------------------------------------------------ 1 - 3. bytes, apply, report
@pytest.mark.parametrize("chunk", [None, CHUNK])
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("dtype", TYPES)
def test_serialised_bytes_equal_numpy_bit_for_bit(monkeypatch, dtype, kind, chunk):
    set_chunk(monkeypatch, chunk)
    eps = mixed_eps(dtype)
    ref, want = expected(dtype, eps)
    assert 0 < want["n_flagged"] < N_CELLS
    corr = device_build(ref, dtype, kind, eps)
    info = corr.info()
    assert 0 < info["n_flagged"] < N_CELLS
    assert corr.to_bytes() == want["bytes"]
    corr.release()


@pytest.mark.parametrize("chunk", [None, CHUNK])
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("dtype", TYPES)
def test_apply_equals_numpy_and_touches_nothing_else(monkeypatch, dtype, kind, chunk):
    set_chunk(monkeypatch, chunk)
    eps = mixed_eps(dtype)
    ref, want = expected(dtype, eps)
    corr = device_build(ref, dtype, "dense", eps)
    got, expect, offset, strides = device_apply(corr, dtype, kind)
    box_view(expect, offset, strides)[...] = want["corrected"]
    assert same_bytes(got, expect)
    assert not same_bytes(want["corrected"], decoded(dtype))      # the correction did something
    check_bound(box_view(got, offset, strides), ref, decoded(dtype), eps)
    # ... and from the serialised bytes alone (uploaded at the first use)
    loaded = api.Correction.from_bytes(corr.to_bytes())
    got2, _, _, _ = device_apply(loaded, dtype, kind)
    assert same_bytes(got2, expect)
    li = loaded.info()
    assert np.isnan(li["max_abs_before"]) and li["worst_after"] == (-1, -1, -1) and li["n_nan"] == 0 and li["max_abs_after"] == want["max_abs_after"]
    corr.release(); loaded.release()


@pytest.mark.parametrize("chunk", [None, CHUNK])
@pytest.mark.parametrize("kind", ["dense", "ghost"])
@pytest.mark.parametrize("dtype", TYPES)
def test_report_equals_numpy_exactly(monkeypatch, dtype, kind, chunk):
    set_chunk(monkeypatch, chunk)
    eps = mixed_eps(dtype)
    ref, want = expected(dtype, eps)
    corr = device_build(ref, dtype, kind, eps)
    info = corr.info()
    print(np.dtype(dtype).name, kind, {k: info[k] for k in ("n_flagged", "n_voxels_flagged", "payload_bytes", "max_abs_before", "max_abs_after", "worst_after")})
    check_report(info, want)
    assert info["max_abs_before"] == block_map(dtype)["max_abs"]
    assert info["params_hash"] == params_id()[0] and info["n_params"] == params_id()[1]
    assert info["eps"] == eps and (info["range_lo"], info["range_hi"]) == tuple(float(np.float32(x)) for x in RANGES[dtype])
    corr.release()


@pytest.mark.parametrize("dtype", [np.uint32, np.float32])
def test_code_widths_one_two_and_four_bytes(monkeypatch, dtype):
    """the tolerance is the largest error over 50, 2 000 and 100 000 (the float32 case beside the issue's uint32: kind 1 with wide codes)"""
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    seen = set()
    for divisor in (50, 2000, 100000):
        eps = block_map(dtype)["max_abs"] / divisor
        ref, want = expected(dtype, eps)
        corr = device_build(ref, dtype, "ghost", eps)
        assert corr.to_bytes() == want["bytes"]
        check_report(corr.info(), want)
        got, expect, offset, strides = device_apply(corr, dtype, "ghost")
        box_view(expect, offset, strides)[...] = want["corrected"]
        assert same_bytes(got, expect)
        check_bound(want["corrected"], ref, decoded(dtype), eps)
        seen.update(w for _, w in want["cells"])
        corr.release()
    assert seen == {1, 2, 4}, seen


# ------------------------------------------------------------------------------------------------ 4. eps = 0
@pytest.mark.parametrize("kind", ["dense", "ghost"])
@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.uint32])
def test_eps_zero_gives_integers_back_exactly(monkeypatch, dtype, kind):
    set_chunk(monkeypatch, CHUNK)
    ref, want = expected(dtype, 0.0)
    corr = device_build(ref, dtype, kind, 0.0)
    assert corr.to_bytes() == want["bytes"]
    check_report(corr.info(), want)
    assert corr.info()["max_abs_after"] == 0.0
    got, expect, offset, strides = device_apply(corr, dtype, kind)
    box_view(expect, offset, strides)[...] = ref
    assert same_bytes(got, expect)
    corr.release()


@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_eps_zero_gives_floats_back_bit_for_bit(monkeypatch, dtype, kind):
    set_chunk(monkeypatch, CHUNK)
    nan = np.frombuffer(np.array([0x7fc12345 if dtype == np.float32 else 0x7ff8000000abcdef], np.uint32 if dtype == np.float32 else np.uint64).tobytes(), dtype)[0]
    plant = (((3, 4, 5), nan), ((17, 20, 33), dtype(-0.0)))
    ref, want = expected(dtype, 0.0, plant)
    assert want["kind"] == 2 and want["n_nan"] == 1 and {w for _, w in want["cells"]} == {np.dtype(dtype).itemsize}
    corr = device_build(ref, dtype, kind, 0.0)
    assert corr.to_bytes() == want["bytes"]
    check_report(corr.info(), want)
    got, expect, offset, strides = device_apply(corr, dtype, kind)
    box_view(expect, offset, strides)[...] = want["corrected"]
    assert same_bytes(got, expect)
    # (an unflagged cell is one whose voxels were bit-identical already) the field itself, NaN payload and -0.0 included
    assert same_bytes(np.ascontiguousarray(box_view(got, offset, strides)), ref)
    assert same_bytes(want["corrected"][3, 4, 5:6], ref[3, 4, 5:6]) and same_bytes(want["corrected"][17, 20, 33:34], ref[17, 20, 33:34])
    corr.release()


# ------------------------------------------------------------------------------------------------ 5. nothing to correct
@pytest.mark.parametrize("dtype", TYPES)
def test_a_tolerance_nothing_misses_is_the_header_alone_and_the_plain_decode(monkeypatch, dtype):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    eps = block_map(dtype)["max_abs"]
    ref, want = expected(dtype, eps)
    corr = device_build(ref, dtype, "ghost", eps)
    info = corr.info()
    assert info["n_flagged"] == 0 and info["payload_bytes"] == 0 and info["max_abs_after"] == info["max_abs_before"] == eps
    b = corr.to_bytes()
    assert len(b) == ebr.HEADER.size and b == want["bytes"]
    check_report(info, want)
    for kind in LAYOUTS:
        got, expect, offset, strides = device_apply(corr, dtype, kind)
        box_view(expect, offset, strides)[...] = decoded(dtype)
        assert same_bytes(got, expect)
    corr.release()


# ------------------------------------------------------------------------------------------------ 7. a NaN in the reference
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_nan_in_the_reference_is_counted_and_stays_as_decoded(monkeypatch, dtype):
    set_chunk(monkeypatch, CHUNK)
    eps = mixed_eps(dtype)
    flagged_cells = dict(expected(dtype, eps)[1]["cells"])
    cell, sl = next((c, s) for c, s in ebr.cells_of(DIMS) if c in flagged_cells)      # a voxel of a cell that is flagged anyway
    at = (sl[0].start + 1, sl[1].start + 2, sl[2].start + 3)
    ref, want = expected(dtype, eps, ((at, dtype(np.nan)),))
    assert want["n_nan"] == 1 and cell in dict(want["cells"])
    corr = device_build(ref, dtype, "ghost", eps)
    assert corr.to_bytes() == want["bytes"]
    check_report(corr.info(), want)
    got, expect, offset, strides = device_apply(corr, dtype, "ghost")
    box_view(expect, offset, strides)[...] = want["corrected"]
    assert same_bytes(got, expect)
    assert same_bytes(box_view(got, offset, strides)[at[0], at[1], at[2]:at[2] + 1], decoded(dtype)[at[0], at[1], at[2]:at[2] + 1])
    check_bound(np.ascontiguousarray(box_view(got, offset, strides)), ref, decoded(dtype), eps)
    corr.release()


# ------------------------------------------------------------------------------------------------ 8. verify_params
def test_verify_params_refuses_after_one_more_training_step():
    _, nv = train(20)
    dtype = np.uint8
    d = api.DeviceArray.from_numpy(field(dtype).ravel())
    corr = api.vnrNeuralVolumeBuildCorrection(nv, d, dtype, 1.0, None, RANGES[dtype])
    d.free()
    assert corr.info()["n_flagged"] > 0
    first, _, _, _ = device_apply(corr, dtype, "dense", nv, verify=True)
    assert int(np.abs(first.astype(np.int64) - field(dtype).ravel().astype(np.int64)).max()) <= 1
    api.vnrNeuralVolumeTrain(nv, 1, True)
    with pytest.raises(api.VnrAmdError, match="not the ones the correction was built on"):
        device_apply(corr, dtype, "dense", nv, verify=True)
    before = np.full(N, sentinel(dtype), dtype)
    out = api.DeviceArray.from_numpy(before)
    st = api.lib().vnrAmdNeuralVolumeDecodeToDeviceCorrected(nv.h, corr.h, C.c_void_p(out.ptr), None, None, 1)
    assert st != 0 and same_bytes(out.numpy(), before)
    st = api.lib().vnrAmdNeuralVolumeDecodeToDeviceCorrected(nv.h, corr.h, C.c_void_p(out.ptr), None, None, 0)      # the caller vouches
    assert st == 0 and not same_bytes(out.numpy(), before)
    out.free(); corr.release()


# ------------------------------------------------------------------------------------------------ 9. refusals
def raw_build(v, ptr, vtype=8, strides=None, rng=(1.0, 0.0), eps=0.5):
    s = (C.c_int64 * 3)(*strides) if strides is not None else None
    h = api.lib().vnrAmdNeuralVolumeBuildCorrection(v.h if v else None, C.c_void_p(ptr), vtype, s, rng[0], rng[1], eps, None)
    msg = api._lib.last_error()
    if h:
        api.lib().vnrAmdReleaseCorrection(h)
    return h, msg


def raw_apply(v, corr, ptr, strides=None, verify=0):
    s = (C.c_int64 * 3)(*strides) if strides is not None else None
    st = api.lib().vnrAmdNeuralVolumeDecodeToDeviceCorrected(v.h if v else None, corr.h if corr else None, C.c_void_p(ptr), s, None, verify)
    return st, api._lib.last_error()


BUILD_REFUSALS = [
    (dict(eps=-1.0), "eps must be a finite tolerance"), (dict(eps=float("nan")), "eps must be a finite tolerance"), (dict(eps=float("inf")), "eps must be a finite tolerance"),
    (dict(ptr=0), "null device data"), (dict(simple=True), "expecting a neural volume"), (dict(null_volume=True), "null volume"),
    (dict(strides=(1, 0, 960)), "strides must be positive"), (dict(strides=(1, 39, 960)), "overlap"), (dict(strides=(2, 3, 960)), "overlap"),
    (dict(vtype=6), "64-bit"), (dict(vtype=9), "vector"), (dict(vtype=13), "unknown value type"),
    (dict(vtype=0), "needs a value range"), (dict(rng=(2.0, 2.0)), "range_lo == range_hi"),
    (dict(misalign=2), "not aligned"), (dict(strides=(1, 40, 2000)), "allocation"),
    (dict(chunk="many"), "VNR_AMD_DECODE_CHUNK"),
]


@pytest.mark.parametrize("kw,word", BUILD_REFUSALS, ids=[f"{i}-{r[1].split()[0]}" for i, r in enumerate(BUILD_REFUSALS)])
def test_build_and_apply_refusals_name_the_cause_and_write_nothing(monkeypatch, kw, word):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    sv, nv = trained()
    kw = dict(kw)
    if "chunk" in kw:
        monkeypatch.setenv("VNR_AMD_DECODE_CHUNK", kw.pop("chunk"))
    volume = None if kw.pop("null_volume", False) else (sv if kw.pop("simple", False) else nv)
    before = np.full(N, sentinel(np.float32), np.float32)
    d = api.DeviceArray.from_numpy(before)
    ptr = kw.pop("ptr", d.ptr) and d.ptr + kw.pop("misalign", 0)
    h, msg = raw_build(volume, ptr, **kw)
    assert not h and word in msg, msg
    assert same_bytes(d.numpy(), before)
    # the apply has the decode's refusals too (its type and range are the correction's: float32 here)
    if "eps" not in kw and "vtype" not in kw and "rng" not in kw:
        corr = api.Correction.from_bytes(expected(np.float32, mixed_eps(np.float32))[1]["bytes"])
        st, msg = raw_apply(volume, corr, ptr, kw.get("strides"))
        assert st != 0 and word in msg, msg
        assert same_bytes(d.numpy(), before)
        corr.release()
    d.free()


def test_codes_wider_than_32_bits_are_refused():
    dtype = np.uint32
    ref = field(dtype).copy()
    at = np.unravel_index(int(np.argmin(decoded(dtype))), ref.shape)
    ref[at] = 4294967295
    assert int(ref[at]) - int(decoded(dtype)[at]) > 2 ** 31 - 1
    with pytest.raises(api.VnrAmdError, match="codes wider than 32 bits"):
        device_build(ref, dtype, "dense", 0.0)
    with pytest.raises(ValueError, match="wider than 32 bits"):
        ebr.build(decoded(dtype).copy(), ref, 0.0, RANGES[dtype])
    device_build(ref, dtype, "dense", 1.0).release()      # 2^32 / 3 fits


def test_apply_refuses_other_dims_a_null_handle_and_malformed_bytes():
    nv = trained()[1]
    before = np.full(N, sentinel(np.float32), np.float32)
    d = api.DeviceArray.from_numpy(before)
    other = (17, 16, 33)
    rng = np.random.default_rng(1)
    dec = rng.uniform(0, 1, other[::-1]).astype(np.float32)
    blob = ebr.build(dec, (dec + rng.normal(0, 0.1, dec.shape)).astype(np.float32), 0.05, (0.0, 1.0))["bytes"]
    corr = api.Correction.from_bytes(blob)
    st, msg = raw_apply(nv, corr, d.ptr)
    assert st != 0 and "differ from the volume's" in msg, msg
    st, msg = raw_apply(nv, None, d.ptr)
    assert st != 0 and "null correction" in msg, msg
    assert same_bytes(d.numpy(), before)
    with pytest.raises(api.VnrAmdError, match="malformed correction bytes"):
        api.Correction.from_bytes(blob[:-3])
    with pytest.raises(api.VnrAmdError, match="malformed correction bytes"):
        api.Correction.from_bytes(b"VNRCORR1" + blob[8:12][::-1] + blob[12:])
    corr.release(); d.free()
