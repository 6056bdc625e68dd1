"""In-situ round trip (include/vnr_amd.h "in-situ round trip"): vnrAmdNeuralVolumeDecodeToDevice and
vnrAmdNeuralVolumeErrorAgainstDevice against vnrAmdNeuralVolumeInference and numpy.

The decode evaluates the network at coordinates built by the arithmetic numpy restates here in float32, and converts every value
by IEEE operations the header spells out one by one (one fp32 product, one fp32 sum, rint of the double, a clamp), so every
comparison has tolerance ZERO except the two double sums of the error report: they are added in another order than numpy's, and
two sums of n <= 19 200 non-negative doubles in different orders differ by at most 2 n 2^-53 = 4.3e-12 relative; the bound used is
1e-11.

Volume (40, 24, 20): x-rows of 40 elements (2.5 16-byte pieces of uint8, 10 of float32), nothing a multiple of 16, ragged
macrocells 3 x 2 x 2.  VNR_AMD_DECODE_CHUNK = 7001 gives 3 chunks, the last one ragged, none ending at the end of a row.

One item of the refusal list cannot be reached through the API and has no case here: a neural volume without a valid network
(every way to create or re-model one either yields parameters or fails)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

pytestmark = pytest.mark.gpu

DIMS = (40, 24, 20)
N = DIMS[0] * DIMS[1] * DIMS[2]
SUB_LO, SUB_SIZE = (3, 5, 2), (17, 9, 6)
CHUNK = "7001"
DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
# ranges that make both saturations act for the integers once the network's output leaves [0.1, 0.9]
RANGES = {np.uint8: (-40.0, 300.0), np.int8: (-160.0, 160.0), np.uint16: (-10000.0, 80000.0), np.int16: (-41000.0, 41000.0),
          np.uint32: (-1.0e9, 5.5e9), np.int32: (-2.7e9, 2.7e9), np.float32: (-3.5, 12.25), np.float64: (-1.0e3, 2.5e3)}
LAYOUTS = ["dense", "ghost", "sx2"]


def ground_truth():
    """[z, y, x] float32 in [0, 1] with plateaus at both ends, so that a small network reaches below 0.1 and above 0.9.  The crop
    is centred on the field's blob: the sub-box of case 3 then spans the whole interval (202 distinct uint8 levels), so that its
    error report cannot come out as all zeros, as it could over a box that lies inside the lower plateau."""
    z0, y0 = (40 - DIMS[2]) // 2, (40 - DIMS[1]) // 2
    a = syn.analytic_volume(40)[z0:z0 + DIMS[2], y0:y0 + DIMS[1], :DIMS[0]]
    a = (a - a.min()) / (a.max() - a.min())
    return np.clip(np.float32(1.6) * a - np.float32(0.3), 0, 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def trained():
    """-> (simple volume, neural volume): the small model of the issue, trained a few hundred steps; shared and left unchanged"""
    before = {k: os.environ.get(k) for k in ("VNR_AMD_INIT_SEED", "VNR_AMD_DECODE_CHUNK")}
    os.environ["VNR_AMD_INIT_SEED"] = "4711"
    os.environ.pop("VNR_AMD_DECODE_CHUNK", None)
    try:
        sv = api.vnrCreateSimpleVolume(ground_truth(), value_range=(0.0, 1.0))
        cfg = syn.model_config(n_levels=4, n_features=2, log2_hashmap_size=12, base_resolution=4, n_neurons=16, n_hidden_layers=1)
        nv = api.vnrCreateNeuralVolume(cfg, sv)
        api.check(api.lib().vnrAmdNeuralVolumeSetSamplerSeed(nv.h, 99, 7))
        api.vnrNeuralVolumeTrain(nv, 400, True)
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return sv, nv


def coords(grid, lo, size):
    """float32 voxel centres [n, 3] of a box, x fastest: ((float)(lo + i) + 0.5f) * (1.0f / (float)grid)"""
    ax = [(np.arange(lo[a], lo[a] + size[a]).astype(np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(grid[a])) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(grid=DIMS, lo=(0, 0, 0), size=DIMS):
    """vnrAmdNeuralVolumeInference on numpy-built coordinates -> [z, y, x] float32; computed once, read only"""
    v = api.neural_inference(trained()[1], coords(grid, lo, size)).reshape(size[::-1])
    v.setflags(write=False)
    return v


def convert(v, dtype, value_range):
    """the header's conversion, step by step"""
    d = np.asarray(v, np.float32)
    if value_range is not None:
        lo, hi = np.float32(value_range[0]), np.float32(value_range[1])
        d = (d * np.float32(hi - lo)).astype(np.float32) + lo
        assert d.dtype == np.float32
    if np.issubdtype(dtype, np.floating):
        return d.astype(dtype)
    r = np.rint(d.astype(np.float64))
    r = np.where(np.isnan(r), 0.0, r)
    info = np.iinfo(dtype)
    return np.clip(r, float(info.min), float(info.max)).astype(dtype)


def sentinel(dtype):
    return np.frombuffer(b"\xa5" * np.dtype(dtype).itemsize, dtype)[0]


def layout(kind, size):
    """-> (elements of the array, element offset of the box's first voxel, strides or None)"""
    bx, by, bz = size
    if kind == "dense":
        return bx * by * bz, 0, None
    if kind == "ghost":   # 2 + 3 ghost elements per row: an odd row length of 45 puts the row starts on every residue of a 16-byte line
        sy, sz = bx + 5, (bx + 5) * (by + 3)
        return sz * (bz + 2), 2 + sy + sz, (1, sy, sz)
    sy, sz = 2 * bx + 3, (2 * bx + 3) * (by + 1)
    return sz * (bz + 1), 1, (2, sy, sz)


def box_view(flat, offset, strides, size):
    bx, by, bz = size
    sx, sy, sz = strides or (1, bx, bx * by)
    it = flat.dtype.itemsize
    return np.lib.stride_tricks.as_strided(flat[offset:], shape=(bz, by, bx), strides=(sz * it, sy * it, sx * it))


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def decode(dtype, kind="dense", box=None, grid_dims=None, value_range=None):
    """-> (whole destination array as it is after the call, flat; the same array as numpy expects it to be untouched, flat; offset; strides)"""
    size = box[1] if box else (grid_dims or DIMS)
    n, offset, strides = layout(kind, size)
    before = np.full(n, sentinel(dtype), dtype)
    d = api.DeviceArray.from_numpy(before)
    api.vnrNeuralVolumeDecodeToDevice(trained()[1], d.ptr + offset * before.dtype.itemsize, dtype, strides, box, grid_dims, value_range)
    got = d.numpy()
    d.free()
    return got, before, offset, strides


# ------------------------------------------------------------------------------------------------ 1. float32, no range, dense, whole grid
def test_reference_values_span_the_unit_interval():
    v = reference()
    print("reference min", float(v.min()), "max", float(v.max()))
    assert v.min() < 0.1 and v.max() > 0.9     # otherwise the saturation cases below are empty


@pytest.mark.parametrize("chunk", [None, CHUNK])
def test_float32_decode_equals_inference_bit_for_bit(monkeypatch, chunk):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    if chunk:
        monkeypatch.setenv("VNR_AMD_DECODE_CHUNK", chunk)
        assert -(-N // int(chunk)) >= 3 and N % int(chunk) != 0
    got, _, _, _ = decode(np.float32)
    assert same_bytes(got.reshape(DIMS[::-1]), reference())


def test_float32_decode_equals_the_progressively_decoded_volume():
    nv = trained()[1]
    for _ in range(api.vnrNeuralVolumeGetNumberOfBlobs(nv)):
        api.vnrNeuralVolumeDecodeProgressive(nv)
    got, _, _, _ = decode(np.float32)
    assert same_bytes(got.reshape(DIMS[::-1]), api.neural_decoded_volume(nv, DIMS))


# ------------------------------------------------------------------------------------------------ 2. every type x every layout
@pytest.mark.parametrize("chunk", [None, CHUNK])
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_type_and_layout_equals_numpy_and_touches_nothing_else(monkeypatch, dtype, kind, chunk):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    if chunk:
        monkeypatch.setenv("VNR_AMD_DECODE_CHUNK", chunk)
    want_box = convert(reference(), dtype, RANGES[dtype])
    if np.issubdtype(dtype, np.integer):      # both saturations act
        assert (want_box == np.iinfo(dtype).min).any() and (want_box == np.iinfo(dtype).max).any()
        assert len(np.unique(want_box)) > 50
    got, want, offset, strides = decode(dtype, kind, value_range=RANGES[dtype])
    if kind == "ghost":                       # row starts on every residue of a 16-byte line the type can have (relative to the 256-byte aligned allocation)
        it = np.dtype(dtype).itemsize
        starts = {((offset + y * strides[1] + z * strides[2]) * it) % 16 for y in range(DIMS[1]) for z in range(DIMS[2])}
        assert starts == set(range(0, 16, it))
    box_view(want, offset, strides, DIMS)[...] = want_box
    assert same_bytes(got, want)


def test_float_types_without_a_range_store_the_output_as_it_is():
    for dtype in (np.float32, np.float64):
        for kind in LAYOUTS:
            got, want, offset, strides = decode(dtype, kind)
            box_view(want, offset, strides, DIMS)[...] = reference().astype(dtype)
            assert same_bytes(got, want)


# ------------------------------------------------------------------------------------------------ 3. sub-box, other grids
@pytest.mark.parametrize("grid", [DIMS, tuple(2 * d for d in DIMS)])
@pytest.mark.parametrize("kind", LAYOUTS)
def test_sub_box_equals_inference_at_its_coordinates(grid, kind):
    got, want, offset, strides = decode(np.float32, kind, box=(SUB_LO, SUB_SIZE), grid_dims=grid)
    box_view(want, offset, strides, SUB_SIZE)[...] = reference(grid, SUB_LO, SUB_SIZE)
    assert same_bytes(got, want)


def test_coarse_preview_grid():
    grid = (13, 7, 5)
    got, _, _, _ = decode(np.float32, grid_dims=grid)
    assert same_bytes(got.reshape(grid[::-1]), reference(grid, (0, 0, 0), grid))


# ------------------------------------------------------------------------------------------------ 4. error report
def reference_field(dtype):
    """the field the network stands for, in data units of `dtype` -> ([z, y, x] array, value range)"""
    if dtype == np.uint8:
        return np.rint(ground_truth() * np.float32(255.0)).astype(np.uint8), (0.0, 255.0)
    lo, hi = RANGES[np.float32]
    return (ground_truth() * np.float32(hi - lo) + np.float32(lo)).astype(np.float32), (lo, hi)


def numpy_report(decoded, ref, lo):
    """decoded, ref: [z, y, x] arrays of the box; lo: the box's lower corner -> the report numpy gives"""
    e = decoded.astype(np.float64) - ref.astype(np.float64)
    a = np.abs(e)
    k = int(np.argmax(a))                       # the first of equals in x-fastest order
    z, y, x = np.unravel_index(k, a.shape)
    mc = tuple(-(-d // 16) for d in DIMS)
    cells = np.zeros(mc[::-1], np.float32)
    for (zz, yy, xx), v in np.ndenumerate(a):
        c = ((lo[2] + zz) >> 4, (lo[1] + yy) >> 4, (lo[0] + xx) >> 4)
        cells[c] = max(cells[c], np.float32(v))
    return {"n_voxels": a.size, "max_abs": float(a.max()), "worst": (lo[0] + int(x), lo[1] + int(y), lo[2] + int(z)),
            "sum_abs": float(a.sum()), "sum_sq": float((e * e).sum()), "block_max": cells}


def report(ref_box, dtype, kind, box, value_range):
    size = box[1] if box else DIMS
    n, offset, strides = layout(kind, size)
    flat = np.full(n, sentinel(dtype), dtype)
    box_view(flat, offset, strides, size)[...] = ref_box
    d = api.DeviceArray.from_numpy(flat)
    out = api.vnrNeuralVolumeErrorAgainstDevice(trained()[1], d.ptr + offset * flat.dtype.itemsize, dtype, strides, box, value_range, block_map=True)
    d.free()
    return out


@pytest.mark.parametrize("chunk", [None, CHUNK])
@pytest.mark.parametrize("box", [None, (SUB_LO, SUB_SIZE)])
@pytest.mark.parametrize("kind", ["dense", "ghost"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_error_report_equals_numpy_on_the_decoded_voxels(monkeypatch, dtype, kind, box, chunk):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    if chunk:
        monkeypatch.setenv("VNR_AMD_DECODE_CHUNK", chunk)
    field, rng = reference_field(dtype)
    lo, size = box if box else ((0, 0, 0), DIMS)
    sl = tuple(slice(lo[a], lo[a] + size[a]) for a in (2, 1, 0))
    decoded, _, _, _ = decode(dtype, box=box, value_range=rng)     # DecodeToDevice's own output
    decoded = decoded.reshape(size[::-1])
    assert same_bytes(decoded, convert(reference()[sl], dtype, rng))
    ref_box = field[sl].copy()

    def check(ref_box):
        want, got = numpy_report(decoded, ref_box, lo), report(ref_box, dtype, kind, box, rng)
        print(dtype.__name__, kind, box, {k: got[k] for k in ("n_voxels", "max_abs", "worst", "sum_abs", "sum_sq", "psnr_db")})
        assert got["n_voxels"] == want["n_voxels"] == size[0] * size[1] * size[2]
        assert got["max_abs"] == want["max_abs"] and got["max_abs"] > 0
        assert got["worst"] == want["worst"]
        assert same_bytes(got["block_max"], want["block_max"])
        assert abs(got["sum_abs"] - want["sum_abs"]) <= 1e-11 * want["sum_abs"]
        assert abs(got["sum_sq"] - want["sum_sq"]) <= 1e-11 * want["sum_sq"]
        width = float(np.float32(rng[1])) - float(np.float32(rng[0]))
        assert got["psnr_db"] == pytest.approx(10.0 * np.log10(width * width * got["n_voxels"] / got["sum_sq"]), rel=1e-12)
        return got

    plain = check(ref_box)
    if box:                                     # cells the box does not reach hold 0
        assert (plain["block_max"][:, :, 2] == 0).all() and (plain["block_max"] > 0).any()
    # one planted voxel far from its value is the worst one, and shows in exactly one block
    px, py, pz = 11, 9, 4
    at = (pz - lo[2], py - lo[1], px - lo[0])
    width = rng[1] - rng[0]
    assert plain["max_abs"] < 0.45 * width     # the planted error below is larger than every natural one
    if dtype == np.uint8:
        ref_box[at] = 0 if decoded[at] > 127 else 255
    else:
        ref_box[at] = decoded[at] + np.float32(0.75 * width)
    planted = check(ref_box)
    assert planted["worst"] == (px, py, pz) and planted["max_abs"] > plain["max_abs"]
    assert int((planted["block_max"] != plain["block_max"]).sum()) == 1
    assert planted["block_max"][pz >> 4, py >> 4, px >> 4] == np.float32(planted["max_abs"])


def test_error_report_without_a_range_and_with_a_nan():
    ref = reference().copy()
    ref[3, 4, 5] += np.float32(0.25)
    e = abs(float(reference()[3, 4, 5]) - float(ref[3, 4, 5]))      # every other voxel's error is exactly 0
    out = report(ref, np.float32, "dense", None, None)
    assert out["max_abs"] == e and out["worst"] == (5, 4, 3) and out["sum_abs"] == e and out["sum_sq"] == e * e
    assert out["psnr_db"] == pytest.approx(10.0 * np.log10(N / (e * e)), rel=1e-12)       # a range of 1
    assert int((out["block_max"] != 0).sum()) == 1 and out["block_max"][0, 0, 0] == np.float32(e)
    ref[7, 8, 9] = np.nan                       # the sums say so; the maximum is that of the other voxels
    out = report(ref, np.float32, "dense", None, None)
    assert np.isnan(out["sum_abs"]) and np.isnan(out["sum_sq"]) and np.isnan(out["psnr_db"])
    assert out["max_abs"] == e and out["worst"] == (5, 4, 3)
    assert int((out["block_max"] != 0).sum()) == 1


# ------------------------------------------------------------------------------------------------ 5. refusals
def raw_decode(v, ptr, vtype=8, strides=None, lo=None, size=None, grid=None, rng=(1.0, 0.0)):
    i3 = lambda t: (C.c_int * 3)(*t) if t is not None else None
    s = (C.c_int64 * 3)(*strides) if strides is not None else None
    st = api.lib().vnrAmdNeuralVolumeDecodeToDevice(v.h if v else None, C.c_void_p(ptr), vtype, s, i3(lo), i3(size), i3(grid), rng[0], rng[1], None)
    return st, api._lib.last_error()


def raw_error(v, ptr, vtype=8, strides=None, lo=None, size=None, rng=(1.0, 0.0), out=True, cells=None):
    i3 = lambda t: (C.c_int * 3)(*t) if t is not None else None
    s = (C.c_int64 * 3)(*strides) if strides is not None else None
    e = api._lib.DecodeError()
    st = api.lib().vnrAmdNeuralVolumeErrorAgainstDevice(v.h if v else None, C.c_void_p(ptr), vtype, s, i3(lo), i3(size), rng[0], rng[1], None,
                                                        C.byref(e) if out else None, cells)
    return st, api._lib.last_error()


REFUSALS = [
    # (keyword arguments of raw_decode / raw_error, a word of the message, applies to the error report as well)
    (dict(ptr=0), "null device data", True),
    (dict(simple=True), "expecting a neural volume", True),
    (dict(null_volume=True), "null volume", True),
    (dict(lo=(30, 0, 0), size=(11, 4, 4)), "outside the grid", True),
    (dict(lo=(-1, 0, 0), size=(4, 4, 4)), "outside the grid", True),
    (dict(lo=(0, 0, 0), size=(4, 0, 4)), "box sizes must be positive", True),
    (dict(lo=(0, 0, 0)), "box_lo and box_size go together", True),
    (dict(grid=(40, -24, 20)), "grid dimensions must be positive", False),
    (dict(strides=(1, 0, 960)), "strides must be positive", True),
    (dict(strides=(1, 39, 960)), "overlap", True),
    (dict(strides=(1, 40, 959)), "overlap", True),
    (dict(strides=(2, 3, 960)), "overlap", True),
    (dict(vtype=6), "64-bit", True), (dict(vtype=7), "64-bit", True), (dict(vtype=9), "vector", True), (dict(vtype=13), "unknown value type", True),
    (dict(vtype=0), "needs a value range", True), (dict(vtype=5), "needs a value range", True),
    (dict(rng=(2.0, 2.0)), "range_lo == range_hi", True), (dict(vtype=2, rng=(7.0, 7.0)), "range_lo == range_hi", True),
    (dict(vtype=8, misalign=2), "not aligned", True), (dict(vtype=12, misalign=4), "not aligned", True), (dict(vtype=2, misalign=1, rng=(0.0, 9.0)), "not aligned", True),
    (dict(strides=(1, 40, 2000)), "allocation", True),
    (dict(chunk="many"), "VNR_AMD_DECODE_CHUNK", True), (dict(chunk="0"), "VNR_AMD_DECODE_CHUNK", True),
]


@pytest.mark.parametrize("kw,word,both", REFUSALS, ids=[f"{i}-{r[1].split()[0]}" for i, r in enumerate(REFUSALS)])
def test_refusals_name_the_cause_and_write_nothing(monkeypatch, kw, word, both):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    sv, nv = trained()
    kw = dict(kw)
    if "chunk" in kw:
        monkeypatch.setenv("VNR_AMD_DECODE_CHUNK", kw.pop("chunk"))
    volume = None if kw.pop("null_volume", False) else (sv if kw.pop("simple", False) else nv)
    before = np.full(N, sentinel(np.float32), np.float32)
    d = api.DeviceArray.from_numpy(before)            # room for the whole grid in every type but double
    ptr = kw.pop("ptr", d.ptr) and d.ptr + kw.pop("misalign", 0)
    if kw.get("vtype") == 12:
        kw.setdefault("lo", (0, 0, 0)); kw.setdefault("size", (20, 24, 20))
    st, msg = raw_decode(volume, ptr, **kw)
    assert st != 0 and word in msg, msg
    assert same_bytes(d.numpy(), before)
    if both:
        kw.pop("grid", None)
        cells = api.DeviceArray((12,), np.float32)
        cells.upload(np.full(12, 7.0, np.float32))
        st, msg = raw_error(volume, ptr, cells=cells.ptr, **kw)
        assert st != 0 and word in msg, msg
        assert same_bytes(cells.numpy(), np.full(12, 7.0, np.float32))
        cells.free()
    d.free()
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    got, _, _, _ = decode(np.float32)                  # the volume is as it was
    assert same_bytes(got.reshape(DIMS[::-1]), reference())


def test_error_report_refuses_a_null_result_and_a_short_block_map():
    nv = trained()[1]
    d = api.DeviceArray.from_numpy(np.zeros(N, np.float32))
    st, msg = raw_error(nv, d.ptr, out=False)
    assert st != 0 and "null result" in msg
    cells = api.DeviceArray((4,), np.float32)          # the macrocell has 3 x 2 x 2 = 12 cells
    st, msg = raw_error(nv, d.ptr, cells=cells.ptr)
    assert st != 0 and "block map" in msg and "allocation" in msg
    d.free(); cells.free()


def test_wrapper_refuses_through_the_library_with_a_vnr_amd_error():
    sv, nv = trained()
    d = api.DeviceArray((N,), np.float32)
    with pytest.raises(api.VnrAmdError, match="expecting a neural volume"):
        api.vnrNeuralVolumeDecodeToDevice(sv, d, np.float32)
    with pytest.raises(api.VnrAmdError, match="outside the grid"):
        api.vnrNeuralVolumeDecodeToDevice(nv, d, np.float32, box=((39, 0, 0), (2, 1, 1)))
    with pytest.raises(api.VnrAmdError, match="outside the grid"):
        api.vnrNeuralVolumeErrorAgainstDevice(nv, d, np.float32, box=((0, 23, 0), (1, 2, 1)))
    d.free()
