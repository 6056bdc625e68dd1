"""In-situ ground truth (include/vnr_amd.h "in-situ ground truth"): vnrAmdCreateSimpleVolumeFromDevice,
vnrAmdSimpleVolumeUpdateFromDevice and vnrAmdSimpleVolumeAppendTimeStepFromDevice against the host load path and numpy.

The device kernels do the host path's IEEE operations per voxel ((float)v, one subtraction, one correctly rounded division, two compares)
and an exact min / max, so every comparison here has tolerance ZERO.

The float and double data hold no negative zeros: with +0 and -0 both present the host's minimum depends on which of its threads saw
which zero first (std::min keeps the running value on a tie, and -0 == +0), so the host path is no yardstick for that case.

Which grid-stride trips the larger shape takes: the kernels cap the grid at 8 blocks per CU (2048 on the MI355X) and one block takes
256 16-byte pieces per trip, so (257, 130, 67) is 547 (1-byte types) to 4373 (double) block items: more than one trip for the 4- and 8-byte
types, many blocks for all."""
import ctypes as C
import functools

import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

pytestmark = pytest.mark.gpu

SMALL, LARGE = (33, 17, 9), (257, 130, 67)
DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
INTEGER = [d for d in DTYPES if np.issubdtype(d, np.integer)]

# per type: bulk interval [a, b) of the random data, the maximum (goes to the very FIRST voxel of the larger shape) and the minimum (the very
# LAST voxel).  The 32-bit integers and the doubles hold values fp32 cannot represent: 2^31 - 1, 2^25 + 1, 2^24 + 1, 2^32 - 101, thirds.
SPEC = {
    np.uint8: (3, 250, 255, 0), np.int8: (-100, 100, 127, -128), np.uint16: (100, 60000, 65535, 0), np.int16: (-30000, 30000, 32767, -32768),
    np.uint32: (2 ** 25, 2 ** 32 - 1024, 2 ** 32 - 101, 2 ** 24 + 1), np.int32: (-2 ** 31 + 1000, 2 ** 31 - 1000, 2 ** 31 - 1, -2 ** 31 + 1),
    np.float32: (-1.0e4, 1.0e4, 10000.5, -10000.25), np.float64: (-2.0e9, 2.0e9, 2.0 ** 31 - 1.0, -(2.0 ** 31 - 1.0) - 1.0 / 3.0),
}


@functools.lru_cache(maxsize=None)
def field(dtype, dims, seed=0):
    """seeded [z, y, x] array; read only (shared between the tests)"""
    rng = np.random.default_rng([seed, DTYPES.index(dtype), dims[0]])
    a, b, top, bottom = SPEC[dtype]
    shape = dims[::-1]
    if np.issubdtype(dtype, np.integer):
        v = rng.integers(a, b, shape, dtype=np.int64).astype(dtype)
    else:
        v = rng.uniform(a, b, shape).astype(dtype)
        v[v == 0] = 0           # no negative zeros (see the module docstring)
        v.flat[7::11] += dtype(1.0) / dtype(3.0)
    f = v.reshape(-1)
    if dtype in (np.uint32, np.int32, np.float64):   # not representable in fp32, in the middle of the data
        f[5] = dtype(2 ** 31 - 1)
        f[f.size // 2] = dtype(2 ** 25 + 1)
    if dims == LARGE:           # a lost block partial changes the range
        f[0], f[-1] = dtype(top), dtype(bottom)
    assert not np.any(np.signbit(v.astype(np.float64)) & (v == 0))
    v.setflags(write=False)
    return v


def norm(a, lo, hi):
    """the float32 expression of tests/test_scene.py::test_simple_volume_from_vidi_scene_with_time_steps"""
    return np.clip((a.astype(np.float32) - np.float32(lo)) / (np.float32(hi) - np.float32(lo)), 0, 1).astype(np.float32)


def data_range(a):
    """the host path's (float)(double) of the exact minimum / maximum"""
    return float(np.float32(np.float64(a.min()))), float(np.float32(np.float64(a.max())))


def explicit_range(a, variant):
    lo, hi = float(np.float64(a.min())), float(np.float64(a.max()))
    if variant == "inside":    # both clamps act
        return float(np.float32(lo + 0.25 * (hi - lo))), float(np.float32(lo + 0.75 * (hi - lo)))
    if variant == "wider":
        return float(np.float32(lo - 0.125 * (hi - lo) - 10.0)), float(np.float32(hi + 0.125 * (hi - lo) + 10.0))
    return None


def dims_of(a):
    return (a.shape[2], a.shape[1], a.shape[0])


def voxels(v, dims):
    p = api.lib().vnrAmdSimpleVolumeDeviceData(v.h)
    assert p
    out = np.empty(dims[::-1], np.float32)
    api.check(api.lib().vnrAmdMemcpyD2H(out.ctypes.data_as(C.c_void_p), p, out.nbytes))
    return out


def stored_range(v):
    r = np.zeros(2, np.float32)
    api.check(api.lib().vnrAmdSimpleVolumeGetDataRange(v.h, r.ctypes.data_as(C.POINTER(C.c_float))))
    return float(r[0]), float(r[1])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def tfn():
    colors, alphas = syn.tfn_ramp_with_bumps()
    t = api.vnrCreateTransferFunction()
    api.vnrTransferFunctionSetColor(t, colors)
    api.vnrTransferFunctionSetAlpha(t, alphas)
    api.vnrTransferFunctionSetValueRange(t, (0, 1))
    return t


def set_tfn(v, t):
    api.check(api.lib().vnrAmdVolumeUpdateMaxOpacity(v.h, t.h))


def from_device(a, value_range=None):
    d = api.DeviceArray.from_numpy(a)
    v, used = api.vnrCreateSimpleVolumeFromDevice(d, dims_of(a), a.dtype, value_range=value_range)
    d.free()
    return v, used


# ------------------------------------------------------------------------------------------------ 1. bit equality
CASES = [(dt, dims, var) for dt in DTYPES for dims in (SMALL, LARGE) for var in ("data", "inside", "wider")
         if var != "wider" or dt in INTEGER]


@pytest.mark.parametrize("dtype,dims,variant", CASES, ids=[f"{np.dtype(d).name}-{s[0]}-{v}" for d, s, v in CASES])
def test_device_ingest_equals_host_path_and_numpy(oracle, dtype, dims, variant):
    a = field(dtype, dims)
    rng = explicit_range(a, variant)
    want_range = data_range(a) if rng is None else rng
    if variant == "inside":
        assert want_range[0] > float(a.min()) and want_range[1] < float(a.max())
    if variant == "wider":
        assert want_range[0] < float(a.min()) and want_range[1] > float(a.max())
    want = norm(a, *want_range)
    host = api.vnrCreateSimpleVolume(a, value_range=rng)
    dev, used = from_device(a, rng)
    assert api.vnrVolumeGetDims(dev) == dims and api.vnrSimpleVolumeGetNumberOfTimeSteps(dev) == 1
    # the range: what was applied, what the volume reports, the host path's, numpy's
    assert np.array_equal(np.asarray(used, np.float32), np.asarray(want_range, np.float32)), (used, want_range)
    assert np.array_equal(np.asarray(stored_range(dev), np.float32), np.asarray(want_range, np.float32))
    assert np.array_equal(np.asarray(stored_range(host), np.float32), np.asarray(want_range, np.float32))
    # the voxels
    got, got_host = voxels(dev, dims), voxels(host, dims)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(got, got_host) and np.array_equal(bits(got), bits(got_host))
    if variant == "inside":
        assert (got == 0).any() and (got == 1).any()
    # the macrocell, and the max opacity under one transfer function
    t = tfn()
    set_tfn(dev, t)
    set_tfn(host, t)
    mc, mc_host = api.volume_macrocell(dev), api.volume_macrocell(host)
    assert mc["dims"] == mc_host["dims"]
    assert np.array_equal(mc["value_range"], mc_host["value_range"])
    assert np.array_equal(mc["max_opacity"], mc_host["max_opacity"])
    assert np.array_equal(mc["value_range"], oracle.macrocell_compute_implicit(want))


# ------------------------------------------------------------------------------------------------ 2. strides
BOX, PADDED, GHOST = (40, 24, 12), (46, 28, 20), (2, 1, 5)    # ghost layers: x 2 + 4, y 1 + 3, z 5 + 3


def ingest_strided(base, offset_elements, dims, strides, value_range):
    d = api.DeviceArray.from_numpy(base)
    ptr = d.ptr + offset_elements * base.dtype.itemsize
    v, used = api.vnrCreateSimpleVolumeFromDevice(ptr, dims, base.dtype, strides=strides, value_range=value_range)
    out = voxels(v, dims)
    mc = api.volume_macrocell(v)["value_range"]
    d.free()
    return out, used, mc


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("variant", ["data", "inside"])
def test_strided_sources_equal_the_dense_copy(dtype, variant):
    box = field(dtype, BOX, seed=1)
    rng = explicit_range(box, variant)
    dense, dense_used = from_device(box, rng)
    want, want_mc = voxels(dense, BOX), api.volume_macrocell(dense)["value_range"]
    assert np.array_equal(want, norm(box, *dense_used))

    def check(out, used, mc, what):
        assert np.array_equal(np.asarray(used, np.float32), np.asarray(dense_used, np.float32)), what
        assert np.array_equal(bits(out), bits(want)), what
        assert np.array_equal(mc, want_mc), what

    # a) ghost layers of different widths per axis and side, filled with values beyond the box's range
    a, b, top, bottom = SPEC[dtype]
    padded = np.empty(PADDED[::-1], dtype)
    padded.reshape(-1)[0::2] = dtype(top)
    padded.reshape(-1)[1::2] = dtype(bottom)
    gx, gy, gz = GHOST
    padded[gz:gz + BOX[2], gy:gy + BOX[1], gx:gx + BOX[0]] = box
    strides = (1, PADDED[0], PADDED[0] * PADDED[1])
    check(*ingest_strided(padded, gx + gy * strides[1] + gz * strides[2], BOX, strides, rng), "ghost layers")
    # b) whole slices contiguous, padding between the slices only
    slab = np.full((BOX[2], BOX[1] * BOX[0] + 7), dtype(top), dtype)
    slab[:, :BOX[1] * BOX[0]] = box.reshape(BOX[2], -1)
    check(*ingest_strided(slab, 0, BOX, (1, BOX[0], BOX[1] * BOX[0] + 7), rng), "padded slices")
    # c) every second voxel along x: the general gather
    wide = np.full((BOX[2], BOX[1], 2 * BOX[0]), dtype(bottom), dtype)
    wide[:, :, ::2] = box
    check(*ingest_strided(wide, 0, BOX, (2, 2 * BOX[0], 2 * BOX[0] * BOX[1]), rng), "sx = 2")
    # d) a dense source one element past a 16-byte boundary: the unaligned dense path
    shifted = np.concatenate([np.full(1, dtype(top), dtype), box.reshape(-1)])
    check(*ingest_strided(shifted, 1, BOX, None, rng), "one element off alignment")
    check(*ingest_strided(shifted, 1, BOX, (1, BOX[0], BOX[0] * BOX[1]), rng), "one element off alignment, dense strides")


# ------------------------------------------------------------------------------------------------ 3. ownership
def test_the_volume_keeps_no_pointer_to_the_source():
    dims = (48, 20, 10)
    a, b = field(np.uint16, dims, seed=2), field(np.uint16, dims, seed=3)
    rng = (500.0, 50000.0)
    d = api.DeviceArray.from_numpy(a)
    v, _ = api.vnrCreateSimpleVolumeFromDevice(d, dims, a.dtype, value_range=rng)
    address = api.lib().vnrAmdSimpleVolumeDeviceData(v.h)
    d.upload(np.full(a.shape, 77, a.dtype))
    d.free()
    assert np.array_equal(voxels(v, dims), norm(a, *rng))
    d = api.DeviceArray.from_numpy(b)
    # (with a producer stream: the library's own, the one vnrAmdMemcpyH2D filled the buffer on)
    same, used = api.vnrSimpleVolumeUpdateFromDevice(v, d, b.dtype, value_range=rng, stream=api.lib().vnrAmdDefaultStream())
    assert same is v and used == rng
    d.upload(np.full(b.shape, 99, b.dtype))
    d.free()
    assert api.lib().vnrAmdSimpleVolumeDeviceData(v.h) == address
    assert np.array_equal(voxels(v, dims), norm(b, *rng))
    assert np.array_equal(api.volume_macrocell(v)["value_range"], api.volume_macrocell(api.vnrCreateSimpleVolume(b, value_range=rng))["value_range"])
    # a one-step volume takes the new step's range; from the data this time
    _, used = api.vnrSimpleVolumeUpdateFromDevice(v, api.DeviceArray.from_numpy(a), a.dtype)
    assert used == data_range(a) and stored_range(v) == data_range(a)
    assert np.array_equal(voxels(v, dims), norm(a, *data_range(a)))


# ------------------------------------------------------------------------------------------------ 4. time steps without scene files
def vidi_scene(files, dims, type_name, volume_extra=None, **source_extra):
    """as tests/test_scene.py builds it"""
    src = [dict({"format": "REGULAR_GRID_RAW_BINARY", "fileName": f, "dimensions": {"x": dims[0], "y": dims[1], "z": dims[2]},
                 "type": type_name}, **source_extra) for f in files]
    return {"dataSource": src,
            "view": {"camera": {"eye": {"x": 10.0, "y": 20.0, "z": -300.0}, "center": {"x": 16.0, "y": 8.0, "z": 4.0},
                                "up": {"x": 0.0, "y": 1.0, "z": 0.0}, "fovy": 42.0},
                     "volume": dict({"transferFunction": {}}, **(volume_extra or {}))}}


def scene_volume(tmp_path, steps, dims, rng):
    files = []
    for i, s in enumerate(steps):
        f = tmp_path / f"t{i}.raw"
        s.astype("<u2").tofile(f)
        files.append(str(f))
    sc = vidi_scene(files, dims, "UNSIGNED_SHORT", {"scalarMappingRangeUnnormalized": {"minimum": rng[0], "maximum": rng[1]}})
    return api.vnrCreateSimpleVolume(sc, "GPU")


def test_time_steps_appended_from_device_equal_a_scene(tmp_path):
    dims = (24, 20, 18)
    rng = (1000.0, 60000.0)
    steps = [field(np.uint16, dims, seed=10 + i) for i in range(3)]
    dev, _ = from_device(steps[0], rng)
    for i in (1, 2):
        index, used = api.vnrSimpleVolumeAppendTimeStepFromDevice(dev, api.DeviceArray.from_numpy(steps[i]), np.uint16, value_range=rng)
        assert index == i and used == rng
        assert np.array_equal(voxels(dev, dims), norm(steps[0], *rng))      # the current step stays current
    scene = scene_volume(tmp_path, steps, dims, rng)
    assert api.vnrSimpleVolumeGetNumberOfTimeSteps(dev) == api.vnrSimpleVolumeGetNumberOfTimeSteps(scene) == 3
    assert stored_range(dev) == stored_range(scene)
    for t in (0, 2, 1, 1, 0):
        for v in (dev, scene):
            api.vnrSimpleVolumeSetCurrentTimeStep(v, t)
        got = voxels(dev, dims)
        assert np.array_equal(bits(got), bits(voxels(scene, dims))) and np.array_equal(got, norm(steps[t], *rng))
        assert np.array_equal(api.volume_macrocell(dev)["value_range"], api.volume_macrocell(scene)["value_range"])
    for v in (dev, scene):
        with pytest.raises(api.VnrAmdError, match="out of range"):
            api.vnrSimpleVolumeSetCurrentTimeStep(v, 3)


def test_ranges_from_the_data_extend_the_volume_range():
    """Append and Update on a volume with several steps extend the data range like a scene's further steps"""
    dims = (24, 20, 18)
    s0, s1, s2 = field(np.int16, dims, seed=20), field(np.int16, dims, seed=21) // 4, field(np.int16, dims, seed=22) // 2
    v, used = from_device(s0)
    assert used == data_range(s0)
    index, used = api.vnrSimpleVolumeAppendTimeStepFromDevice(v, api.DeviceArray.from_numpy(s1), np.int16)
    assert index == 1 and used == data_range(s1)
    assert stored_range(v) == (min(data_range(s0)[0], used[0]), max(data_range(s0)[1], used[1]))
    before = stored_range(v)
    _, used = api.vnrSimpleVolumeUpdateFromDevice(v, api.DeviceArray.from_numpy(s2), np.int16)
    assert used == data_range(s2) and stored_range(v) == (min(before[0], used[0]), max(before[1], used[1]))
    assert np.array_equal(voxels(v, dims), norm(s2, *used))
    api.vnrSimpleVolumeSetCurrentTimeStep(v, 1)
    assert np.array_equal(voxels(v, dims), norm(s1, *data_range(s1)))


# ------------------------------------------------------------------------------------------------ 5. warm start through an update
def test_training_through_an_update_equals_a_time_step_switch(tmp_path, monkeypatch):
    monkeypatch.setenv("VNR_AMD_INIT_SEED", "4711")
    monkeypatch.delenv("VNR_AMD_DETERMINISTIC", raising=False)
    monkeypatch.delenv("VNR_AMD_TRAIN_OVERLAP", raising=False)
    dims = (32, 32, 32)
    rng = (0.0, 65535.0)
    steps = [(syn.analytic_volume(32) * 65535.0).astype(np.uint16), (syn.analytic_volume(32)[::-1, :, ::-1] * 40000.0 + 9000.0).astype(np.uint16)]
    cfg = syn.model_config(n_levels=4, n_features=2, log2_hashmap_size=12, base_resolution=4, n_neurons=16, n_hidden_layers=1)

    def train(sv, switch):
        nv = api.vnrCreateNeuralVolume(cfg, sv)
        api.neural_set_deterministic_training(nv, True)
        api.check(api.lib().vnrAmdNeuralVolumeSetSamplerSeed(nv.h, 99, 7))
        api.vnrNeuralVolumeTrain(nv, 20, True)
        switch(sv)
        api.vnrNeuralVolumeTrain(nv, 20, True)
        assert api.vnrNeuralVolumeGetTrainingStep(nv) == 40
        return api.neural_get_params_fp16(nv).view(np.uint16).copy()

    scene = scene_volume(tmp_path, steps, dims, rng)
    params_a = train(scene, lambda sv: api.vnrSimpleVolumeSetCurrentTimeStep(sv, 1))
    dev, _ = from_device(steps[0], rng)
    params_b = train(dev, lambda sv: api.vnrSimpleVolumeUpdateFromDevice(sv, api.DeviceArray.from_numpy(steps[1]), np.uint16, value_range=rng))
    assert np.isfinite(params_a.view(np.float16).astype(np.float32)).all() and len(np.unique(params_a)) > 100
    assert np.array_equal(params_a, params_b)

    # one mode-4 frame of the updated volume against a fresh host-created volume of step 1
    def frame(sv):
        cam = syn.oblique_camera(dims)
        camera = api.vnrCreateCamera()
        api.vnrCameraSet(camera, cam["from"], cam["at"], cam["up"], cam["fovy"])
        ren = api.vnrCreateRenderer(sv)
        api.vnrRendererSetTransferFunction(ren, tfn())
        api.vnrRendererSetCamera(ren, camera)
        api.vnrRendererSetFramebufferSize(ren, (64, 64))
        api.vnrRendererSetMode(ren, 4)
        api.vnrRender(ren)
        return api.vnrRendererMapFrame(ren).copy()

    got, want = frame(dev), frame(api.vnrCreateSimpleVolume(steps[1], value_range=rng))
    assert float(np.abs(want[..., :3]).max()) > 0.05       # the frame shows the volume
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_name_the_cause_and_leave_the_volume_usable(tmp_path):
    L = api.lib()
    dims = (20, 12, 8)
    a = field(np.uint8, dims, seed=30)
    d = api.DeviceArray.from_numpy(a)
    cd = (C.c_int * 3)(*dims)
    used = (C.c_float * 2)()

    def create(ptr=d.ptr, dims_=cd, vtype=0, strides=None):
        s = (C.c_int64 * 3)(*strides) if strides else None
        h = L.vnrAmdCreateSimpleVolumeFromDevice(C.c_void_p(ptr), dims_, vtype, s, 1.0, 0.0, None, used)
        assert not h
        return api._lib.last_error()

    assert "null device data" in create(ptr=None)
    assert "dimensions must be positive" in create(dims_=(C.c_int * 3)(20, 0, 8))
    assert "dimensions must be positive" in create(dims_=(C.c_int * 3)(-20, 12, 8))
    assert "strides must be positive" in create(strides=(0, 20, 240))
    assert "strides must be positive" in create(strides=(1, -20, 240))
    for vtype, word in ((6, "64-bit"), (7, "64-bit"), (9, "vector"), (10, "vector"), (11, "vector"), (13, "unknown value type")):
        assert word in create(vtype=vtype)
    assert "not aligned" in create(ptr=d.ptr + 1, vtype=2)

    v, _ = api.vnrCreateSimpleVolumeFromDevice(d, dims, a.dtype, value_range=(10.0, 200.0))
    want = norm(a, 10.0, 200.0)
    own = L.vnrAmdSimpleVolumeDeviceData(v.h)

    def refused(fn, match, *args, **kwargs):
        with pytest.raises(api.VnrAmdError, match=match):
            fn(*args, **kwargs)

    for name in ("vnrAmdSimpleVolumeUpdateFromDevice", "vnrAmdSimpleVolumeAppendTimeStepFromDevice"):
        fn = getattr(L, name)
        bad = 1 if name.endswith("UpdateFromDevice") else -1
        assert fn(v.h, None, 0, None, 1.0, 0.0, None, used) == bad and "null device data" in api._lib.last_error()
        assert fn(v.h, C.c_void_p(d.ptr), 6, None, 1.0, 0.0, None, used) == bad and "64-bit" in api._lib.last_error()
        assert fn(v.h, C.c_void_p(d.ptr), 10, None, 1.0, 0.0, None, used) == bad and "vector" in api._lib.last_error()
        assert fn(v.h, C.c_void_p(d.ptr), 0, (C.c_int64 * 3)(1, 0, 240), 1.0, 0.0, None, used) == bad and "strides must be positive" in api._lib.last_error()
        # the volume's own voxels as the source (float data, the same dims), and a source that ends inside them
        assert fn(v.h, C.c_void_p(own), 8, None, 1.0, 0.0, None, used) == bad and "overlaps the volume's own voxel buffer" in api._lib.last_error()
        assert fn(v.h, C.c_void_p(own + 4 * a.size - 16), 0, None, 1.0, 0.0, None, used) == bad and "overlaps" in api._lib.last_error()
    assert api.vnrSimpleVolumeGetNumberOfTimeSteps(v) == 1
    assert L.vnrAmdSimpleVolumeDeviceData(v.h) == own and np.array_equal(voxels(v, dims), want)     # the old voxels

    # volumes that have no resident voxels to replace, and volumes that are not simple volumes
    f = tmp_path / "v.raw"
    a.tofile(f)
    g = tmp_path / "ooc.raw"
    np.random.default_rng(31).uniform(0, 1, (4, 30, 100)).astype(np.float32).tofile(g)
    ooc = api.vnrCreateSimpleVolumeOutOfCore(g, (100, 30, 4), np.float32, (0.0, 1.0), n_concurrent_blocks=2, n_blocks=4)
    sc = vidi_scene([str(f)], dims, "UNSIGNED_BYTE")
    shape_only = api.vnrCreateSimpleVolume(sc, "NOTHING")
    neural = api.vnrCreateNeuralVolume(syn.model_config(n_levels=2, n_features=2, log2_hashmap_size=10, base_resolution=4, n_hidden_layers=1), v)
    for fn in (api.vnrSimpleVolumeUpdateFromDevice, api.vnrSimpleVolumeAppendTimeStepFromDevice):
        refused(fn, "out-of-core", ooc, d, np.uint8, value_range=(0.0, 255.0))
        refused(fn, "shape without data", shape_only, d, np.uint8, value_range=(0.0, 255.0))
        refused(fn, "expecting a simple volume", neural, d, np.uint8, value_range=(0.0, 255.0))

    # ... and everything still works afterwards
    _, rng = api.vnrSimpleVolumeUpdateFromDevice(v, d, np.uint8)
    assert rng == data_range(a) and np.array_equal(voxels(v, dims), norm(a, *rng))
    index, _ = api.vnrSimpleVolumeAppendTimeStepFromDevice(v, d, np.uint8, value_range=(10.0, 200.0))
    assert index == 1
    api.vnrSimpleVolumeSetCurrentTimeStep(v, 1)
    assert np.array_equal(voxels(v, dims), want)
