"""Corrections to a byte budget on the device (include/vnr_amd.h, "corrections to a byte budget"; correction_rate_kernel and its
neighbours in csrc/correction.hip, the search of csrc/correction_budget.cpp) against the numpy restatement
tests/correction_rate_ref.py and against the real build.  Counts and sizes are integers and the chosen tolerance is a chain of
single double operations: every comparison has tolerance ZERO.

The setup is the one of tests/test_gpu_correction_roi.py, restated: the trained (40, 24, 20) volume (ragged upper faces, clean cells,
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
import correction_rate_ref as crr  # noqa: E402

pytestmark = pytest.mark.gpu

DIMS = (40, 24, 20)
TAIL_DIMS = (21, 10, 3)
ALL_DIMS = [DIMS, TAIL_DIMS]
DIMS_IDS = ["40x24x20", "21x10x3"]
# (dtype, the eps the perturbation is scaled by): kind 1, kind 0 of a narrow and of a wide type, 64-bit values
TYPES = [(np.float32, 1e-3), (np.int16, 2), (np.uint32, 1), (np.float64, 0)]
TYPE_IDS = [t.__name__ for t, _ in TYPES]
RANGES = {np.int16: (-30000.0, 30000.0), np.uint32: (0.0, 4.0e9), np.float32: (-3.5, 12.25), np.float64: (-1.0e3, 2.5e3)}
FORMS = {"fixed": "serialized_bytes", "packed": "packed_serialized_bytes"}


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
def tolerances(dtype, eps, dims):
    """33 tolerances, so batches of 16, 16 and 1: the ladder top * 2^-j, j = 0 .. 15, 0 (twice), a duplicate, one at which the float
    types' build is refused (a code of 2^32), points between the ladder's steps; in no order"""
    top = top_error(dtype, eps, dims)
    ladder = [math.ldexp(top, -j) for j in range(16)]
    between = [1.5 * ladder[j] for j in (14, 2, 9, 0, 7, 11, 4, 13, 1, 6, 3, 10)]
    tol = ladder + [0.0, math.ldexp(top, -33), ladder[5], 0.0, ladder[5]] + between
    order = np.random.default_rng(33).permutation(len(tol))
    tol = tuple(tol[i] for i in order)
    assert len(tol) == 33 and len(set(tol)) == 30
    return tol


@functools.lru_cache(maxsize=None)
def expected(dtype, eps, dims, tol):
    """correction_rate_ref.rates of `tol`; computed once per list"""
    return crr.rates(decoded(dtype, dims), reference(dtype, eps, dims), list(tol))


def device_reference(dtype, eps, dims, kind):
    """-> (device array, its host copy, address of the first voxel, strides): reference() in an array of sentinels"""
    n, offset, strides = layout(kind, dims)
    host = np.full(n, sentinel(dtype), dtype)
    box_view(host, offset, strides, dims)[...] = reference(dtype, eps, dims)
    d = api.DeviceArray.from_numpy(host)
    return d, host, d.ptr + offset * host.dtype.itemsize, strides


def device_rates(dtype, eps, dims, tol, kind="dense"):
    d, host, ptr, strides = device_reference(dtype, eps, dims, kind)
    try:
        got = api.vnrNeuralVolumeCorrectionRates(trained(dims)[1], ptr, dtype, tol, strides, RANGES[dtype])
        assert np.array_equal(d.numpy().view(np.uint8), host.view(np.uint8)), "the rate call wrote into the reference array"
        return got
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------ 1. against numpy
@pytest.mark.parametrize("dims", ALL_DIMS, ids=DIMS_IDS)
@pytest.mark.parametrize("dtype,eps", TYPES, ids=TYPE_IDS)
def test_rates_equal_numpy(dtype, eps, dims, monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    tol = tolerances(dtype, eps, dims)
    want = expected(dtype, eps, dims, tol)
    for kind in ("dense", "ghost", "gather"):
        got = device_rates(dtype, eps, dims, tol, kind)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g == w, (kind, k, tol[k], g, w)
    is_float = np.dtype(dtype).kind == "f"
    assert sum(w["refused"] for w in want) == (1 if is_float else 0)
    assert {w["kind"] for w in want} == ({1, 2} if is_float else {0})
    flagged = [w["n_flagged"] for w in want if not w["refused"]]
    assert min(flagged) == 0 and max(flagged) > 0


# ------------------------------------------------------------------------------------------------ 2. chunks
@pytest.mark.parametrize("dims", ALL_DIMS, ids=DIMS_IDS)
@pytest.mark.parametrize("dtype,eps", TYPES, ids=TYPE_IDS)
def test_rates_do_not_depend_on_the_chunk_size(dtype, eps, dims, monkeypatch):
    tol = tolerances(dtype, eps, dims)
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    want = device_rates(dtype, eps, dims, tol, "ghost")
    assert want == expected(dtype, eps, dims, tol)
    for chunk in (64, 1000, 5000):                            # one group a chunk; chunks that end inside cells
        monkeypatch.setenv("VNR_AMD_DECODE_CHUNK", str(chunk))
        assert device_rates(dtype, eps, dims, tol, "ghost") == want, chunk


# ------------------------------------------------------------------------------------------------ 3. the real build
@pytest.mark.parametrize("dims", ALL_DIMS, ids=DIMS_IDS)
@pytest.mark.parametrize("dtype,eps", TYPES, ids=TYPE_IDS)
def test_rates_equal_what_the_build_reports(dtype, eps, dims, monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    top = top_error(dtype, eps, dims)
    tol = [math.ldexp(top, -2), math.ldexp(top, -8), math.ldexp(top, -14), 0.0]      # three of the ladder, and E = 0 / verbatim
    d, _, ptr, strides = device_reference(dtype, eps, dims, "ghost")
    try:
        got = api.vnrNeuralVolumeCorrectionRates(trained(dims)[1], ptr, dtype, tol, strides, RANGES[dtype])
        for e, r in zip(tol, got):
            c = api.vnrNeuralVolumeBuildCorrection(trained(dims)[1], ptr, dtype, e, strides, RANGES[dtype])
            info = c.info()
            assert not r["refused"] and r["eps"] == e and r["kind"] == info["kind"]
            assert (r["serialized_bytes"], r["packed_serialized_bytes"]) == (len(c.to_bytes()), len(c.to_packed_bytes())), (e, r)
            assert (r["n_flagged"], r["n_voxels_flagged"], r["payload_bytes"]) == (info["n_flagged"], info["n_voxels_flagged"], info["payload_bytes"]), (e, r, info)
            assert r["serialized_bytes"] == info["serialized_bytes"] and r["n_flagged"] > 0
            c.release()
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------ 4. no side effects
def test_a_rate_call_changes_neither_the_reference_nor_a_later_build(monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    dtype, eps = TYPES[0]
    nv = trained(DIMS)[1]
    tol = tolerances(dtype, eps, DIMS)
    d, host, ptr, strides = device_reference(dtype, eps, DIMS, "ghost")
    try:
        build_eps = math.ldexp(top_error(dtype, eps, DIMS), -9)
        before = api.vnrNeuralVolumeBuildCorrection(nv, ptr, dtype, build_eps, strides, RANGES[dtype])
        params = api.neural_get_params_fp16(nv).copy()
        api.vnrNeuralVolumeCorrectionRates(nv, ptr, dtype, tol, strides, RANGES[dtype])
        assert np.array_equal(d.numpy().view(np.uint8), host.view(np.uint8))          # ghost layers included
        assert np.array_equal(api.neural_get_params_fp16(nv), params)
        after = api.vnrNeuralVolumeBuildCorrection(nv, ptr, dtype, build_eps, strides, RANGES[dtype])
        assert after.to_bytes() == before.to_bytes() and after.to_packed_bytes() == before.to_packed_bytes()
        assert after.info() == before.info() and before.info()["n_flagged"] > 0
        before.release(); after.release()
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------ 5. the build within a budget
def serialised(corr, form):
    return corr.to_packed_bytes() if form == "packed" else corr.to_bytes()


@pytest.mark.parametrize("dims", ALL_DIMS, ids=DIMS_IDS)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype,eps", TYPES, ids=TYPE_IDS)
def test_build_within_bytes_chooses_what_numpy_chooses(dtype, eps, form, dims, monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    nv = trained(dims)[1]
    dec, ref = decoded(dtype, dims), reference(dtype, eps, dims)
    eps_hi = top_error(dtype, eps, dims)
    ladder = tuple(math.ldexp(eps_hi, -j) for j in range(16))
    sizes = [r[FORMS[form]] for r in expected(dtype, eps, dims, ladder)]
    a = next(j for j in range(3, 15) if sizes[j] < sizes[j + 1])                      # two ladder steps of different sizes
    max_bytes = (sizes[a] + sizes[a + 1]) // 2                                        # midway: t_a fits, t_(a+1) does not
    assert sizes[a] <= max_bytes < sizes[a + 1]

    def size_of(points):
        return [None if r["refused"] else r[FORMS[form]] for r in crr.rates(dec, ref, points)]

    want = crr.budget_search(size_of, max_bytes, eps_hi, 2)
    d, _, ptr, strides = device_reference(dtype, eps, dims, "ghost")
    out = None
    try:
        corr, report = api.vnrNeuralVolumeBuildCorrectionWithinBytes(nv, ptr, dtype, max_bytes, eps_hi, form, 2, strides, RANGES[dtype])
        assert report["eps"].hex() == want["eps"].hex() and report["eps_tighter"].hex() == want["eps_tighter"].hex(), (report, want)
        assert report == want and report["rate_passes"] == 3
        blob = serialised(corr, form)
        assert report["bytes"] == len(blob) <= max_bytes < report["bytes_tighter"]
        assert math.ldexp(eps_hi, -a - 1) <= report["eps_tighter"] < report["eps"] <= math.ldexp(eps_hi, -a)
        plain = api.vnrNeuralVolumeBuildCorrection(nv, ptr, dtype, report["eps"], strides, RANGES[dtype])
        assert corr.to_bytes() == plain.to_bytes() and corr.to_packed_bytes() == plain.to_packed_bytes()
        info = corr.info()
        assert info["eps"] == report["eps"] and info["n_flagged"] > 0
        out = api.DeviceArray((dims[0] * dims[1] * dims[2],), dtype)
        api.vnrNeuralVolumeDecodeToDeviceCorrected(nv, corr, out)
        worst = float(np.abs(out.numpy().reshape(dims[::-1]).astype(np.float64) - ref.astype(np.float64)).max())
        assert worst <= info["max_abs_after"] < top_error(dtype, eps, dims), (worst, info)
        corr.release(); plain.release()

        # a budget below the size at eps_hi: refused with the numbers named, nothing returned
        assert sizes[0] == 104
        with pytest.raises(api.VnrAmdError) as refused:
            api.vnrNeuralVolumeBuildCorrectionWithinBytes(nv, ptr, dtype, 103, eps_hi, form, 2, strides, RANGES[dtype])
        msg = str(refused.value)
        assert "max_bytes 103" in msg and ("eps_hi %.17g" % eps_hi) in msg and "104 bytes" in msg, msg
        # a huge budget: the last step of the ladder after one pass
        corr, report = api.vnrNeuralVolumeBuildCorrectionWithinBytes(nv, ptr, dtype, 1 << 40, eps_hi, form, 2, strides, RANGES[dtype])
        assert report["eps"] == math.ldexp(eps_hi, -15) and report["rate_passes"] == 1
        assert math.isnan(report["eps_tighter"]) and report["bytes_tighter"] == 0 and report["bytes"] == len(serialised(corr, form)) == sizes[15]
        corr.release()
    finally:
        d.free()
        if out is not None:
            out.free()
