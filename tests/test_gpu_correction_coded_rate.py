"""Byte budgets in the coded form on the device (include/vnr_amd.h, "byte budgets in the coded form"; correction_rate_coded_kernel
and correction_rate_final_coded_kernel in csrc/correction.hip, vnrAmdNeuralVolumeBuildCorrectionCodedWithinBytes in csrc/capi.cpp)
against the numpy restatement tests/correction_coded_rate_ref.py, against the plain rate call and against the real builds and the
real device encoder.  Sizes are integers and the chosen tolerance is a chain of single double operations: every comparison has
tolerance ZERO.

The setup is the one of tests/test_gpu_correction_rate.py, restated: the trained (40, 24, 20) volume and a (21, 10, 3) one whose
cells have 480 and 150 voxels, and references that are the decoded field perturbed.  The integer references additionally carry
whole groups of placed residuals, which the tolerance 0 (E = 0, a step of 1) gives back as codes exactly: top planes with 1, 9, 10
and 64 lanes set, a group of zeros in a flagged cell, an empty plane between two occupied ones, one code in the last lane of the
short last group of the 150-voxel cell, and (uint32) the largest magnitude the build accepts, 2^31 - 1."""
import functools
import math
import os
import sys

import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correction_coded_rate_ref as ccrr  # noqa: E402
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
LARGEST = 2 ** 31 - 1


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


def group_voxels(dims, cell, group):
    """-> the (z, y, x) index arrays of the voxels of group `group` of cell `cell` = (ix, iy, iz), in lane order (fewer than 64 for a
    short last group): a cell's codes run in lx + cx (ly + cy lz)"""
    x0, y0, z0 = (16 * c for c in cell)
    cx, cy, cz = (min(16, d - o) for d, o in zip(dims, (x0, y0, z0)))
    li = np.arange(64 * group, min(64 * group + 64, cx * cy * cz))
    return z0 + li // (cx * cy), y0 + li // cx % cy, x0 + li % cx


def lanes(**codes):
    """64 codes of a group: lanes(a=(code, first lane, count), ...), the rest 0"""
    q = np.zeros(64, np.int64)
    for code, first, count in codes.values():
        q[first:first + count] = code
    return q


def placed(dtype, dims):
    """[(cell, group, 64 codes)] of the groups whose residuals are placed; integer types only"""
    if np.dtype(dtype).kind == "f":
        return []
    if dims == TAIL_DIMS:                                    # cell (1, 0, 0) has 5 * 10 * 3 = 150 voxels: groups of 64, 64 and 22
        return [((1, 0, 0), 2, lanes(last=(1, 21, 1)))]
    alternating = np.where(np.arange(64) % 2, -1, 1)
    out = [((0, 0, 0), 8, lanes(top=(4, 3, 1), low=(-1, 10, 6))),                   # the top plane has 1 lane
           ((0, 0, 0), 9, lanes(top=(2, 0, 9), low=(1, 20, 10))),                   # 9: the longest list; below it 10: the shortest dense plane
           ((0, 0, 0), 10, lanes(top=(-2, 0, 10))),                                 # 10
           ((0, 0, 0), 11, alternating),                                            # 64
           ((0, 0, 0), 12, lanes()),                                                # a group of zeros in a flagged cell
           ((0, 0, 0), 13, lanes(both=(5, 0, 3)))]                                  # planes 2 and 0 occupied, plane 1 empty
    if np.dtype(dtype) == np.uint32:
        out.append(((0, 0, 0), 14, lanes(largest=(LARGEST, 7, 1))))
    return out


def perturbed(dec, dtype, eps, dims):
    """the decoded field perturbed: codes of a few -3 .. 3 among zeros where x < 16 (none at all from z = 16 on: clean cells),
    thousands where 16 <= x < 32, millions (a 16-bit type: hundreds) beyond; eps == 0: +0.0 in the slice z = 0 from x = 16 on; then
    the placed groups: ref = dec + code there (towards the inside of the type's range for the largest magnitude)"""
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
        return ref
    info = np.iinfo(dtype)
    wanted = dec.astype(np.int64) + q * (2 * int(eps) + 1)
    for cell, group, codes in placed(dtype, dims):
        at = group_voxels(dims, cell, group)
        d = dec[at].astype(np.int64)
        codes = codes[:len(d)]
        codes = np.where((d + codes > info.max) | (d + codes < info.min), -codes, codes)      # (a sign changes no plane)
        wanted[at] = d + codes
        assert (wanted[at] >= info.min).all() and (wanted[at] <= info.max).all()               # the codes come back exactly
    return np.clip(wanted, info.min, info.max).astype(dtype)


@functools.lru_cache(maxsize=None)
def reference(dtype, eps, dims):
    ref = perturbed(decoded(dtype, dims), dtype, eps, dims)
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
    """correction_coded_rate_ref.rates of `tol`; computed once per list"""
    return ccrr.rates(decoded(dtype, dims), reference(dtype, eps, dims), list(tol))


def device_reference(dtype, eps, dims, kind):
    """-> (device array, its host copy, address of the first voxel, strides): reference() in an array of sentinels"""
    n, offset, strides = layout(kind, dims)
    host = np.full(n, sentinel(dtype), dtype)
    box_view(host, offset, strides, dims)[...] = reference(dtype, eps, dims)
    d = api.DeviceArray.from_numpy(host)
    return d, host, d.ptr + offset * host.dtype.itemsize, strides


def device_rates(dtype, eps, dims, tol, kind="dense", check_plain=False):
    d, host, ptr, strides = device_reference(dtype, eps, dims, kind)
    try:
        got = api.vnrNeuralVolumeCorrectionRates(trained(dims)[1], ptr, dtype, tol, strides, RANGES[dtype], coded=True)
        assert np.array_equal(d.numpy().view(np.uint8), host.view(np.uint8)), "the coded rate call wrote into the reference array"
        if check_plain:                                     # the `rate` part is the plain call's entry
            plain = api.vnrNeuralVolumeCorrectionRates(trained(dims)[1], ptr, dtype, tol, strides, RANGES[dtype])
            assert [{k: v for k, v in g.items() if k not in ccrr.FIELDS} for g in got] == plain
            assert all(set(g) - set(p) == set(ccrr.FIELDS) for g, p in zip(got, plain))
        return got
    finally:
        d.free()


def top_plane_counts(m):
    """m [groups, 64] -> the lanes set in the top plane of every group (0 for a group of zeros)"""
    out = []
    for g in m:
        mbits = int(g.max()).bit_length()
        out.append(int(((g >> np.uint64(mbits - 1)) & np.uint64(1)).sum()) if mbits else 0)
    return out


def assert_the_placed_codes_are_met(dtype, eps, dims, tol, want):
    """from the numpy side: what the comparison at tolerance 0 covers"""
    assert 0.0 in tol and not want[tol.index(0.0)]["refused"]
    dec, ref = decoded(dtype, dims), reference(dtype, eps, dims)
    cells = {cell: m for cell, m, _ in ccrr.flagged_cells(dec, ref, 0.0)}
    if dims == TAIL_DIMS:
        m = cells[1]
        assert m.shape == (3, 64) and m[:2].any() and np.flatnonzero(m[2]).tolist() == [21] and m[2, 21] == 1
        assert int(ccrr.group_bits(m[2:], True)[0]) == 7 + 5 + 6 + 1
        return
    m = cells[0]
    assert top_plane_counts(m[8:14]) == [1, 9, 10, 64, 0, 3]
    assert int(((m[9] >> np.uint64(0)) & np.uint64(1)).sum()) == 10                            # 9 and 10 side by side: 59 and 65 bits
    assert [int(b) for b in ccrr.group_bits(m[8:14], True)] == [7 + 11 + 5 + 41 + 7, 7 + 59 + 65 + 19, 7 + 65 + 5 + 10, 7 + 65 + 64, 7, 7 + 23 + 5 + 23 + 3]
    if np.dtype(dtype) == np.uint32:
        assert int(m[14].max()) == LARGEST == int(m.max()) and int(ccrr.group_bits(m[14:15], True)[0]) == 7 + 31 * 11 + 1


# ------------------------------------------------------------------------------------------------ 1. against numpy
@pytest.mark.parametrize("dims", ALL_DIMS, ids=DIMS_IDS)
@pytest.mark.parametrize("dtype,eps", TYPES, ids=TYPE_IDS)
def test_coded_rates_equal_numpy(dtype, eps, dims, monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    tol = tolerances(dtype, eps, dims)
    want = expected(dtype, eps, dims, tol)
    is_float = np.dtype(dtype).kind == "f"
    if not is_float:
        assert_the_placed_codes_are_met(dtype, eps, dims, tol, want)
    for kind in ("dense", "ghost", "gather"):
        got = device_rates(dtype, eps, dims, tol, kind, check_plain=True)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g == w, (kind, k, tol[k], g, w)
    assert sum(w["refused"] for w in want) == (1 if is_float else 0)
    assert all(w[k] == 0 for w in want if w["refused"] for k in ccrr.FIELDS)
    assert {w["kind"] for w in want} == ({1, 2} if is_float else {0})
    clean = [w for w in want if not w["refused"] and w["n_flagged"] == 0]
    assert clean and all((w["coded_stream_words"], w["coded_payload_bytes"], w["coded_serialized_bytes"]) == (0, 0, 104) for w in clean)
    assert max(w["coded_stream_words"] for w in want) > 0


# ------------------------------------------------------------------------------------------------ 2. chunks
@pytest.mark.parametrize("dims", ALL_DIMS, ids=DIMS_IDS)
@pytest.mark.parametrize("dtype,eps", TYPES, ids=TYPE_IDS)
def test_coded_rates_do_not_depend_on_the_chunk_size(dtype, eps, dims, monkeypatch):
    tol = tolerances(dtype, eps, dims)
    want = expected(dtype, eps, dims, tol)
    for chunk in (64, 1000, 5000):                            # one group a chunk; chunks that end inside cells
        monkeypatch.setenv("VNR_AMD_DECODE_CHUNK", str(chunk))
        assert device_rates(dtype, eps, dims, tol, "ghost") == want, chunk


# ------------------------------------------------------------------------------------------------ 3. the real builds and the real encoder
@pytest.mark.parametrize("dims", ALL_DIMS, ids=DIMS_IDS)
@pytest.mark.parametrize("dtype,eps", TYPES, ids=TYPE_IDS)
def test_coded_rates_equal_what_the_encoder_writes(dtype, eps, dims, monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    nv = trained(dims)[1]
    top = top_error(dtype, eps, dims)
    tol = [math.ldexp(top, -2), math.ldexp(top, -8), math.ldexp(top, -14), 0.0]      # three of the ladder, and E = 0 / verbatim
    d, _, ptr, strides = device_reference(dtype, eps, dims, "ghost")
    try:
        got = api.vnrNeuralVolumeCorrectionRates(nv, ptr, dtype, tol, strides, RANGES[dtype], coded=True)
        for e, r in zip(tol, got):
            c = api.vnrNeuralVolumeBuildCorrection(nv, ptr, dtype, e, strides, RANGES[dtype])
            direct = api.vnrNeuralVolumeBuildCorrectionPacked(nv, ptr, dtype, e, strides, RANGES[dtype])
            coded = c.to_coded_bytes()                        # (encoded on the device from the resident fixed-width codes)
            assert not r["refused"] and r["eps"] == e
            assert r["coded_serialized_bytes"] == len(coded) == direct.to_coded_device(), (e, r)          # (from the resident planes: the size alone)
            assert r["coded_payload_bytes"] == len(coded) - 104 - 8 * r["n_flagged"] and r["n_flagged"] == c.info()["n_flagged"]
            assert r["coded_stream_words"] * 8 == r["coded_payload_bytes"] - (4 * r["n_flagged"] + 7) // 8 * 8
            c.release(); direct.release()
        assert got[-1]["n_flagged"] > 0
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------ 4. the coded build within a budget
@pytest.mark.parametrize("dims", ALL_DIMS, ids=DIMS_IDS)
@pytest.mark.parametrize("dtype,eps", TYPES, ids=TYPE_IDS)
def test_coded_build_within_bytes_chooses_what_numpy_chooses(dtype, eps, dims, monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    nv = trained(dims)[1]
    dec, ref = decoded(dtype, dims), reference(dtype, eps, dims)
    eps_hi = top_error(dtype, eps, dims)
    ladder = tuple(math.ldexp(eps_hi, -j) for j in range(16))
    sizes = [r["coded_serialized_bytes"] for r in expected(dtype, eps, dims, ladder)]
    a = next(j for j in range(3, 15) if sizes[j] < sizes[j + 1] and max(sizes[:j + 1]) == sizes[j])      # two ladder steps of different sizes
    max_bytes = (sizes[a] + sizes[a + 1]) // 2                                        # midway: t_0 .. t_a fit, t_(a+1) does not
    assert sizes[a] <= max_bytes < sizes[a + 1]
    rounds = []

    def size_of(points):
        s = [None if r["refused"] else r["coded_serialized_bytes"] for r in ccrr.rates(dec, ref, points)]
        rounds.append([x is not None and x <= max_bytes for x in s])
        return s

    want = crr.budget_search(size_of, max_bytes, eps_hi, 2)
    # the ladder and at least one refinement round each hold probes that fit and probes that do not
    assert len(rounds) == 3 and any(rounds[0]) and not all(rounds[0]) and any(any(r) and not all(r) for r in rounds[1:]), rounds
    d, _, ptr, strides = device_reference(dtype, eps, dims, "ghost")
    try:
        corr, report = api.vnrNeuralVolumeBuildCorrectionWithinBytes(nv, ptr, dtype, max_bytes, eps_hi, "coded", 2, strides, RANGES[dtype])
        assert report["eps"].hex() == want["eps"].hex() and report["eps_tighter"].hex() == want["eps_tighter"].hex(), (report, want)
        assert report == want and report["rate_passes"] == 3
        assert corr.residency()["form"] == "packed" and corr.residency()["on_device"]
        blob = corr.to_coded_bytes()
        assert report["bytes"] == len(blob) <= max_bytes < report["bytes_tighter"]
        assert corr.to_coded_device() == len(blob)
        direct = api.vnrNeuralVolumeBuildCorrectionPacked(nv, ptr, dtype, report["eps"], strides, RANGES[dtype])
        assert blob == direct.to_coded_bytes() and corr.to_packed_bytes() == direct.to_packed_bytes()
        assert corr.residency()["form"] == "packed"
        info = corr.info()
        assert info["eps"] == report["eps"] and info["n_flagged"] > 0
        corr.release(); direct.release()

        # a budget below the size at eps_hi: refused with the numbers named, nothing returned
        assert sizes[0] == 104
        with pytest.raises(api.VnrAmdError) as refused:
            api.vnrNeuralVolumeBuildCorrectionWithinBytes(nv, ptr, dtype, 103, eps_hi, "coded", 2, strides, RANGES[dtype])
        msg = str(refused.value)
        assert "max_bytes 103" in msg and ("eps_hi %.17g" % eps_hi) in msg and "104 bytes" in msg, msg
        # a huge budget: the last step of the ladder after one pass
        corr, report = api.vnrNeuralVolumeBuildCorrectionWithinBytes(nv, ptr, dtype, 1 << 40, eps_hi, "coded", 2, strides, RANGES[dtype])
        assert report["eps"] == math.ldexp(eps_hi, -15) and report["rate_passes"] == 1
        assert math.isnan(report["eps_tighter"]) and report["bytes_tighter"] == 0 and report["bytes"] == len(corr.to_coded_bytes()) == sizes[15]
        corr.release()
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------ 5. no side effects
def test_a_coded_rate_call_changes_neither_the_parameters_nor_a_later_rate_call_or_build(monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    dtype, eps = TYPES[0]
    nv = trained(DIMS)[1]
    tol = tolerances(dtype, eps, DIMS)
    d, host, ptr, strides = device_reference(dtype, eps, DIMS, "ghost")
    try:
        build_eps = math.ldexp(top_error(dtype, eps, DIMS), -9)
        before = api.vnrNeuralVolumeBuildCorrection(nv, ptr, dtype, build_eps, strides, RANGES[dtype])
        plain_before = api.vnrNeuralVolumeCorrectionRates(nv, ptr, dtype, tol, strides, RANGES[dtype])
        params = api.neural_get_params_fp16(nv).copy()
        api.vnrNeuralVolumeCorrectionRates(nv, ptr, dtype, tol, strides, RANGES[dtype], coded=True)
        assert np.array_equal(d.numpy().view(np.uint8), host.view(np.uint8))          # ghost layers included
        assert np.array_equal(api.neural_get_params_fp16(nv), params)
        assert api.vnrNeuralVolumeCorrectionRates(nv, ptr, dtype, tol, strides, RANGES[dtype]) == plain_before
        assert all(set(r) == {"eps", "kind", "refused"} | set(crr.FIELDS) for r in plain_before)
        after = api.vnrNeuralVolumeBuildCorrection(nv, ptr, dtype, build_eps, strides, RANGES[dtype])
        assert after.to_bytes() == before.to_bytes() and after.to_packed_bytes() == before.to_packed_bytes() and after.to_coded_bytes() == before.to_coded_bytes()
        assert after.info() == before.info() and before.info()["n_flagged"] > 0
        before.release(); after.release()
    finally:
        d.free()
