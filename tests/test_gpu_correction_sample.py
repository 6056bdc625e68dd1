"""Random access to the corrected field on the device (include/vnr_amd.h, "random access to the corrected field";
correction_voxels_check_kernel, correction_gather_kernel and correction_sample_kernel, csrc/correction.hip) against the numpy
restatements tests/error_bound_ref.py and tests/correction_sample_ref.py.  Every comparison of stored values has tolerance ZERO and
compares bytes.

The setup is the one of tests/test_gpu_correction_roi.py, imported: the trained (40, 24, 20) volume and the (21, 10, 3) one (cells of
480 and 150 voxels, cx = 5: rows that wrap a group), the perturbed references with clean cells where x < 16 and z >= 16, corrections
read from packed bytes with the form set before their first use.  The sampler's restatement is fed vnrAmdNeuralVolumeInference's own
values at the same points."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correction_coded_ref as ccr  # noqa: E402
import correction_sample_ref as csr  # noqa: E402
import error_bound_ref as ebr  # noqa: E402
import test_gpu_correction_roi as roi  # noqa: E402

pytestmark = pytest.mark.gpu

DIMS, TAIL_DIMS, FORMS, RANGES = roi.DIMS, roi.TAIL_DIMS, roi.FORMS, roi.RANGES
BOTH_DIMS = [DIMS, TAIL_DIMS]
DIM_IDS = ["40x24x20", "21x10x3"]
GATHER_TYPES, GATHER_IDS = roi.APPLY_TYPES, roi.TYPE_IDS
SAMPLE_TYPES = roi.APPLY_TYPES[:3] + [(np.float64, 1e-3)]       # kinds 0 and 1; the verbatim one is refused
SAMPLE_IDS = [f"{t.__name__}-{e}" for t, e in SAMPLE_TYPES]
same_bytes, sentinel = roi.same_bytes, roi.sentinel


@functools.lru_cache(maxsize=None)
def voxel_list(dims):
    """every voxel of the grid in a seeded permutation plus 100 duplicates, (n, 3) int32; read only"""
    z, y, x = np.meshgrid(*(np.arange(d) for d in dims[::-1]), indexing="ij")
    v = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.int32)
    rng = np.random.default_rng(dims[0])
    v = np.concatenate([v[rng.permutation(len(v))], v[rng.integers(0, len(v), 100)]])
    v.setflags(write=False)
    return v


def at(a, voxels):
    return a[voxels[:, 2], voxels[:, 1], voxels[:, 0]]


def gather(corr, dims, voxels, nv=None, verify=False):
    """-> (status, message, the destination of n + 3 elements after the call, the same as it was before): sentinels all around"""
    dtype = {v: k for k, v in api.VALUE_TYPES.items()}[corr.info()["value_type"]]
    voxels = np.ascontiguousarray(voxels, np.int32).reshape(-1, 3)
    before = np.full(len(voxels) + 3, sentinel(dtype), dtype)
    d_v, d_o = api.DeviceArray.from_numpy(voxels), api.DeviceArray.from_numpy(before)
    try:
        st = api.lib().vnrAmdNeuralVolumeGatherVoxelsCorrected((nv or roi.trained(dims)[1]).h, corr.h, len(voxels), C.c_void_p(d_v.ptr), C.c_void_p(d_o.ptr), None,
                                                               int(verify))
        return st, api._lib.last_error(), d_o.numpy(), before
    finally:
        d_v.free(); d_o.free()


def gathered(corr, dims, voxels):
    st, msg, got, before = gather(corr, dims, voxels)
    assert st == 0, msg
    assert same_bytes(got[len(voxels):], before[len(voxels):])            # nothing beyond the n elements
    return got[:len(voxels)]


def sample(corr, dims, coords, nv=None, verify=False):
    """-> (status, message, the n + 3 values after the call, the same before)"""
    coords = np.ascontiguousarray(coords, np.float32).reshape(-1, 3)
    before = np.full(len(coords) + 3, sentinel(np.float32), np.float32)
    d_c, d_o = api.DeviceArray.from_numpy(coords), api.DeviceArray.from_numpy(before)
    try:
        st = api.lib().vnrAmdNeuralVolumeSampleCorrected((nv or roi.trained(dims)[1]).h, corr.h, len(coords), C.c_void_p(d_c.ptr), C.c_void_p(d_o.ptr), None, int(verify))
        return st, api._lib.last_error(), d_o.numpy(), before
    finally:
        d_c.free(); d_o.free()


def sampled(corr, dims, coords):
    st, msg, got, before = sample(corr, dims, coords)
    assert st == 0, msg
    assert same_bytes(got[len(coords):], before[len(coords):])
    return got[:len(coords)]


@functools.lru_cache(maxsize=None)
def points(dims):
    """(a) all voxel centres by the decode's arithmetic, (b) 4096 seeded uniform points, (c) the edge set -> (coords, the network's
    values there); read only"""
    coords = np.concatenate([csr.voxel_centres(dims), csr.uniform_points(4096, 11), csr.edge_points(dims)])
    v = api.neural_inference(roi.trained(dims)[1], coords)
    coords.setflags(write=False); v.setflags(write=False)
    return coords, v


# ------------------------------------------------------------------------------------------------ 1. gather equals decode
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dims", BOTH_DIMS, ids=DIM_IDS)
@pytest.mark.parametrize("dtype,eps", GATHER_TYPES, ids=GATHER_IDS)
def test_gather_equals_the_corrected_decode(dtype, eps, dims, form):
    voxels = voxel_list(dims)
    assert len(voxels) == dims[0] * dims[1] * dims[2] + 100 and (dims != DIMS or len(voxels) == 19300)
    corrected = roi.expected(dtype, eps, dims)[2]                           # error_bound_ref.apply(decoded, blob)
    got = gathered(roi.correction(dtype, eps, dims, form), dims, voxels)
    assert same_bytes(got, at(corrected, voxels))
    assert not same_bytes(got, at(roi.decoded(dtype, dims), voxels))
    # and the restatement of the route says the same
    assert same_bytes(csr.gather(csr.Source(roi.expected(dtype, eps, dims)[0], form), at(roi.decoded(dtype, dims), voxels), voxels), got)
    assert roi.correction(dtype, eps, dims, form).residency()["form"] == form


# ------------------------------------------------------------------------------------------------ 2. sizes and chunks
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype,eps", GATHER_TYPES, ids=GATHER_IDS)
def test_gather_sizes_around_a_wave_and_chunks_of_64(dtype, eps, form, monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    corr, corrected = roi.correction(dtype, eps, DIMS, form), roi.expected(dtype, eps, DIMS)[2]
    voxels = voxel_list(DIMS)
    for n in (1, 63, 64, 65):
        assert same_bytes(gathered(corr, DIMS, voxels[5:5 + n]), at(corrected, voxels[5:5 + n])), n
    monkeypatch.setenv("VNR_AMD_DECODE_CHUNK", "64")
    assert same_bytes(gathered(corr, DIMS, voxels), at(corrected, voxels))
    assert same_bytes(gathered(roi.correction(dtype, eps, TAIL_DIMS, form), TAIL_DIMS, voxel_list(TAIL_DIMS)), at(roi.expected(dtype, eps, TAIL_DIMS)[2], voxel_list(TAIL_DIMS)))
    monkeypatch.setenv("VNR_AMD_DECODE_CHUNK", "sixty-four")
    st, msg, got, before = gather(corr, DIMS, voxels[:8])
    assert st != 0 and "VNR_AMD_DECODE_CHUNK" in msg and same_bytes(got, before)
    st, msg, got, before = gather(corr, DIMS, voxels[:0])                    # the variable is read before an empty list returns
    assert st != 0 and "VNR_AMD_DECODE_CHUNK" in msg
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK")
    st, msg, got, before = gather(corr, DIMS, voxels[:0])
    assert st == 0 and same_bytes(got, before), msg


# ------------------------------------------------------------------------------------------------ 3. the guarantee
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype,eps", GATHER_TYPES, ids=GATHER_IDS)
def test_gather_keeps_the_guarantee(dtype, eps, form):
    voxels = voxel_list(DIMS)
    got = gathered(roi.correction(dtype, eps, DIMS, form), DIMS, voxels)
    ref, dec = at(roi.reference(dtype, eps, DIMS), voxels), at(roi.decoded(dtype, DIMS), voxels)
    if np.dtype(dtype).kind != "f":
        assert (np.abs(got.astype(np.int64) - ref.astype(np.int64)) <= int(np.floor(eps))).all()
    elif eps > 0:
        assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= ebr.float_bound(got, ref, dec, eps)).all()
    else:
        assert same_bytes(got, ref)                                          # verbatim: a cell is flagged or equal already


# ------------------------------------------------------------------------------------------------ 4. out of range
@pytest.mark.parametrize("form", FORMS)
def test_gather_refuses_a_voxel_outside_the_grid_by_its_lowest_position(form):
    dtype, eps = GATHER_TYPES[1]
    corr = roi.correction(dtype, eps, DIMS, form)
    base = np.array(voxel_list(DIMS)[:300])
    for places in ({170: (DIMS[0], 3, 3)}, {64: (5, -1, 2)}, {299: (1, 2, DIMS[2])}, {131: (2, DIMS[1], 0), 77: (-1, 0, 0)}, {0: (-2 ** 31, 0, 0)},
                   {200: (0, 0, 2 ** 31 - 1), 201: (0, 0, -1)}):
        voxels = base.copy()
        for j, v in places.items():
            voxels[j] = v
        st, msg, got, before = gather(corr, DIMS, voxels)
        j = min(places)
        assert st != 0 and f"voxel {j} of the list ({places[j][0]}, {places[j][1]}, {places[j][2]}) is outside the grid 40 x 24 x 20" in msg, msg
        assert same_bytes(got, before)
    assert same_bytes(gathered(corr, DIMS, base), at(roi.expected(dtype, eps, DIMS)[2], base))


# ------------------------------------------------------------------------------------------------ 5. no flagged cell
@pytest.mark.parametrize("dtype,eps", [(np.float32, 1.0e6), (np.int16, 70000)], ids=["float32", "int16"])
def test_a_correction_without_flagged_cells_gives_the_plain_decode_and_the_converted_inference(dtype, eps):
    h, n = roi.params_id(DIMS)
    dec = roi.decoded(dtype, DIMS)
    blob = ebr.build(dec.copy(), roi.reference(dtype, GATHER_TYPES[0][1] if dtype == np.float32 else 2, DIMS).copy(), eps, RANGES[dtype], params_hash=h, n_params=n)["bytes"]
    corr = api.Correction.from_bytes(blob)
    assert corr.info()["n_flagged"] == 0
    voxels = voxel_list(DIMS)
    st, msg, got, before = gather(corr, DIMS, voxels, verify=True)
    assert st == 0 and same_bytes(got[:len(voxels)], at(dec, voxels)), msg
    coords, v = points(DIMS)
    st, msg, got, before = sample(corr, DIMS, coords, verify=True)
    assert st == 0 and same_bytes(got[:len(coords)], csr.convert(csr.Source(blob, "fixed"), v)), msg
    assert not corr.residency()["on_device"]                                 # nothing touched the device on its behalf
    corr.release()


def test_sample_without_flagged_cells_and_without_a_range_is_the_inference():
    h, n = roi.params_id(DIMS)
    dec = roi.decoded(np.float32, DIMS)
    blob = ebr.build(dec.copy(), dec.copy(), 1e-3, None, params_hash=h, n_params=n)["bytes"]
    corr = api.Correction.from_bytes(blob)
    coords, v = points(DIMS)
    assert same_bytes(sampled(corr, DIMS, coords), v)
    corr.release()


# ------------------------------------------------------------------------------------------------ 6. corrections from bytes
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("source", ["fixed", "packed", "coded"])
def test_first_use_of_a_correction_from_bytes_uploads_the_form_that_is_set(source, form):
    dtype, eps = GATHER_TYPES[0]
    blob, packed, corrected = roi.expected(dtype, eps, DIMS)
    corr = {"fixed": lambda: api.Correction.from_bytes(blob), "packed": lambda: api.Correction.from_packed_bytes(packed),
            "coded": lambda: api.Correction.from_coded_bytes(ccr.encode(blob))}[source]()
    corr.set_resident_form(form)
    assert not corr.residency()["on_device"]
    voxels = voxel_list(DIMS)
    assert same_bytes(gathered(corr, DIMS, voxels), at(corrected, voxels))
    r = corr.residency()
    assert r["on_device"] and r["form"] == form
    if form == "packed":                                                     # no fixed-width payload and no cell table of it
        assert r["payload_device_bytes"] == roi.packed_payload_bytes(packed) and r["device_bytes"] == r["payload_device_bytes"] + r["index_device_bytes"]
    else:
        assert r["payload_device_bytes"] == roi.fixed_payload_bytes(blob) and r["index_device_bytes"] == 0
    coords, v = points(DIMS)                                                 # and the sampler reads what is resident now
    assert same_bytes(sampled(corr, DIMS, coords[:4096]), csr.sample(csr.Source(blob, form), v[:4096], coords[:4096]))
    assert corr.residency() == r
    corr.release()


# ------------------------------------------------------------------------------------------------ 7. sample equals the restatement
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dims", BOTH_DIMS, ids=DIM_IDS)
@pytest.mark.parametrize("dtype,eps", SAMPLE_TYPES, ids=SAMPLE_IDS)
def test_sample_equals_the_restatement(dtype, eps, dims, form, monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    coords, v = points(dims)
    blob = roi.expected(dtype, eps, dims)[0]
    corr = roi.correction(dtype, eps, dims, form)
    want = csr.sample(csr.Source(blob, form), v, coords)
    got = sampled(corr, dims, coords)
    assert same_bytes(got, want)
    assert not same_bytes(got, csr.convert(csr.Source(blob, form), v))       # residuals were added
    monkeypatch.setenv("VNR_AMD_DECODE_CHUNK", "64")
    assert same_bytes(sampled(corr, dims, coords), want)
    for n in (1, 63, 65):
        assert same_bytes(sampled(corr, dims, coords[7:7 + n]), want[7:7 + n]), n


# ------------------------------------------------------------------------------------------------ 8. clean cells
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype,eps", SAMPLE_TYPES, ids=SAMPLE_IDS)
def test_sample_in_clean_cells_is_the_converted_inference(dtype, eps, form):
    rng = np.random.default_rng(3)
    n = 2000                                                                 # t_x in [0, 14.5], t_z in [16.1, 19.5 -> 19]: x < 16 and z >= 16
    coords = np.stack([rng.uniform(0.5, 15.0, n) / DIMS[0], rng.uniform(0.0, 1.0, n), rng.uniform(16.6, 20.0, n) / DIMS[2]], axis=1).astype(np.float32)
    src = csr.Source(roi.expected(dtype, eps, DIMS)[0], form)
    q = csr.corners(src, coords)[0]
    assert not any(q[c][b][a].any() for c in range(2) for b in range(2) for a in range(2))
    v = api.neural_inference(roi.trained(DIMS)[1], coords)
    assert same_bytes(sampled(roi.correction(dtype, eps, DIMS, form), DIMS, coords), csr.convert(src, v))


# ------------------------------------------------------------------------------------------------ 9. verbatim
@pytest.mark.parametrize("form", FORMS)
def test_sample_refuses_a_verbatim_correction(form):
    dtype, eps = GATHER_TYPES[3]
    corr = roi.correction(dtype, eps, DIMS, form)
    assert corr.info()["kind"] == 2
    st, msg, got, before = sample(corr, DIMS, points(DIMS)[0][:100])
    assert st != 0 and "verbatim correction" in msg and same_bytes(got, before)
    with pytest.raises(api.VnrAmdError, match="verbatim correction"):
        api.vnrNeuralVolumeSampleCorrected(roi.trained(DIMS)[1], corr, api.DeviceArray((4, 3), np.float32))


# ------------------------------------------------------------------------------------------------ 10. the parameter check
def test_verify_params_refuses_other_parameters_in_both_calls():
    dtype, eps = SAMPLE_TYPES[0]
    corr = roi.correction(dtype, eps, DIMS, "packed")
    voxels, (coords, _) = voxel_list(DIMS)[:500], points(DIMS)
    coords = coords[:500]
    cfg = syn.model_config(n_levels=4, n_features=2, log2_hashmap_size=12, base_resolution=4, n_neurons=16, n_hidden_layers=1)
    other = api.vnrCreateNeuralVolume(cfg, DIMS)
    p = api.neural_get_params_fp16(roi.trained(DIMS)[1]).copy()
    api.neural_set_params_fp16(other, p)
    st, msg, got, _ = gather(corr, DIMS, voxels, nv=other, verify=True)      # the same parameters in another volume
    assert st == 0 and same_bytes(got[:500], at(roi.expected(dtype, eps, DIMS)[2], voxels)), msg
    k = int(np.flatnonzero(np.isfinite(p) & (p != 0))[0])
    p.view(np.uint16)[k] ^= 1                                                # one fp16 value, by one ulp
    api.neural_set_params_fp16(other, p)
    for call, arg in ((gather, voxels), (sample, coords)):
        st, msg, got, before = call(corr, DIMS, arg, nv=other, verify=True)
        assert st != 0 and "hash differs" in msg and same_bytes(got, before), msg
        st, msg, got, before = call(corr, DIMS, arg, nv=other, verify=False)
        assert st == 0 and not same_bytes(got[:500], before[:500]), msg
        st, msg, _, _ = call(corr, DIMS, arg, verify=True)                   # the volume it was built on
        assert st == 0, msg
    # dims that differ
    tail = roi.correction(dtype, eps, TAIL_DIMS, "packed")
    for call, arg in ((gather, voxels), (sample, coords)):
        st, msg, got, before = call(tail, DIMS, arg)
        assert st != 0 and "differ from the volume's" in msg and same_bytes(got, before)
    other.release()


def test_python_entry_points_return_device_arrays():
    dtype, eps = GATHER_TYPES[1]
    corr, nv = roi.correction(dtype, eps, DIMS, "fixed"), roi.trained(DIMS)[1]
    voxels = voxel_list(DIMS)[:1000]
    d_v = api.DeviceArray.from_numpy(np.ascontiguousarray(voxels))
    out = api.vnrNeuralVolumeGatherVoxelsCorrected(nv, corr, d_v)
    assert out.dtype == np.dtype(dtype) and same_bytes(out.numpy(), at(roi.expected(dtype, eps, DIMS)[2], voxels))
    coords, v = points(DIMS)
    d_c = api.DeviceArray.from_numpy(np.ascontiguousarray(coords[:1000]))
    values = api.vnrNeuralVolumeSampleCorrected(nv, corr, d_c, out=api.DeviceArray((1000,), np.float32))
    assert same_bytes(values.numpy(), csr.sample(csr.Source(roi.expected(dtype, eps, DIMS)[0], "fixed"), v[:1000], coords[:1000]))
    with pytest.raises(api.VnrAmdError, match="at least 1000"):
        api.vnrNeuralVolumeSampleCorrected(nv, corr, d_c, out=api.DeviceArray((10,), np.float32))
    for d in (d_v, d_c, out, values):
        d.free()
