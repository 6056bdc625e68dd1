"""Random access to the corrected field, the host side (include/vnr_amd.h, "random access to the corrected field"): the numpy
restatement tests/correction_sample_ref.py against error_bound_ref on synthetic fields (no network: the "network's values" are
arrays), its convex bound, five deliberate mistakes that each change a result, and what the two entry points answer without a
device.  CPU only; every comparison of stored values has tolerance zero and compares bytes."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from instantvnr_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import correction_pack_cases as cases  # noqa: E402
import correction_sample_ref as csr  # noqa: E402
import error_bound_ref as ebr  # noqa: E402

DIMS = [(40, 24, 20), (21, 10, 3)]
DIM_IDS = ["40x24x20", "21x10x3"]
LONG_DIMS = (1024, 3, 2)                             # one axis of 1024: 64 cells in a row, t up to 1023
GATHER_TYPES = [(np.float32, 1e-3), (np.int16, 2), (np.uint32, 1), (np.float64, 0), (np.float64, 1e-3), (np.int32, 1), (np.float32, 0), (np.uint8, 3), (np.int8, 0),
                (np.uint16, 1)]
SAMPLE_TYPES = [(np.float32, 1e-3), (np.int16, 2), (np.float64, 1e-3)]
ROUTES = ["fixed", "packed"]
F32 = np.float32


def ids(types):
    return [f"{t.__name__}-{e}" for t, e in types]


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def synthetic(dtype, eps, dims, value_range=None):
    """-> (dec, ref, fixed-width blob) of correction_pack_cases.fields; an unsigned or 8-bit type gets the int16 fields moved into its range"""
    dt = np.dtype(dtype)
    own = dt.kind == "f" or (dt.kind == "i" and dt.itemsize > 1)
    dec, ref = cases.fields(dtype if own else np.int16, dims, eps, seed=dims[0] * 7 + dt.itemsize)
    if not own:
        lift = 0 if dt.kind == "i" else (128 if dt.itemsize == 1 else 40000)
        dec, ref = (np.clip(a.astype(np.int64) // (80 if dt.itemsize == 1 else 1) + lift, np.iinfo(dt).min, np.iinfo(dt).max).astype(dt) for a in (dec, ref))
    if value_range is None:
        value_range = (0.0, 1.0) if dt.kind in "iu" else (1.0, 0.0)
    return dec, ref, ebr.build(dec.copy(), ref.copy(), eps, value_range)["bytes"]


def all_voxels(dims, seed):
    z, y, x = np.meshgrid(*(np.arange(d) for d in dims[::-1]), indexing="ij")
    v = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    return v[np.random.default_rng(seed).permutation(len(v))]


# ------------------------------------------------------------------------------------------------ 1. lerp endpoints
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype,eps", [(np.float32, 1e-3), (np.int16, 2)], ids=["kind1", "kind0"])
def test_integral_t_gives_the_corrected_voxel_before_its_cast(dtype, eps, route):
    dims = DIMS[0]
    dec, ref, blob = synthetic(dtype, eps, dims)
    src = csr.Source(blob, route)
    voxels = all_voxels(dims, 1)
    coords = np.stack([[csr.integral_coord(int(i), dims[a]) for i in voxels[:, a]] for a in range(3)], axis=1).astype(F32)
    for a in range(3):                                        # the precondition: t is the voxel index exactly, so w = 0
        i0, _, w, t = csr.axis_place(coords[:, a], dims[a])
        assert np.array_equal(i0, voxels[:, a]) and not w.any() and np.array_equal(t, voxels[:, a].astype(F32))
    dec_at = dec[voxels[:, 2], voxels[:, 1], voxels[:, 0]]
    v = dec_at.astype(F32)                                    # range (0, 1) or none: d = v, and an integer dec is exact in float32
    assert np.array_equal(csr.convert(src, v), v)
    q = ebr.quantise(dec, ref, eps)[0]
    cell_flagged = csr.Source(blob, "fixed").codes(voxels[:, 0], voxels[:, 1], voxels[:, 2])[1]
    q_at = np.where(cell_flagged, q[voxels[:, 2], voxels[:, 1], voxels[:, 0]], 0)
    got = csr.sample(src, v, coords)
    if src.kind == 1:                                         # corrected_value's own cast is the sample's cast
        want = ebr.corrected_value(dec_at, q_at, 1, src.step)
    else:                                                     # dec + q s in int64, before the clamp to the type
        want = (dec_at.astype(np.int64) + q_at * src.step).astype(np.float64).astype(F32)
        inside = np.abs(dec_at.astype(np.int64) + q_at * src.step) <= 32767
        assert inside.any() and np.array_equal(ebr.corrected_value(dec_at, q_at, 0, src.step)[inside].astype(F32), want[inside])
    assert (q_at != 0).sum() > 1000 and same_bytes(got, want)


# ------------------------------------------------------------------------------------------------ 2. the gather
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dims", DIMS, ids=DIM_IDS)
@pytest.mark.parametrize("dtype,eps", GATHER_TYPES, ids=ids(GATHER_TYPES))
def test_gather_over_a_permuted_list_equals_apply(dtype, eps, dims, route):
    dec, _, blob = synthetic(dtype, eps, dims)
    want = ebr.apply(dec.copy(), blob)
    assert not same_bytes(want, dec)
    voxels = np.concatenate([all_voxels(dims, 2), all_voxels(dims, 3)[:100]])       # duplicates
    got = csr.gather(csr.Source(blob, route), dec[voxels[:, 2], voxels[:, 1], voxels[:, 0]], voxels)
    assert same_bytes(got, want[voxels[:, 2], voxels[:, 1], voxels[:, 0]])


# ------------------------------------------------------------------------------------------------ 3. the convex bound
@pytest.mark.parametrize("dims", DIMS + [LONG_DIMS], ids=DIM_IDS + ["1024x3x2"])
@pytest.mark.parametrize("dtype,eps", SAMPLE_TYPES, ids=ids(SAMPLE_TYPES))
def test_convex_bound_at_the_voxel_centres(dtype, eps, dims):
    """|sample - (d + residual(voxel))| <= (delta_x + delta_y + delta_z) (max - min of the eight residuals) + slack.  The slack is the
    roundings the bound leaves out: the result's rounding to float32, half an ulp of it, and at most 22 double roundings (three a
    lerp, seven lerps, one of d + blend) of values no larger than |d| + max |residual|, each 2^-53 relative: 22 * 2^-53 < 2^-48."""
    dec, _, blob = synthetic(dtype, eps, dims, (-3.0, 9.5) if np.dtype(dtype).kind == "f" else (0.0, 1.0))
    coords = csr.voxel_centres(dims)
    v = np.random.default_rng(dims[0]).uniform(0.0, 1.0, len(coords)).astype(F32)
    worst = 0.0
    for route in ROUTES:
        src = csr.Source(blob, route)
        got = csr.sample(src, v, coords).astype(np.float64)
        centre, bound = csr.centre_bound(src, v, coords)
        q, _, t = csr.corners(src, coords)
        rmax = np.max([np.abs(csr.residual(src, q[c][b][a])) for c in range(2) for b in range(2) for a in range(2)], axis=0)
        slack = np.spacing(np.abs(got).astype(F32)).astype(np.float64) / 2 + 2.0 ** -48 * (np.abs(centre) + rmax)
        assert (np.abs(got - centre) <= bound + slack).all()
        # the centres: t is an integer within rounding, on (1024, 3, 2) exactly, where the bound is 0 and the slack is all there is
        assert (bound.max() > 0) == (dims != LONG_DIMS) and max(np.abs(ta - np.rint(ta)).max() for ta in t) < 2.0 ** -10
        worst = max(worst, float((np.abs(got - centre) - slack).max()))
    print("largest |sample - centre| beyond the roundings", worst)


# ------------------------------------------------------------------------------------------------ 4. sharpness
def point_sets(dims):
    return np.concatenate([csr.voxel_centres(dims), csr.uniform_points(4096, 11), csr.edge_points(dims)])


@pytest.mark.parametrize("broken", csr.BROKEN)
def test_each_broken_variant_differs_on_the_point_sets(broken):
    differs = {}
    for dtype, eps in SAMPLE_TYPES[:2]:
        for dims in DIMS:
            # (an integer type needs a range: with (-0.0, 1.0) the conversion v * 1 + -0.0 keeps v, the sign of a zero included)
            _, _, blob = synthetic(dtype, eps, dims, (-0.0, 1.0) if np.dtype(dtype).kind == "i" else None)
            coords = point_sets(dims)
            # the values: seeded, and -0.0 wherever all eight codes are 0, which only the rule "all eight 0: d as it is" keeps
            v = np.random.default_rng(5).uniform(0.0, 1.0, len(coords)).astype(F32)
            q = csr.corners(csr.Source(blob, "fixed"), coords)[0]
            clean = ~np.any([q[c][b][a] != 0 for c in range(2) for b in range(2) for a in range(2)], axis=0)
            v[clean] = F32(-0.0)
            for route in ROUTES:
                want = csr.sample(csr.Source(blob, route), v, coords)
                assert same_bytes(want, csr.sample(csr.Source(blob, "fixed"), v, coords))
                assert clean.sum() > 100 and np.signbit(want[clean]).all()
                differs[(dtype.__name__, dims, route)] = not same_bytes(csr.sample(csr.Source(blob, route, broken), v, coords), want)
    if broken == "no-zigzag":                                  # a mistake of the plane route alone
        assert all(d == (route == "packed") for (_, _, route), d in differs.items()), differs
    elif broken == "neighbour-cell":                           # shows where a cell is clean: (21, 10, 3) has none
        assert all(d == (dims == DIMS[0]) for (_, dims, _), d in differs.items()), differs
    else:
        assert all(differs.values()), differs


def test_the_edge_set_holds_what_it_is_for():
    for dims in DIMS:
        pts = csr.edge_points(dims)
        tx = pts[:, 0].astype(np.float64) * dims[0] - 0.5
        assert (tx < 0).any() and (tx > dims[0] - 1).any() and (pts == 0.0).any() and (pts == 1.0).any()
        assert ((tx > 15) & (tx < 16)).any() and ((tx > 31) & (tx < 32)).any() == (dims[0] > 32)
    # (21, 10, 3): the pair x = 19, 20 of row ly = 2, lz = 1 of the cell with cx = 5 is codes 63 and 64 of the cell: two groups
    src = csr.Source(synthetic(np.int16, 2, DIMS[1])[2], "packed")
    i0, i1, _, _ = csr.axis_place(csr.edge_points(DIMS[1])[:, 0], 21)
    j0 = csr.axis_place(csr.edge_points(DIMS[1])[:, 1], 10)[0]
    k0 = csr.axis_place(csr.edge_points(DIMS[1])[:, 2], 3)[0]
    assert ((i0 == 19) & (i1 == 20) & (j0 == 2) & (k0 == 1)).any() and 3 + 5 * (2 + 10 * 1) == 63
    # a NaN coordinate lands at t = 0
    assert [int(a) for a in csr.axis_place(F32("nan"), 21)[:2]] == [0, 1] and csr.axis_place(F32("nan"), 21)[2] == 0
    assert src.kind == 0


# ------------------------------------------------------------------------------------------------ 5. the interface, without a device
NAMES = ("vnrAmdNeuralVolumeGatherVoxelsCorrected", "vnrAmdNeuralVolumeSampleCorrected")


def test_header_library_and_bindings_know_both_entry_points():
    text = open(os.path.join(ROOT, "include", "vnr_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code)
        assert name in api._lib.declared_symbols()
        f = getattr(api.lib(), name)                          # exported
        assert f.argtypes is not None and len(f.argtypes) == 7
    assert "random access to the corrected field" in text and "E + 0.5" in text and "delta_x + delta_y + delta_z" in text
    assert callable(api.vnrNeuralVolumeGatherVoxelsCorrected) and callable(api.vnrNeuralVolumeSampleCorrected)
    for doc in ("INTEGRATION.md", "README.md"):
        assert all(n in open(os.path.join(ROOT, doc)).read() for n in NAMES), doc


def test_refusals_that_need_no_device_are_reported_by_name():
    L = api.lib()
    fake, odd = C.c_void_p(256), C.c_void_p(258)              # never dereferenced: every call below is refused before
    corr = api.Correction.from_bytes(synthetic(np.float64, 1e-3, DIMS[1])[2])
    verbatim = api.Correction.from_bytes(synthetic(np.float32, 0, DIMS[1])[2])
    assert corr.info()["kind"] == 1 and verbatim.info()["kind"] == 2

    def refused(f, word, handle, n, a, b):
        st = f(None, handle, n, a, b, None, 1)
        msg = api._lib.last_error()
        assert st != 0 and word in msg, (word, msg)

    for f, first in ((L.vnrAmdNeuralVolumeGatherVoxelsCorrected, "null voxel list"), (L.vnrAmdNeuralVolumeSampleCorrected, "null coordinates")):
        refused(f, "null correction", None, 5, fake, fake)
        refused(f, first, corr.h, 5, None, fake)
        refused(f, "null device data", corr.h, 5, fake, None)
        refused(f, "not aligned to 4 bytes", corr.h, 5, odd, fake)
        refused(f, "not aligned to its value type", corr.h, 5, fake, odd)
        refused(f, "null volume", corr.h, 5, fake, fake)
        refused(f, "null volume", corr.h, 0, fake, fake)      # an empty list is no way round a handle; with a volume it is a success (GPU tests)
        refused(f, first, corr.h, 0, None, fake)
    refused(L.vnrAmdNeuralVolumeGatherVoxelsCorrected, "not aligned to its value type (8 bytes)", corr.h, 5, fake, C.c_void_p(260))
    refused(L.vnrAmdNeuralVolumeGatherVoxelsCorrected, "null volume", verbatim.h, 5, fake, fake)      # the gather takes a verbatim correction
    refused(L.vnrAmdNeuralVolumeSampleCorrected, "verbatim correction", verbatim.h, 5, fake, fake)
    refused(L.vnrAmdNeuralVolumeSampleCorrected, "verbatim correction", verbatim.h, 0, None, None)    # by name, before anything else is looked at
    assert not corr.residency()["on_device"] and not verbatim.residency()["on_device"]
    with pytest.raises(api.VnrAmdError, match=r"shape \(n, 3\)"):
        api.vnrNeuralVolumeSampleCorrected(None, corr, np.zeros((4, 3), np.float32))
    corr.release(); verbatim.release()


def test_the_series_tool_offers_a_probe():
    import subprocess
    text = open(os.path.join(ROOT, "tools", "README.md")).read()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "insitu_series.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    assert "--probe" in text and "--probe" in out.stdout
