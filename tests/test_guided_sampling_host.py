"""CPU checks of error-guided sampling (include/vnr_amd.h "error-guided training batches"): the C-ABI declares and
exports the five entry points, the Python layer binds and wraps them, the refusals that need no device are reported by name, and
the numpy restatement the GPU tests compare with (tests/guided_sampling_ref.py) is sane on its own.  No kernel runs here.

Without a device neither a simple nor a neural volume can exist, so of the handle refusals only the null handle is reached here;
the neural handle, the out-of-core volume and the invalid weights are cases of tests/test_gpu_guided_sampling.py.  The fraction is
an argument check in front of the handle, which is what makes it reachable here."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from instantvnr_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guided_sampling_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vnrAmdSimpleVolumeSetSamplingWeights", "vnrAmdSimpleVolumeSamplingInfo", "vnrAmdSimpleVolumeSamplingCdf",
         "vnrAmdSimpleVolumeTakeSamplesWeighted", "vnrAmdNeuralVolumeGuideSamplingByError"]
DIMS = (19, 37, 50)   # 2 x 3 x 4 = 24 cells, ragged on all axes


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


def test_header_declares_the_entry_points():
    text = open(_lib.HEADER).read()
    assert re.search(r"int\s+vnrAmdSimpleVolumeSetSamplingWeights\(vnrAmdVolume simple, const float\* d_weights, float uniform_fraction, void\* stream\);", text)
    assert re.search(r"int\s+vnrAmdSimpleVolumeSamplingInfo\(vnrAmdVolume simple, int\* active, uint64_t\* n_cells, uint64_t\* total, float\* uniform_fraction\);", text)
    assert re.search(r"const uint64_t\*\s+vnrAmdSimpleVolumeSamplingCdf\(vnrAmdVolume simple\);", text)
    assert re.search(r"int\s+vnrAmdSimpleVolumeTakeSamplesWeighted\(vnrAmdVolume simple, size_t n, float\* d_coords, float\* d_values, void\* stream\);", text)
    assert re.search(r"int\s+vnrAmdNeuralVolumeGuideSamplingByError\(vnrAmdVolume neural, float uniform_fraction, vnrAmdDecodeError\* report\);", text)
    for n in NAMES:
        assert n in _lib.declared_symbols()
    # the arithmetic is part of the interface
    for phrase in ("16777216.0", "4294967296.0", "__umul64hi", "0x1.fffffep-1f", "offset + 6e"):
        assert phrase in text, phrase


def test_library_exports_them_and_lib_binds_them(L):
    for n, n_args in zip(NAMES, (4, 5, 1, 5, 3)):
        fn = getattr(L, n)
        assert fn.argtypes is not None and len(fn.argtypes) == n_args, n
    assert L.vnrAmdSimpleVolumeSamplingCdf.restype is C.c_void_p
    for n in (NAMES[0], NAMES[1], NAMES[3], NAMES[4]):
        assert getattr(L, n).restype is C.c_int
    assert C.POINTER(_lib.DecodeError) in L.vnrAmdNeuralVolumeGuideSamplingByError.argtypes
    for n in ("simple_volume_set_sampling_weights", "simple_volume_take_samples_weighted", "simple_volume_sampling_info",
              "simple_volume_sampling_cdf", "neural_volume_guide_sampling_by_error"):
        assert callable(getattr(api, n))


def test_refusals_that_need_no_device_are_reported_by_name(L):
    info = (C.c_int(), C.c_uint64(), C.c_uint64(), C.c_float())
    assert L.vnrAmdSimpleVolumeSetSamplingWeights(None, C.c_void_p(0x1000), 0.5, None) != 0
    assert "null volume" in _lib.last_error()
    assert L.vnrAmdSimpleVolumeSamplingInfo(None, *(C.byref(x) for x in info)) != 0
    assert "null volume" in _lib.last_error()
    assert L.vnrAmdSimpleVolumeSamplingCdf(None) is None
    assert "null volume" in _lib.last_error()
    assert L.vnrAmdSimpleVolumeTakeSamplesWeighted(None, 16, C.c_void_p(0x1000), C.c_void_p(0x2000), None) != 0
    assert "null volume" in _lib.last_error()
    assert L.vnrAmdNeuralVolumeGuideSamplingByError(None, 0.5, None) != 0
    assert "null volume" in _lib.last_error()
    for bad in (-0.25, 1.5, float("nan"), float("inf")):
        assert L.vnrAmdSimpleVolumeSetSamplingWeights(None, C.c_void_p(0x1000), bad, None) != 0
        assert "uniform_fraction must lie in [0, 1]" in _lib.last_error()
        assert L.vnrAmdNeuralVolumeGuideSamplingByError(None, bad, None) != 0
        assert "uniform_fraction must lie in [0, 1]" in _lib.last_error()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) for arguments the wrapper must refuse itself")


@pytest.mark.parametrize("fraction", [-0.1, 1.0001, float("nan"), "much", None])
def test_wrappers_refuse_a_bad_fraction_without_calling_the_library(monkeypatch, fraction):
    monkeypatch.setattr(api, "lib", lambda: _NoLibrary())
    volume = type("V", (), {"h": 0x2000})()
    with pytest.raises(api.VnrAmdError, match="uniform_fraction"):
        api.simple_volume_set_sampling_weights(volume, np.ones(24, np.float32), fraction)
    with pytest.raises(api.VnrAmdError, match="uniform_fraction"):
        api.neural_volume_guide_sampling_by_error(volume, fraction)


# ------------------------------------------------------------------------------------------------ the restatement's own sanity
def weights24():
    """24 weights over six decades with two zero cells (one of them the first, one in the middle)"""
    w = np.random.default_rng(5).uniform(0.0, 1.0, 24).astype(np.float32) ** 4
    w[0] = 0.0
    w[13] = 0.0
    w[7] = 1e-6
    return w


def test_restated_pcg32_equals_the_oracle(oracle):
    L = oracle.lib()
    for seed, stream, offset in ((1337, ref.DEFAULT_STREAM, 0), (99, 7, 123457), (2 ** 63 + 11, 2 ** 64 - 3, 6 * 65536 * 1000 + 5)):
        r = oracle.pcg32(seed, stream)
        L.vnro_pcg32_advance(C.byref(r), C.c_int64(offset))
        want = np.array([L.vnro_pcg32_next_uint(C.byref(r)) for _ in range(600)], np.uint32)
        assert np.array_equal(ref.pcg32_uints(100, offset, seed, stream, 6).ravel(), want)
        assert np.array_equal(ref.pcg32_uints(600, offset, seed, stream, 1).ravel(), want)
    assert np.array_equal(ref.uniform_coords(50, 30, 1337).ravel(), oracle.pcg32_floats(150, 30, 1337))


def test_table_restatement():
    t = ref.table(weights24(), 0.25)
    q = t["q"]
    assert q[0] == 0 and q[13] == 0 and q.max() == 1 << 24 and t["total"] == int(q.astype(object).sum())
    assert q[7] == round(1e-6 / float(weights24().max()) * 2 ** 24)
    assert t["threshold"] == 1 << 30 and ref.table(weights24(), 1.0)["threshold"] == 1 << 32 and ref.table(weights24(), 0.0)["threshold"] == 0
    # the floor: a positive weight that rounds to 0 still gets 1, fp32 denormals included
    tiny = ref.table(np.array([1.0, 1e-30, 1e-45, 0.0, 2.0 ** -26], np.float32), 0.0)
    assert list(tiny["q"]) == [1 << 24, 1, 1, 0, 1] and list(tiny["cdf"]) == [1 << 24, (1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 2, (1 << 24) + 3]
    # ties to even: 2^-25 * 2^24 = 0.5 -> 0 -> floored to 1; 1.5 -> 2; 2.5 -> 2
    ties = ref.table(np.array([1.0, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24], np.float32), 0.0)
    assert list(ties["q"]) == [1 << 24, 1, 2, 2]
    for bad in ([1.0, np.nan], [1.0, -1e-3], [np.inf, 1.0], [0.0, 0.0, -0.0]):
        with pytest.raises(ValueError):
            ref.table(np.array(bad, np.float32), 0.0)
    with pytest.raises(ValueError):
        ref.table(np.ones(3, np.float32), 1.5)


def test_restated_draws_follow_the_table():
    """200 000 samples, seed 2024 / sequence 5, a quarter uniform: per cell the weighted branch's count stays within 5 sigma of
    n_weighted * q / total (binomial), no weighted sample falls into a cell with q = 0, all coordinates lie in [0, 1)."""
    n = 200000
    t = ref.table(weights24(), 0.25)
    coords, uniform, cells = ref.draw(t, DIMS, n, offset=0, seed=2024, stream=5)
    assert coords.dtype == np.float32 and (coords >= 0).all() and (coords < 1).all()
    share = uniform.mean()
    assert abs(share - 0.25) < 5 * np.sqrt(0.25 * 0.75 / n)
    nw = int((~uniform).sum())
    p = t["q"].astype(np.float64) / t["total"]
    hist = np.bincount(cells[~uniform], minlength=24)
    sigma = np.sqrt(nw * p * (1 - p))
    assert (np.abs(hist - nw * p) <= 5 * sigma).all(), (hist, nw * p, sigma)
    assert hist[0] == 0 and hist[13] == 0
    # a weighted sample lies in the box of its cell (upper face included); a uniform one is draws 3 to 5 untouched
    cd = ref.cell_dims(DIMS)
    c_axis = (cells % cd[0], (cells // cd[0]) % cd[1], cells // (cd[0] * cd[1]))
    for a in range(3):
        lo = 16 * c_axis[a]
        hi = np.minimum(lo + 16, DIMS[a])
        v = coords[~uniform, a].astype(np.float64) * DIMS[a]
        assert (v >= lo[~uniform] - 1e-4).all() and (v <= hi[~uniform] + 1e-4).all()
    u = ref.pcg32_uints(n, 0, 2024, 5, 6)
    assert np.array_equal(coords[uniform], ref.uint_to_float(u[:, 3:6])[uniform])
    # samples in the zero cells exist all the same: through the uniform share
    in_zero = (coords[:, 0] * DIMS[0] < 16) & (coords[:, 1] * DIMS[1] < 16) & (coords[:, 2] * DIMS[2] < 16)
    assert in_zero.any() and uniform[in_zero].all()


def test_documents_describe_the_feature():
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "vnrAmdSimpleVolumeSetSamplingWeights" in integration and "vnrAmdNeuralVolumeGuideSamplingByError" in integration
    assert "vnrAmdNeuralVolumeGuideSamplingByError" in open(os.path.join(ROOT, "README.md")).read()
    assert "guided_sampler.hip" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "--guided" in open(os.path.join(ROOT, "tools", "README.md")).read()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "insitu_series.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--guided" in out.stdout and "--uniform-fraction" in out.stdout and "--refresh-every" in out.stdout
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vnr_cmd_train.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--guided-every" in out.stdout and "--uniform-fraction" in out.stdout
