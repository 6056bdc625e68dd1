"""Error-guided sampling on the GPU (include/vnr_amd.h "error-guided training batches") against the numpy restatement
of tests/guided_sampling_ref.py.  The definition is integer work or single fp32 / fp64 roundings, so every comparison is bit for bit.

Shapes: (16, 16, 16) is one cell; (19, 37, 50) has 2 x 3 x 4 cells, ragged on all axes; (640, 48, 144) has 1080 cells, more than
one scan block of 256; (4100, 4100, 2) has 66 049 cells, more than the 256 x 256 two scan levels cover, so the scan runs three.

Data-parallel training is not covered here: the two-rank shm pattern of tests/test_gpu_dist.py starts two processes that each
train a model, which does not fit a few seconds next to these cases.  What a rank runs per step is the call the training
integration test below steps by hand."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guided_sampling_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

RAGGED = (19, 37, 50)
SHAPES = {"one_cell": (16, 16, 16), "ragged": RAGGED, "blocks": (640, 48, 144), "levels": (4100, 4100, 2)}
BATCH = 1 << 16


def small_model():
    return syn.model_config(n_levels=4, n_features=2, log2_hashmap_size=12, base_resolution=4, n_neurons=16, n_hidden_layers=1)


def field(dims, seed=3):
    """[z, y, x] float32 in [0, 1]; with value_range (0, 1) the volume's voxels are these values exactly"""
    return np.random.default_rng(seed).uniform(0.0, 1.0, dims[::-1]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def volume(name):
    """-> (simple volume, its voxels [z, y, x] or None for the Perlin volume of the large shape, a neural volume that lets the sampler be seeded)"""
    dims = SHAPES[name]
    if name == "levels":
        return api.vnrCreateSimpleVolumePerlin(dims, seed=1, octaves=1), None, None
    vox = field(dims)
    vox.setflags(write=False)
    sv = api.vnrCreateSimpleVolume(vox, value_range=(0.0, 1.0))
    return sv, vox, api.vnrCreateNeuralVolume(small_model(), sv)


def seed_sampler(nv, seed, stream):
    api.check(api.lib().vnrAmdNeuralVolumeSetSamplerSeed(nv.h, seed, stream))


@functools.lru_cache(maxsize=None)
def briefly_trained():
    """-> (simple volume, voxels, neural volume trained 60 steps on a smooth field over the ragged shape); the model stays as it is"""
    before = os.environ.get("VNR_AMD_INIT_SEED")
    os.environ["VNR_AMD_INIT_SEED"] = "4711"
    try:
        z0, y0 = (50 - RAGGED[2]) // 2, (50 - RAGGED[1]) // 2
        a = syn.analytic_volume(50)[z0:z0 + RAGGED[2], y0:y0 + RAGGED[1], :RAGGED[0]]
        vox = np.ascontiguousarray((a - a.min()) / (a.max() - a.min()), dtype=np.float32)
        sv = api.vnrCreateSimpleVolume(vox, value_range=(0.0, 1.0))
        nv = api.vnrCreateNeuralVolume(small_model(), sv)
        seed_sampler(nv, 99, 7)
        api.vnrNeuralVolumeTrain(nv, 60, True)
    finally:
        if before is None:
            os.environ.pop("VNR_AMD_INIT_SEED", None)
        else:
            os.environ["VNR_AMD_INIT_SEED"] = before
    return sv, vox, nv


def error_map(sv, nv):
    """the two-call form's first half: ErrorAgainstDevice on the ground truth's own float voxels -> (report, block_max [z, y, x])"""
    p = api.lib().vnrAmdSimpleVolumeDeviceData(sv.h)
    r = api.vnrNeuralVolumeErrorAgainstDevice(nv, p, np.float32, block_map=True)
    return {k: v for k, v in r.items() if k != "block_max"}, r["block_max"]


def patterns(n):
    rng = np.random.default_rng(n)
    hot = np.zeros(n, np.float32)
    hot[n // 3] = 0.37
    edges = rng.uniform(0.1, 1.0, n).astype(np.float32)
    edges[:max(1, n // 5)] = 0.0
    edges[n - max(1, n // 7):] = 0.0
    if n == 1:
        edges[:] = 0.5
    span = (10.0 ** rng.uniform(-30, 0, n)).astype(np.float32)
    span[rng.integers(0, n)] = 1.0
    span[::5] = np.float32(1e-45) if n > 5 else span[::5]   # fp32 denormals
    return {"equal": np.full(n, 0.731, np.float32), "hot": hot, "edges": edges, "span": span}


def assert_table(sv, w, fraction):
    t = ref.table(w, fraction)
    info = api.simple_volume_sampling_info(sv)
    assert info == {"active": True, "n_cells": t["n_cells"], "total": t["total"], "uniform_fraction": float(np.float32(fraction))}
    assert np.array_equal(api.simple_volume_sampling_cdf(sv), t["cdf"])
    return t


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("name", list(SHAPES))
def test_table_equals_numpy(name):
    sv = volume(name)[0]
    n = int(np.prod(ref.cell_dims(SHAPES[name])))
    assert n == {"one_cell": 1, "ragged": 24, "blocks": 1080, "levels": 66049}[name]
    for k, (pattern, w) in enumerate(patterns(n).items()):
        api.simple_volume_set_sampling_weights(sv, w, (0.0, 0.25, 1.0, 0.6)[k])
        t = assert_table(sv, w, (0.0, 0.25, 1.0, 0.6)[k])
        if pattern == "span" and n > 5:
            assert (t["q"] == 1).any()
    api.simple_volume_set_sampling_weights(sv, None)


def test_table_of_an_error_map_of_a_briefly_trained_model():
    sv, _, nv = briefly_trained()
    report, block_max = error_map(sv, nv)
    assert block_max.shape == (4, 3, 2) and report["max_abs"] > 0 and float(block_max.max()) == np.float32(report["max_abs"])
    api.simple_volume_set_sampling_weights(sv, block_max, 0.125)
    assert_table(sv, block_max, 0.125)
    api.simple_volume_set_sampling_weights(sv, None)


# ------------------------------------------------------------------------------------------------ the draws
def weights_for_draws(n):
    w = np.random.default_rng(11).uniform(0.0, 1.0, n).astype(np.float32) ** 3
    w[0] = 0.0
    w[n // 2] = 0.0
    w[n - 1] = 1e-7
    return w


@pytest.mark.parametrize("fraction", [0.0, 0.25, 1.0])
def test_draws_equal_numpy_and_calls_follow_one_another(fraction):
    sv, vox, nv = volume("ragged")
    w = weights_for_draws(24)
    api.simple_volume_set_sampling_weights(sv, w, fraction)
    t = assert_table(sv, w, fraction)
    seed, stream = 77 + int(fraction * 100), 13
    seed_sampler(nv, seed, stream)
    offset = 0
    for n in (1, 63, 4097):
        c, v = api.simple_volume_take_samples_weighted(sv, n)
        wc, uniform, cells = ref.draw(t, RAGGED, n, offset, seed, stream)
        assert np.array_equal(c.view(np.uint32), wc.view(np.uint32)), (n, fraction)
        assert np.array_equal(v.view(np.uint32), ref.values(vox, wc).view(np.uint32)), (n, fraction)
        assert (c >= 0).all() and (c < 1).all()
        if fraction == 1.0:   # draws 3 to 5 untouched
            assert uniform.all() and np.array_equal(c, ref.uint_to_float(ref.pcg32_uints(n, offset, seed, stream, 6)[:, 3:6]))
        if fraction == 0.0:
            assert not uniform.any() and t["q"][cells].min() > 0
        offset += 6 * n
        if n == 63:   # a uniform TakeSamples in between continues at offset + 6 n and stays on the stream
            c, v = api.simple_volume_take_samples(sv, 100)
            wc = ref.uniform_coords(100, offset, seed, stream)
            assert np.array_equal(c.view(np.uint32), wc.view(np.uint32))
            assert np.array_equal(v.view(np.uint32), ref.values(vox, wc).view(np.uint32))
            offset += 3 * 100
    api.simple_volume_set_sampling_weights(sv, None)


@pytest.mark.parametrize("staged", ["0", "1"])
def test_draws_on_more_cells_than_one_block_with_both_searches(monkeypatch, staged):
    """1080 cells: the staged top of the CDF has 540 entries of stride 2, the plain search 11 steps; the same bits either way"""
    monkeypatch.setenv("VNR_AMD_GUIDED_LDS", staged)
    sv, vox, nv = volume("blocks")
    w = weights_for_draws(1080)
    api.simple_volume_set_sampling_weights(sv, w, 0.1)
    t = assert_table(sv, w, 0.1)
    seed_sampler(nv, 5, 2 ** 63 + 9)
    c, v = api.simple_volume_take_samples_weighted(sv, 3001)
    wc, uniform, cells = ref.draw(t, SHAPES["blocks"], 3001, 0, 5, 2 ** 63 + 9)
    assert np.array_equal(c.view(np.uint32), wc.view(np.uint32))
    assert np.array_equal(v.view(np.uint32), ref.values(vox, wc).view(np.uint32))
    assert len(np.unique(cells[~uniform])) > 256
    api.simple_volume_set_sampling_weights(sv, None)


def test_all_weight_on_the_last_ragged_cell():
    """cell (1, 2, 3) of (19, 37, 50) is 3 x 5 x 2 voxels: every coordinate inside its box (upper face included) and below 1"""
    sv, vox, nv = volume("ragged")
    w = np.zeros(24, np.float32)
    w[23] = 3.5
    api.simple_volume_set_sampling_weights(sv, w, 0.0)
    seed_sampler(nv, 1, 1)
    c, v = api.simple_volume_take_samples_weighted(sv, 20000)
    assert (c < 1).all()
    for a, lo in enumerate((16, 32, 48)):
        x = c[:, a].astype(np.float64) * RAGGED[a]
        assert x.min() >= lo - 1e-5 and x.max() <= RAGGED[a]
        assert (c[:, a] >= np.float32(lo) * (np.float32(1) / np.float32(RAGGED[a]))).all()
    wc, _, cells = ref.draw(ref.table(w, 0.0), RAGGED, 20000, 0, 1, 1)
    assert (cells == 23).all() and np.array_equal(c.view(np.uint32), wc.view(np.uint32))
    api.simple_volume_set_sampling_weights(sv, None)


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_weights_leave_the_previous_table_in_force():
    sv, vox, nv = volume("ragged")
    good = weights_for_draws(24)
    api.simple_volume_set_sampling_weights(sv, good, 0.5)
    t = assert_table(sv, good, 0.5)
    for bad, word in ((np.nan, "NaN"), (-0.5, "negative"), (np.inf, "infinity"), (-np.inf, "infinity")):
        w = good.copy()
        w[17] = bad
        with pytest.raises(api.VnrAmdError, match=word):
            api.simple_volume_set_sampling_weights(sv, w, 0.25)
        assert_table(sv, good, 0.5)
    with pytest.raises(api.VnrAmdError, match="all weights are zero"):
        api.simple_volume_set_sampling_weights(sv, np.zeros(24, np.float32), 0.25)
    assert_table(sv, good, 0.5)
    d = api.DeviceArray.from_numpy(good)
    assert api.lib().vnrAmdSimpleVolumeSetSamplingWeights(sv.h, C.c_void_p(d.ptr), 1.25, None) != 0
    assert "uniform_fraction must lie in [0, 1]" in api._lib.last_error()
    assert_table(sv, good, 0.5)
    # the table still draws
    seed_sampler(nv, 3, 3)
    c, _ = api.simple_volume_take_samples_weighted(sv, 257)
    assert np.array_equal(c.view(np.uint32), ref.draw(t, RAGGED, 257, 0, 3, 3)[0].view(np.uint32))
    # NULL clears it, and the weighted draw then fails by name
    api.simple_volume_set_sampling_weights(sv, None)
    assert api.simple_volume_sampling_info(sv) == {"active": False, "n_cells": 0, "total": 0, "uniform_fraction": 0.0}
    assert api.simple_volume_sampling_cdf(sv) is None
    with pytest.raises(api.VnrAmdError, match="no sampling weights"):
        api.simple_volume_take_samples_weighted(sv, 16)
    # a neural handle is not a simple volume
    assert api.lib().vnrAmdSimpleVolumeSetSamplingWeights(nv.h, C.c_void_p(d.ptr), 0.5, None) != 0
    assert "expecting a simple volume" in api._lib.last_error()
    assert api.lib().vnrAmdNeuralVolumeGuideSamplingByError(sv.h, 0.5, None) != 0
    assert "expecting a neural volume" in api._lib.last_error()
    d.free()


def test_an_out_of_core_volume_is_refused(tmp_path):
    vol = np.random.default_rng(0).integers(0, 255, (4, 20, 40), dtype=np.uint8)
    path = tmp_path / "vol.raw"
    path.write_bytes(vol.tobytes())
    sv = api.vnrCreateSimpleVolumeOutOfCore(path, (40, 20, 4), np.uint8, (0.0, 255.0), n_concurrent_blocks=2, n_blocks=8)
    with pytest.raises(api.VnrAmdError, match="out-of-core"):
        api.simple_volume_set_sampling_weights(sv, np.ones(3 * 2 * 1, np.float32), 0.5)
    assert not api.simple_volume_sampling_info(sv)["active"]
    with pytest.raises(api.VnrAmdError, match="no sampling weights"):
        api.simple_volume_take_samples_weighted(sv, 16)


# ------------------------------------------------------------------------------------------------ training
def params_bits(nv):
    return api.neural_get_params_fp16(nv).view(np.uint16)


def hand_step(sv, nv, weighted, bufs):
    """one training step on a batch the test draws itself: the weighted or the uniform draw -> ForwardBackward -> TrainEnd"""
    c, v = bufs
    L = api.lib()
    if weighted:
        api.check(L.vnrAmdSimpleVolumeTakeSamplesWeighted(sv.h, BATCH, c.ptr, v.ptr, None))
    else:
        api.check(L.vnrAmdSimpleVolumeTakeSamples(sv.h, BATCH, api._fp(api._vec((0, 0, 0))), api._fp(api._vec((1, 1, 1))), c.ptr, v.ptr, None))
    api.check(L.vnrAmdNeuralVolumeForwardBackward(nv.h, BATCH, c.ptr, v.ptr))
    api.check(L.vnrAmdNeuralVolumeTrainEnd(nv.h, 1.0, 0))


def test_training_draws_from_the_table(monkeypatch):
    """deterministic training: vnrAmdNeuralVolumeTrain with a table equals the same steps made by hand on a twin, bit for bit; without
    the table the next steps equal the uniform hand loop; the test loss stays uniform (3 draws per sample) with a table set"""
    monkeypatch.setenv("VNR_AMD_INIT_SEED", "1234")
    monkeypatch.delenv("VNR_AMD_TRAIN_OVERLAP", raising=False)
    dims = (40, 36, 33)
    vox = np.clip(1.6 * syn.analytic_volume(40)[:33, :36, :40] - 0.3, 0, 1).astype(np.float32)
    w = np.random.default_rng(2).uniform(0.0, 1.0, 27).astype(np.float32) ** 2
    w[5] = 0.0
    pair = []
    for _ in range(2):
        sv = api.vnrCreateSimpleVolume(vox, value_range=(0.0, 1.0))
        nv = api.vnrCreateNeuralVolume(small_model(), sv)
        api.neural_set_deterministic_training(nv, True)
        seed_sampler(nv, 424242, 3)
        api.simple_volume_set_sampling_weights(sv, w, 0.25)
        pair.append((sv, nv))
    (sv_a, nv_a), (sv_b, nv_b) = pair
    assert np.array_equal(params_bits(nv_a), params_bits(nv_b))
    start = params_bits(nv_a).copy()
    bufs = (api.DeviceArray((BATCH, 3), np.float32), api.DeviceArray((BATCH,), np.float32))
    api.vnrNeuralVolumeTrain(nv_a, 8, False)
    for _ in range(8):
        hand_step(sv_b, nv_b, True, bufs)
    assert api.vnrNeuralVolumeGetTrainingStep(nv_a) == 8 and api.vnrNeuralVolumeGetTrainingStep(nv_b) == 8
    assert not np.array_equal(params_bits(nv_a), start)
    assert np.array_equal(params_bits(nv_a), params_bits(nv_b))
    # the last guided batch is where the restatement puts it: samples of step 8 start at 6 * 7 * BATCH
    c = bufs[0].numpy()
    wc = ref.draw(ref.table(w, 0.25), dims, 512, 6 * 7 * BATCH, 424242, 3)[0]
    assert np.array_equal(c[:512].view(np.uint32), wc.view(np.uint32))
    # the test loss draws 3 floats per sample, table or not: a following TakeSamples tells by its offset
    assert np.isfinite(api.vnrNeuralVolumeGetTestingLoss(nv_a))
    offset = 6 * 8 * BATCH + 3 * BATCH
    c, _ = api.simple_volume_take_samples(sv_a, 64)
    assert np.array_equal(c.view(np.uint32), ref.uniform_coords(64, offset, 424242, 3).view(np.uint32))
    c, _ = api.simple_volume_take_samples(sv_b, BATCH + 64)   # the twin catches up: the same 3 * (BATCH + 64) draws
    # without the table: the code and the stream of before
    api.simple_volume_set_sampling_weights(sv_a, None)
    api.simple_volume_set_sampling_weights(sv_b, None)
    api.vnrNeuralVolumeTrain(nv_a, 3, False)
    for _ in range(3):
        hand_step(sv_b, nv_b, False, bufs)
    assert np.array_equal(params_bits(nv_a), params_bits(nv_b))
    offset += 3 * 64 + 3 * 3 * BATCH
    c, _ = api.simple_volume_take_samples(sv_a, 64)
    assert np.array_equal(c.view(np.uint32), ref.uniform_coords(64, offset, 424242, 3).view(np.uint32))


# ------------------------------------------------------------------------------------------------ the loop in one call
def test_guide_sampling_by_error_equals_the_two_calls():
    sv, _, nv = briefly_trained()
    api.simple_volume_set_sampling_weights(sv, None)
    report, block_max = error_map(sv, nv)
    api.simple_volume_set_sampling_weights(sv, block_max, 0.3)
    cdf = api.simple_volume_sampling_cdf(sv)
    info = api.simple_volume_sampling_info(sv)
    api.simple_volume_set_sampling_weights(sv, None)
    got = api.neural_volume_guide_sampling_by_error(nv, 0.3)
    assert got == report
    assert api.simple_volume_sampling_info(sv) == info and np.array_equal(api.simple_volume_sampling_cdf(sv), cdf)
    assert np.array_equal(cdf, ref.table(block_max, 0.3)["cdf"])
    # a refused call leaves it in force
    assert api.lib().vnrAmdNeuralVolumeGuideSamplingByError(nv.h, -1.0, None) != 0
    assert "uniform_fraction" in api._lib.last_error()
    assert np.array_equal(api.simple_volume_sampling_cdf(sv), cdf)
    api.simple_volume_set_sampling_weights(sv, None)


def test_guide_sampling_by_error_on_a_fresh_model_and_without_ground_truth():
    sv, vox, _ = volume("ragged")
    fresh = api.vnrCreateNeuralVolume(small_model(), sv)
    r = api.neural_volume_guide_sampling_by_error(fresh, 0.0)
    assert r["max_abs"] > 0 and r["n_voxels"] == vox.size
    info = api.simple_volume_sampling_info(sv)
    assert info["active"] and info["n_cells"] == 24 and info["total"] >= 1 << 24
    api.simple_volume_set_sampling_weights(sv, None)
    alone = api.vnrCreateNeuralVolume(small_model(), RAGGED)
    with pytest.raises(api.VnrAmdError, match="no resident ground truth"):
        api.neural_volume_guide_sampling_by_error(alone, 0.0)
    # the all-zero refusal (a perfect fit) is the two-call form's: zeros through SetSamplingWeights
    with pytest.raises(api.VnrAmdError, match="all weights are zero"):
        api.simple_volume_set_sampling_weights(sv, np.zeros((4, 3, 2), np.float32), 0.0)
    assert not api.simple_volume_sampling_info(sv)["active"]
