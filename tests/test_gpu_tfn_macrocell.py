"""What decides which matter a frame shows, on the GPU against tests/tfn_macrocell_ref.py (numpy; held to the C oracle by
tests/test_tfn_macrocell_ref_host.py on these same inputs): the macrocell a neural volume builds from samples, what training leaves in it,
the per-cell opacity bound for every table length and window, and frames under windowed value ranges and long tables, where the compose
kernels read the tables from global memory.  Integer work, comparisons and single fp32 roundings: value ranges and bounds are compared bit
for bit; frames keep the bars tests/test_gpu_render.py states for the same paths."""
import functools
import os
import sys

import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn
from instantvnr_amd._lib import check, lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guided_sampling_ref as gref  # noqa: E402
import tfn_macrocell_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH = 1 << 16          # NeuralVolume's training batch (network.cu:183)
RAGGED = ref.VOLUMES[0]
FRAME_WINDOWS = [(0.0, 1.0), (0.25, 0.7), (-0.5, 0.4)]
TABLE_PAIRS = [(256, 256), (1228, 1228), (1229, 1229), (1536, 1), (4096, 4096), (300, 4096)]
SIZES = {"decoupled": (96, 80), "coupled": (200, 144)}


def psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 199.0 if mse == 0 else 10 * np.log10(1.0 / mse)


def small_model():
    return syn.model_config(n_levels=4, n_features=2, log2_hashmap_size=12, base_resolution=4, n_neurons=16, n_hidden_layers=1)


def field(dims, seed=3):
    """[z, y, x] float32 in [0, 1]; with value_range (0, 1) the volume's voxels are these values exactly"""
    return np.random.default_rng(seed).uniform(0.0, 1.0, dims[::-1]).astype(np.float32)


def online_volume(dims_or_voxels, online=True, seed=None):
    """-> (ground truth, its voxels, a small neural volume over it); seed = (seed, stream) of the ground truth's sampler"""
    vox = field(dims_or_voxels) if isinstance(dims_or_voxels, tuple) else dims_or_voxels
    sv = api.vnrCreateSimpleVolume(vox, value_range=(0.0, 1.0))
    nv = api.vnrCreateNeuralVolume(small_model(), sv, online_macrocell_construction=online)
    if seed is not None:
        check(lib().vnrAmdNeuralVolumeSetSamplerSeed(nv.h, seed[0], seed[1]))
    return sv, vox, nv


def feed(nv, coords, values):
    dc, dv = api.DeviceArray.from_numpy(np.ascontiguousarray(coords)), api.DeviceArray.from_numpy(np.ascontiguousarray(values))
    check(lib().vnrAmdNeuralVolumeUpdateMacrocell(nv.h, coords.shape[0], dc.ptr, dv.ptr, None))
    check(lib().vnrAmdSynchronize())


def make_tfn(colors, alphas, window):
    t = api.vnrCreateTransferFunction()
    api.vnrTransferFunctionSetColor(t, colors)
    api.vnrTransferFunctionSetAlpha(t, alphas)
    api.vnrTransferFunctionSetValueRange(t, window)
    return t


def set_bound(volume, tfn):
    check(lib().vnrAmdVolumeUpdateMaxOpacity(volume.h, tfn.h))
    return api.volume_macrocell(volume)["max_opacity"]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ============================================================================================= a. the explicit kernel, exact
@pytest.mark.parametrize("dims", ref.VOLUMES)
def test_online_macrocell_equals_numpy_for_every_batch_size(dims):
    for n in ref.BATCH_SIZES:
        coords, values = ref.batch(dims, n)
        _, _, nv = online_volume(dims)
        before = api.volume_macrocell(nv)
        assert before["dims"] == ref.cell_dims(dims) and not before["value_range"].any()
        feed(nv, coords, values)
        want = ref.explicit_update(ref.empty_range(dims), dims, coords, values)
        assert same_bits(api.volume_macrocell(nv)["value_range"], want), (dims, n)


@pytest.mark.parametrize("dims", ref.VOLUMES)
def test_online_macrocell_merges_calls_and_ignores_the_order(dims):
    coords, values = ref.batch(dims, 5000)
    want = ref.explicit_update(ref.empty_range(dims), dims, coords, values)
    _, _, two = online_volume(dims)
    feed(two, coords[:2743], values[:2743])
    first = api.volume_macrocell(two)["value_range"]
    assert same_bits(first, ref.explicit_update(ref.empty_range(dims), dims, coords[:2743], values[:2743]))
    feed(two, coords[2743:], values[2743:])
    assert same_bits(api.volume_macrocell(two)["value_range"], want)
    _, _, shuffled = online_volume(dims)
    order = np.random.default_rng(8).permutation(5000)
    feed(shuffled, coords[order], values[order])
    assert same_bits(api.volume_macrocell(shuffled)["value_range"], want)


# ============================================================================================= b. what training leaves
def uniform_batches(vox, k, seed):
    """the k batches vnrNeuralVolumeTrain draws: BATCH samples each, 3 floats of the sampler's pcg32 stream per sample, call after call"""
    out = []
    for step in range(k):
        c = gref.uniform_coords(BATCH, 3 * BATCH * step, *seed)
        out.append((c, gref.values(vox, c)))
    return out


def merged(dims, batches, start=None):
    vr = ref.empty_range(dims) if start is None else start
    for c, v in batches:
        vr = ref.explicit_update(vr, dims, c, v)
    return vr


TRAIN_TFN = dict(window=(0.25, 0.7), n=1229)


def training_case(online=True, seed=(4242, 5)):
    """a volume with a transfer function and a bound that is not all zeros: one batch fed by hand before any training"""
    sv, vox, nv = online_volume(RAGGED, online=online, seed=seed)
    alphas = ref.alpha_table(TRAIN_TFN["n"])
    tfn = make_tfn(ref.color_table(2), alphas, TRAIN_TFN["window"])
    start = ref.empty_range(RAGGED)
    if online:
        c, v = ref.online_batch()
        feed(nv, c, v)
        start = ref.online_range()
    mo = set_bound(nv, tfn)
    window = ref.tfn_window(*TRAIN_TFN["window"])
    if online:
        assert same_bits(mo, ref.max_opacity(alphas, window, start)) and (mo > 0).any() and (mo == 0).any()
    return sv, vox, nv, alphas, window, start, mo


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("how", ["train", "begin_end"])
def test_training_leaves_the_batches_in_the_online_macrocell(fast, how):
    """vnrNeuralVolumeTrain(nv, 3, fast) and three TrainBegin / TrainEnd pairs: the value range is the three batches of the sampler's
    stream merged into what was there (nothing else draws from the stream in between).  The bound: Train(..., fast = False) ends with a
    refresh (NeuralVolume::train, network.cu:778), Train(..., fast = True) leaves it alone on purpose, and TrainEnd never touches it"""
    seed = (4242, 5)
    _, vox, nv, alphas, window, start, mo_before = training_case(seed=seed)
    if how == "train":
        api.vnrNeuralVolumeTrain(nv, 3, fast)
    else:
        for _ in range(3):
            api.neural_train_begin(nv)
            api.neural_train_end(nv, 1.0, fast)
    check(lib().vnrAmdSynchronize())
    assert api.vnrNeuralVolumeGetTrainingStep(nv) == 3
    want = merged(RAGGED, uniform_batches(vox, 3, seed), start)
    got = api.volume_macrocell(nv)
    assert same_bits(got["value_range"], want)
    fresh = ref.max_opacity(alphas, window, want)
    assert not same_bits(fresh, mo_before)          # the batches did move the bound, so "left alone" and "refreshed" differ
    if how == "train" and not fast:
        assert same_bits(got["max_opacity"], fresh)
    else:
        assert same_bits(got["max_opacity"], mo_before)


def test_a_step_on_the_caller_s_coordinates_leaves_the_macrocell_alone():
    _, vox, nv, _, _, start, mo_before = training_case()
    c = np.random.default_rng(2).uniform(0, 1, (BATCH, 3)).astype(np.float32)
    api.neural_forward_backward(nv, c, gref.values(vox, c))
    api.neural_train_end(nv, 1.0, False)
    check(lib().vnrAmdSynchronize())
    assert api.vnrNeuralVolumeGetTrainingStep(nv) == 1
    got = api.volume_macrocell(nv)
    assert same_bits(got["value_range"], start) and same_bits(got["max_opacity"], mo_before)


@pytest.mark.parametrize("fast", [False, True])
def test_training_leaves_a_ground_truth_macrocell_alone(oracle, fast):
    sv, vox, nv, alphas, window, _, _ = training_case(online=False)
    before = api.volume_macrocell(sv)
    assert same_bits(before["value_range"], oracle.macrocell_compute_implicit(vox))
    assert same_bits(before["max_opacity"], ref.max_opacity(alphas, window, before["value_range"]))
    api.vnrNeuralVolumeTrain(nv, 3, fast)
    check(lib().vnrAmdSynchronize())
    assert api.vnrNeuralVolumeGetTrainingStep(nv) == 3
    for volume in (sv, nv):     # (the neural volume shows the ground truth's)
        after = api.volume_macrocell(volume)
        assert same_bits(after["value_range"], before["value_range"]) and same_bits(after["max_opacity"], before["max_opacity"])


def test_guided_batches_reach_the_online_macrocell():
    """with a sampling table on the ground truth the batches are the table's draws (6 stream positions per sample); cells without weight are
    reached over their neighbours' aprons only, or not at all"""
    seed = (99, 11)
    sv, vox, nv = online_volume(RAGGED, seed=seed)
    w = np.zeros(ref.cell_dims(RAGGED)[::-1], np.float32)
    w[:2, :2, :] = np.random.default_rng(6).uniform(0.1, 1.0, (2, 2, 2))
    api.simple_volume_set_sampling_weights(sv, w, 0.0)
    table = gref.table(w, 0.0)
    api.vnrNeuralVolumeTrain(nv, 3, True)
    check(lib().vnrAmdSynchronize())
    batches = []
    for step in range(3):
        c = gref.draw(table, RAGGED, BATCH, 6 * BATCH * step, *seed)[0]
        batches.append((c, gref.values(vox, c)))
    want = merged(RAGGED, batches)
    assert same_bits(api.volume_macrocell(nv)["value_range"], want)
    seen = (want != 0).any(axis=-1)
    assert seen[:3].all() and not seen[3].any(), seen    # [z, y, x]: the weighted cells, one apron cell beyond them in y and z, nothing further


# ============================================================================================= c. the bound, exact
@functools.lru_cache(maxsize=None)
def bound_volumes():
    """-> {kind: (volume, its value range)}: the implicit macrocell of a ragged dense volume, an online one with unvisited cells"""
    from oracle import oracle
    oracle.build()
    vox = ref.ragged_volume()
    sv = api.vnrCreateSimpleVolume(vox, value_range=(0.0, 1.0))
    implicit = api.volume_macrocell(sv)["value_range"]
    assert same_bits(implicit, oracle.macrocell_compute_implicit(vox))
    _, _, nv = online_volume(RAGGED)
    feed(nv, *ref.online_batch())
    online = api.volume_macrocell(nv)["value_range"]
    assert same_bits(online, ref.online_range()) and (online == 0).all(axis=-1).any()
    return {"implicit": (sv, implicit), "online": (nv, online)}


@pytest.mark.parametrize("n", ref.ALPHA_LENGTHS)
def test_opacity_bound_equals_numpy(n):
    """every table length (a single entry; the last that fits the compose kernels' LDS and the first that does not; 8192, the last the bound
    kernel stages in its own LDS, and 8193, the first it reads from global memory; 16 385 entries, which would have been 64 KB + 4 bytes of
    dynamic LDS, and 65 536, 256 KB) under every window, for a dense volume's cells and for an online macrocell with cells nothing was
    seen in; with a table of white noise and with a rising and a falling ramp, on which a range one entry short at its upper or lower end
    changes every cell's bound (a library built with `j < iu` in the kernel's global-memory loop passed 16 384 entries of noise alone)"""
    colors = ref.color_table(2)
    for kind, (volume, vr) in bound_volumes().items():
        for table, alphas in ref.bound_tables(n).items():
            for window in ref.WINDOWS:
                got = set_bound(volume, make_tfn(colors, alphas, window))
                assert same_bits(got, ref.max_opacity(alphas, ref.tfn_window(*window), vr)), (kind, n, table, window)
        assert same_bits(api.volume_macrocell(volume)["value_range"], vr)


# ============================================================================================= d. frames of a dense volume
@functools.lru_cache(maxsize=None)
def dense_scene():
    vol = syn.analytic_volume(48)
    vol.setflags(write=False)
    cam = syn.oblique_camera((48, 48, 48))
    camera = api.vnrCreateCamera()
    api.vnrCameraSet(camera, cam["from"], cam["at"], cam["up"], cam["fovy"])
    return {"vol": vol, "sv": api.vnrCreateSimpleVolume(vol), "cam": cam, "camera": camera}


@functools.lru_cache(maxsize=None)
def tables(n_colors, n_alphas):
    colors = syn.tfn_ramp_with_bumps(n=n_colors)[0]
    alphas = syn.tfn_ramp_with_bumps(n=n_alphas)[1] if n_alphas > 1 else np.array([0.3], np.float32)   # (a one-entry ramp would be 0)
    return colors, alphas


def renderer(volume, tfn, size, mode=5, camera=None):
    r = api.vnrCreateRenderer(volume)
    api.vnrRendererSetTransferFunction(r, tfn)
    api.vnrRendererSetCamera(r, camera or dense_scene()["camera"])
    api.vnrRendererSetFramebufferSize(r, size)
    api.vnrRendererSetMode(r, mode)
    return r


def frame(r):
    api.vnrRender(r)
    return api.vnrRendererMapFrame(r).copy(), api.vnrRendererGetFrameStats(r)


def oracle_scene(oracle, pair, window, mo, size, dims=(48, 48, 48), **kw):
    cam = dense_scene()["cam"]
    colors, alphas = tables(*pair)
    otfn = oracle.TfnHolder(colors, alphas, *ref.tfn_window(*window)[:2])
    return oracle.SceneHolder(size[0], size[1], dims, otfn, mo, cam["from"], cam["at"], cam["up"], cam["fovy"], **kw)


def test_schedule_reports_where_the_tables_are():
    """the compose kernels keep both tables in LDS while they fit the budget the report names: for tables of equal length (16 + 4 bytes an
    entry) the last length that fits and the first that does not"""
    sc = dense_scene()
    r0 = renderer(sc["sv"], make_tfn(*tables(256, 256), (0.0, 1.0)), SIZES["decoupled"])
    frame(r0)
    budget = api.renderer_schedule(r0, tables=True)["tfn_lds_bytes"]
    assert budget >= 20 * 256 and api.renderer_schedule(r0, tables=True)["tfn_in_lds"]
    for size in SIZES.values():
        for fits in (True, False):
            n = budget // 20 + (0 if fits else 1)
            r = renderer(sc["sv"], make_tfn(*tables(n, n), (0.0, 1.0)), size)
            frame(r)
            assert api.renderer_schedule(r, tables=True)["tfn_in_lds"] == fits, (size, n)
    # the budget counts both tables: a long colour table with few opacities, a single colour with many opacities
    for pair in ((budget // 16, 1), (budget // 16 - 1, 4), (1, (budget - 16) // 4), (1, (budget - 16) // 4 + 1)):
        r = renderer(sc["sv"], make_tfn(*tables(*pair), (0.0, 1.0)), SIZES["decoupled"])
        frame(r)
        assert api.renderer_schedule(r, tables=True)["tfn_in_lds"] == (16 * pair[0] + 4 * pair[1] <= budget), pair


_unwindowed = {}


@pytest.mark.parametrize("window", FRAME_WINDOWS)
@pytest.mark.parametrize("pair", TABLE_PAIRS)
def test_windowed_frames_match_the_oracle(oracle, pair, window):
    """mode 5 on the dense volume through the decoupled loop (96 x 80) and the coupled one (200 x 144), tables in LDS and in global memory,
    against the oracle's marcher with the window clamped as the library clamps it and the library's own bound (held exact above).  The bar
    of tests/test_gpu_render.py's test_streaming_groundtruth_matches_oracle: identical arithmetic except powf, max |err| < 2e-4, PSNR > 80
    (measured over the 36 frames: max |err| 6.0e-8 .. 3.6e-7, PSNR 157.7 .. 167.6 dB; tables in LDS and in global memory alike)"""
    sc = dense_scene()
    colors, alphas = tables(*pair)
    tfn = make_tfn(colors, alphas, window)
    for loop, size in SIZES.items():
        r = renderer(sc["sv"], tfn, size)
        img, st = frame(r)
        sched = api.renderer_schedule(r, tables=True)
        assert sched["decoupled"] == (loop == "decoupled"), (loop, sched)
        assert sched["tfn_in_lds"] == (16 * pair[0] + 4 * pair[1] <= sched["tfn_lds_bytes"])
        mc = api.volume_macrocell(sc["sv"])
        mo = mc["max_opacity"]
        assert same_bits(mo, ref.max_opacity(alphas, ref.tfn_window(*window), mc["value_range"]))
        want, _, ost = oracle.render_streaming(oracle_scene(oracle, pair, window, mo, size), lambda c: oracle.sample_volume(sc["vol"], c, nodal=True))
        assert st["n_rays_hit"] == ost["n_rays_hit"] > 1000 and st["n_iterations"] == ost["n_iterations"]
        err = float(np.abs(img - want).max())
        print(f"\nwindowed frame {pair} {window} {loop}: max |err| {err:.2e}, PSNR {psnr(img, want):.1f} dB, cells of bound 0: {int((mo == 0).sum())} of {mo.size}")
        assert err < 2e-4 and psnr(img, want) > 80, (loop, err, psnr(img, want))
        assert (img[..., 3] > 0).mean() > 0.02
        # not vacuous: a window that were ignored would give the unwindowed frame, which is far from this one; and the window empties cells
        if window == FRAME_WINDOWS[0]:
            _unwindowed[(pair, loop)] = img
        else:
            if (pair, loop) not in _unwindowed:
                _unwindowed[(pair, loop)] = frame(renderer(sc["sv"], make_tfn(colors, alphas, FRAME_WINDOWS[0]), size))[0]
            assert float(np.abs(img - _unwindowed[(pair, loop)]).max()) > 0.05
        if window == (0.25, 0.7) and pair[1] > 1:
            assert (mo == 0).any() and (mo > 0).any()


LONG = (4096, 4096)
WINDOW = (0.25, 0.7)


def test_windowed_long_tables_in_the_monolithic_marcher(oracle):
    """mode 4, bar of test_monolithic_mode4_matches_oracle: max |err| < 2e-4, PSNR > 80 (measured 2.4e-7, 162.9 dB)"""
    sc = dense_scene()
    size = SIZES["decoupled"]
    img, _ = frame(renderer(sc["sv"], make_tfn(*tables(*LONG), WINDOW), size, mode=4))
    mo = api.volume_macrocell(sc["sv"])["max_opacity"]
    want, _ = oracle.render_monolithic(oracle_scene(oracle, LONG, WINDOW, mo, size), sc["vol"])
    err = float(np.abs(img - want).max())
    print(f"\nmode 4 {LONG} {WINDOW}: max |err| {err:.2e}, PSNR {psnr(img, want):.1f} dB")
    assert (want[..., 3] > 0).mean() > 0.02
    assert err < 2e-4 and psnr(img, want) > 80, (err, psnr(img, want))


def test_windowed_long_tables_with_gradient_shading(oracle):
    """mode 8, bar of test_gradient_shading_groundtruth_matches_oracle: max |err| < 2e-5, PSNR > 110 (measured 2.4e-7, 163.2 dB)"""
    sc = dense_scene()
    size = SIZES["decoupled"]
    img, st = frame(renderer(sc["sv"], make_tfn(*tables(*LONG), WINDOW), size, mode=8))
    mo = api.volume_macrocell(sc["sv"])["max_opacity"]
    want, _, ost = oracle.render_streaming(oracle_scene(oracle, LONG, WINDOW, mo, size, shading_mode=1),
                                           lambda c: oracle.sample_volume(sc["vol"], c, nodal=True))
    assert st["n_rays_hit"] == ost["n_rays_hit"] > 1000 and st["n_iterations"] == ost["n_iterations"]
    err = float(np.abs(img - want).max())
    print(f"\nmode 8 {LONG} {WINDOW}: max |err| {err:.2e}, PSNR {psnr(img, want):.1f} dB")
    assert err < 2e-5 and psnr(img, want) > 110, (err, psnr(img, want))


def test_windowed_long_tables_in_the_path_tracer(oracle):
    """mode 14, bar of test_path_tracing_streaming_matches_oracle: alpha equal, at least 0.995 of the pixels within 1e-5, mean within 2e-3
    (measured: every pixel within 1e-5, both means 0.01778)"""
    sc = dense_scene()
    size = SIZES["decoupled"]
    r = renderer(sc["sv"], make_tfn(*tables(*LONG), WINDOW), size, mode=14)
    api.vnrRendererSetVolumeDensityScale(r, 6.0)
    img, st = frame(r)
    mo = api.volume_macrocell(sc["sv"])["max_opacity"]
    want, _, ost = oracle.render_pathtracing(oracle_scene(oracle, LONG, WINDOW, mo, size, density_scale=6.0),
                                             lambda c: oracle.sample_volume(sc["vol"], c, nodal=True))
    assert st["n_rays_hit"] == ost["n_rays_hit"] > 1000
    assert np.array_equal(img[..., 3], want[..., 3])
    assert (want[..., :3].sum(axis=2) > 0).mean() > 0.03
    same = np.abs(img - want).max(axis=2) < 1e-5
    print(f"\nmode 14 {LONG} {WINDOW}: {same.mean():.4f} of the pixels within 1e-5, means {float(img[..., :3].mean()):.5f} / {float(want[..., :3].mean()):.5f}")
    assert same.mean() > 0.995, same.mean()
    assert abs(float(img[..., :3].mean()) - float(want[..., :3].mean())) < 2e-3


@pytest.mark.parametrize("pair", [(256, 256), (4096, 4096)])
def test_a_new_window_on_a_live_renderer(pair):
    """a value range changed on the transfer function and set again on a renderer that has rendered: the renderer's lookup and the volume's
    bound both follow, and the next frame is a fresh renderer's, bit for bit"""
    sc = dense_scene()
    colors, alphas = tables(*pair)
    for size in SIZES.values():
        tfn = make_tfn(colors, alphas, (0.0, 1.0))
        live = renderer(sc["sv"], tfn, size)
        first, _ = frame(live)
        api.vnrTransferFunctionSetValueRange(tfn, WINDOW)
        api.vnrRendererSetTransferFunction(live, tfn)
        mc = api.volume_macrocell(sc["sv"])
        assert same_bits(mc["max_opacity"], ref.max_opacity(alphas, ref.tfn_window(*WINDOW), mc["value_range"]))
        second, st = frame(live)
        fresh, fst = frame(renderer(sc["sv"], make_tfn(colors, alphas, WINDOW), size))
        assert same_bits(second, fresh) and st["n_samples"] == fst["n_samples"]
        assert float(np.abs(second - first).max()) > 0.05


# ============================================================================================= e. frames of a neural volume
def random_network(oracle, sv, online, seed=21):
    L, F, log2T, base, H = 8, 4, 14, 4, 2
    cfg = syn.model_config(n_levels=L, n_features=F, log2_hashmap_size=log2T, base_resolution=base, n_hidden_layers=H)
    nv = api.vnrCreateNeuralVolume(cfg, sv, online_macrocell_construction=online)
    info = api.neural_info(nv)
    api.neural_set_params_fp16(nv, syn.random_params(info["n_params"], oracle.mlp_n_params(info["padded_width"], 64, H - 1), seed=seed))
    return nv


def compositor_alone(oracle, nv, r, size, window):
    """the "compositor alone" method of test_neural_streaming_matches_oracle: the oracle's marcher fed by the library's network values at
    the oracle's own sample positions, with the bound read from the library; its bar: max |err| < 5e-6, PSNR > 130 (measured 1.8e-7, 157.9 dB
    with the ground-truth macrocell; 2.4e-7, 158.7 dB through the online one)"""
    img, st = frame(r)
    mo = api.volume_macrocell(nv)["max_opacity"]
    want, _, ost = oracle.render_streaming(oracle_scene(oracle, LONG, window, mo, size), lambda c: api.neural_inference(nv, c))
    assert st["n_rays_hit"] == ost["n_rays_hit"] and st["n_iterations"] == ost["n_iterations"]
    assert img[..., 3].max() > 0.05 and (img[..., 3] > 0).mean() > 0.02
    return img, want, mo


def test_neural_frame_under_a_window_and_long_tables(oracle):
    sc = dense_scene()
    size = (64, 56)
    nv = random_network(oracle, sc["sv"], online=False)
    img, want, mo = compositor_alone(oracle, nv, renderer(nv, make_tfn(*tables(*LONG), WINDOW), size), size, WINDOW)
    err = float(np.abs(img - want).max())
    print(f"\nneural frame, ground-truth macrocell, {LONG} {WINDOW}: max |err| {err:.2e}, PSNR {psnr(img, want):.1f} dB")
    assert (mo == 0).any()
    assert err < 5e-6 and psnr(img, want) > 130, (err, psnr(img, want))


def test_neural_frame_through_an_online_macrocell(oracle):
    """a neural volume that built its macrocell from 20 training batches, drawn from a sampling table that leaves a third of the volume
    without weight: cells that were trained on, cells reached over an apron only and cells never visited (their bound is 0: skipped)"""
    size = (64, 56)
    vol = dense_scene()["vol"]
    sv = api.vnrCreateSimpleVolume(vol)
    L, F, log2T, base, H = 8, 4, 14, 4, 2
    cfg = syn.model_config(n_levels=L, n_features=F, log2_hashmap_size=log2T, base_resolution=base, n_hidden_layers=H)
    before = os.environ.get("VNR_AMD_INIT_SEED")
    os.environ["VNR_AMD_INIT_SEED"] = "515"
    try:
        nv = api.vnrCreateNeuralVolume(cfg, sv, online_macrocell_construction=True)
    finally:
        if before is None:
            os.environ.pop("VNR_AMD_INIT_SEED", None)
        else:
            os.environ["VNR_AMD_INIT_SEED"] = before
    w = np.zeros((3, 3, 3), np.float32)
    w[:, :, 0] = 1.0                      # [z, y, x]: the cells of the first x layer
    api.simple_volume_set_sampling_weights(sv, w, 0.0)
    colors, alphas = tables(*LONG)
    window = (-0.5, 0.4)   # (clamped to (0, 0.4): what a briefly trained network puts out stays visible)
    r = renderer(nv, make_tfn(colors, alphas, window), size)     # (the volume holds the transfer function from here on)
    api.vnrNeuralVolumeTrain(nv, 20, False)
    mc = api.volume_macrocell(nv)
    never = (mc["value_range"] == 0).all(axis=-1)
    assert never[:, :, 2].all() and not never[:, :, :2].any()
    assert same_bits(mc["max_opacity"], ref.max_opacity(alphas, ref.tfn_window(*window), mc["value_range"]))
    assert not mc["max_opacity"][never].any() and (mc["max_opacity"] > 0).any()
    img, want, _ = compositor_alone(oracle, nv, r, size, window)
    err = float(np.abs(img - want).max())
    print(f"\nneural frame, online macrocell, {LONG} {window}: max |err| {err:.2e}, PSNR {psnr(img, want):.1f} dB")
    assert err < 5e-6 and psnr(img, want) > 130, (err, psnr(img, want))


def test_in_shader_kernel_under_a_window_and_long_tables(oracle):
    """mode 6 with the network inside the marching loop against the library's streaming path, as test_in_shader_kernel_on_a_neural_volume
    compares them (the C4 model shape, which has an in-shader instance): max |err| < 2e-3, PSNR > 70, the same rays hit (measured: the two
    frames are equal; the in-shader kernel reads the tables from global memory whatever their length)"""
    sc = dense_scene()
    L, F, log2T, base, pls, H = 16, 2, 19, 16, 1.3195, 3
    cfg = syn.model_config(n_levels=L, n_features=F, log2_hashmap_size=log2T, base_resolution=base, n_hidden_layers=H, per_level_scale=pls)
    nv = api.vnrCreateNeuralVolume(cfg, sc["sv"], online_macrocell_construction=False)
    info = api.neural_info(nv)
    api.neural_set_params_fp16(nv, syn.random_params(info["n_params"], oracle.mlp_n_params(info["padded_width"], 64, H - 1), seed=26))
    tfn = make_tfn(*tables(*LONG), WINDOW)
    frames, stats = {}, {}
    for kernel in (1, 0):
        r = renderer(nv, tfn, (64, 56), mode=6)
        check(lib().vnrAmdRendererSetInShaderKernel(r.h, kernel))
        frames[kernel], stats[kernel] = frame(r)
    assert stats[1]["n_iterations"] == 1 and stats[0]["n_iterations"] >= 1
    assert stats[1]["n_rays_hit"] == stats[0]["n_rays_hit"] > 1000
    assert frames[1][..., 3].max() > 0.05
    err = float(np.abs(frames[1] - frames[0]).max())
    print(f"\nin-shader mode 6, {LONG} {WINDOW}: max |err| {err:.2e}, PSNR {psnr(frames[1], frames[0]):.1f} dB")
    assert err < 2e-3 and psnr(frames[1], frames[0]) > 70, (err, psnr(frames[1], frames[0]))
