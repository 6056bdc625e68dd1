"""Path tracing on a neural volume (rendering modes 14 and 15), both implementations -- in_shader_pt_kernel (csrc/in_shader.h, the default) and the
streaming path tracer (render_pathtracing in csrc/render.hip) -- held to the oracle's path tracer on frames that are lit.

The models are those of tests/neural_pt_cases.py: tests/test_neural_pt_cases_host.py proves on the host that the oracle's frame of each is lit
and that its value varies in space, and every test here asserts again that its own reference frame is lit.  "The renderer alone" is the oracle's
path tracer fed by the LIBRARY's network values (the same bits in whatever batch they are asked for: tests/test_gpu_inference_stages.py), so what
is left between the two frames is the device's logf / sincosf against glibc's: a last-bit difference there can send a path another way, hence a
bar on the share of equal pixels (the dense-volume tests' bar, tests/test_gpu_render.py test_path_tracing_streaming_matches_oracle) -- and, on
a neural volume, moves the value a path sees (EQUAL below)."""
import os
import sys

import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn
from instantvnr_amd._lib import check, lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neural_pt_cases as npc  # noqa: E402

pytestmark = pytest.mark.gpu

KERNELS = {1: "in-shader", 0: "streaming"}


# A pixel counts as equal within 1e-5, and more than 0.995 of them must be: the dense-volume tests' cap.  On a neural volume it is also the guard of
# csrc/pt_device.h pt_logf / pt_sincosf: with the device library's logf and sincosf (last bit unlike glibc's on 39 % and 33 % of the path tracer's
# 2^24 random numbers) a sample lies an ulp of t away from the oracle's, a grid of random features multiplies that by its resolution, some fp16
# feature rounds the other way, and the pixel moves by 1e-4 .. 1e-3 on the same path: 0.951 .. 0.994 of the pixels were equal on 12 of the 13
# models below, and every pixel only with Nearest interpolation.
EQUAL = 1e-5


def make_scene(oracle, distance_scale=1.6):
    hs = npc.HostScene(oracle, distance_scale)
    sv = api.vnrCreateSimpleVolume(hs.vol)
    tfn = api.vnrCreateTransferFunction()
    api.vnrTransferFunctionSetColor(tfn, hs.colors)
    api.vnrTransferFunctionSetAlpha(tfn, hs.alphas)
    api.vnrTransferFunctionSetValueRange(tfn, (0, 1))
    camera = api.vnrCreateCamera()
    api.vnrCameraSet(camera, hs.cam["from"], hs.cam["at"], hs.cam["up"], hs.cam["fovy"])
    api.lib().vnrAmdVolumeUpdateMaxOpacity(sv.h, tfn.h)
    # the majorants the library tracks with are the ones the host test's frames were made with
    assert np.array_equal(api.volume_macrocell(sv)["max_opacity"], hs.max_opacity)
    return {"host": hs, "sv": sv, "tfn": tfn, "camera": camera, "runs": {}}


@pytest.fixture(scope="module")
def scene(oracle):
    return make_scene(oracle)


def neural_volume(oracle, scene, case):
    nv = api.vnrCreateNeuralVolume(npc.model_config(case), scene["sv"], online_macrocell_construction=False)
    params = npc.parameters(oracle, case)
    assert api.neural_info(nv)["n_params"] == params.size
    api.neural_set_params_fp16(nv, params)
    return nv, params


def library_frames(scene, nv, mode, kernel, density_scale, n_frames):
    r = api.vnrCreateRenderer(nv)
    api.vnrRendererSetTransferFunction(r, scene["tfn"])
    api.vnrRendererSetCamera(r, scene["camera"])
    api.vnrRendererSetFramebufferSize(r, npc.SIZE)
    api.vnrRendererSetMode(r, mode)
    api.vnrRendererSetVolumeDensityScale(r, density_scale)
    check(lib().vnrAmdRendererSetInShaderKernel(r.h, kernel))
    out = []
    for _ in range(n_frames):
        api.vnrRender(r)
        out.append((api.vnrRendererMapFrame(r).copy(), api.vnrRendererGetFrameStats(r)))
    return out


def oracle_frames(oracle, scene, value_fn, mode, density_scale, n_frames):
    out, acc = [], None
    for frame_index in range(1, n_frames + 1):
        sc = scene["host"].holder(oracle, mode=mode, frame_index=frame_index, density_scale=density_scale)
        want, acc, ost = oracle.render_pathtracing(sc, value_fn, accumulation=acc)
        out.append((want.copy(), ost))
    return out


def both_kernels_and_the_oracle(oracle, scene, what, make_volume, mode, density_scale=npc.DENSITY_SCALE, n_frames=2):
    """the oracle's path tracer on the LIBRARY's network values and the library's frames from both kernels, frame by frame of an accumulation;
    rendered once for the tests (and bars) that look at the same frames"""
    key = (what, mode, density_scale)
    if key not in scene["runs"]:
        nv = make_volume()
        wants = oracle_frames(oracle, scene, lambda c: api.neural_inference(nv, c), mode, density_scale, n_frames)
        scene["runs"][key] = wants, {kernel: library_frames(scene, nv, mode, kernel, density_scale, n_frames) for kernel in (1, 0)}
    return scene["runs"][key]


def assert_the_renderer_alone(oracle, scene, what, make_volume, mode, density_scale=npc.DENSITY_SCALE):
    """the bars of the dense-volume path-tracing tests on both kernels; returns the last reference frame"""
    wants, gots = both_kernels_and_the_oracle(oracle, scene, what, make_volume, mode, density_scale)
    lit = npc.lit_share(wants[0][0])
    assert lit >= npc.MIN_LIT, (what, "the reference frame is not lit", lit)
    misses = []      # every kernel and frame is looked at before the test fails: a report names both kernels

    def hold(ok, *what_missed):
        if not ok:
            misses.append(what_missed)

    for kernel in (1, 0):
        for k, ((img, st), (want, ost)) in enumerate(zip(gots[kernel], wants)):
            err = np.abs(img - want).max(axis=2)
            same = float((err < EQUAL).mean())
            mean_diff = abs(float(img[..., :3].mean()) - float(want[..., :3].mean()))
            print(f"\n{what} mode {mode} density {density_scale} {KERNELS[kernel]} frame {k + 1}: lit {npc.lit_share(want):.3f}, equal pixels {same:.4f} "
                  f"(worst {float(err.max()):.2e}), |mean difference| {mean_diff:.2e}, "
                  f"samples {st['n_samples']} / oracle {ost['n_samples']}, iterations {st['n_iterations']}")
            where = (what, mode, KERNELS[kernel], k + 1)
            hold(np.array_equal(img[..., 3], want[..., 3]) and (want[..., 3] == 1.0).all(), where, "alpha")
            hold(st["n_rays_hit"] == ost["n_rays_hit"] > 500, where, "rays hit", st["n_rays_hit"], ost["n_rays_hit"])
            hold(mean_diff < 2e-3, where, "image mean", mean_diff)
            hold(abs(st["n_samples"] - ost["n_samples"]) < 0.01 * ost["n_samples"], where, "evaluations", st["n_samples"], ost["n_samples"])
            hold(st["n_iterations"] == 1 if kernel == 1 else st["n_iterations"] > 1, where, "not the kernel that was asked for", st["n_iterations"])
            hold(same > 0.995, where, "share of equal pixels", same)
    assert not misses, misses
    return wants[-1][0]


@pytest.mark.parametrize("mode", [14, 15])
@pytest.mark.parametrize("name", sorted(npc.CASES))
def test_both_kernels_follow_the_oracle_on_the_library_s_network_values(oracle, scene, name, mode):
    """(a) every case, modes 14 and 15, in-shader kernel forced on and forced off, two accumulated frames of 64 x 48 at density scale 0.5: alpha 1
    everywhere, hit rays equal, image means within 2e-3, evaluations within 1 %, and more than 0.995 of the pixels within 1e-5 (a cap, not a
    tolerance).
    Measured on an MI355X: 1.0000 for every case, mode, kernel and frame, worst pixel 0.0 -- every frame is the oracle's bit for bit (lowest: 1.0000).
    With the device library's logf / sincosf in pt_device.h it was, mode 14 / mode 15: c4 0.9593 / 0.9508; f1-k32 0.9850 / 0.9831; f2-k64 0.9759 /
    0.9714; f4-k64 0.9681 / 0.9639; f8-k128 0.9668 / 0.9564; w128 0.9932 / 0.9919; w16 0.9733 / 0.9707; w16-f1 0.9840 / 0.9827;
    w16-tiled-smoothstep 0.9958 / 0.9932; w32 0.9772 / 0.9720; w32-f8 0.9912 / 0.9906; w32-nearest-quantized 1.0000 / 1.0000; w64-sigmoid-exp
    0.9938 / 0.9919.  With the two random draws of pt_shade's bounce swapped in a scratch build the test fails for both kernels (c4: 0.890 of the pixels in
    mode 14, 0.878 in mode 15; w16-f1 0.896 / 0.879; f8-k128 0.916 / 0.903)"""
    assert_the_renderer_alone(oracle, scene, name, lambda: neural_volume(oracle, scene, npc.CASES[name])[0], mode)


@pytest.mark.parametrize("density_scale", [0.25, 0.5, 6.0])
def test_thin_and_thick_media(oracle, scene, density_scale):
    """(b) the C4 shape at three thicknesses under the same bars: many real collisions per path in the thick medium; in the thin one a bounce
    often leaves the volume at once, where mode 15 collects the ambient light and mode 14 does not (method_pathtracing.cu:631-635 vs 447-452), so
    the two reference frames differ (327 pixels at 0.25) and the library has to follow each.
    Measured: every frame the oracle's bit for bit at all three (0.959 .. 0.987 with the device library's logf / sincosf)"""
    volume = lambda: neural_volume(oracle, scene, npc.CASES["c4"])[0]   # noqa: E731
    wants = {mode: assert_the_renderer_alone(oracle, scene, "c4", volume, mode, density_scale) for mode in (14, 15)}
    if density_scale == 0.25:
        differ = int((np.abs(wants[14] - wants[15]).max(axis=2) > 1e-6).sum())
        print(f"\nmodes 14 and 15 differ on {differ} pixels of the reference")
        assert differ > 10, differ


@pytest.mark.parametrize("name", ["c4", npc.GENERAL_CASE])
def test_end_to_end_against_the_oracle_s_own_network(oracle, scene, name):
    """(c) the whole chain, network included, against the oracle's path tracer on the oracle's network (fp32 accumulation), one frame.  The network
    values now differ at rounding level, and a value on the other side of a collision decision sends the path elsewhere; how many pixels that
    costs is measured on the reference itself, with the oracle's fp16-accumulating network (acc_mode 1) in place of the fp32 one: the library
    (MFMA, fp32 accumulation) must differ on no more pixels than that variant does, and its image mean by no more than max(2e-3, the variant's).
    Measured on an MI355X, pixels off the fp32 oracle frame, library (either kernel) against the fp16-accumulating oracle, of 3072: c4 3 against 437 (mode
    14), 1 against 455 (mode 15); w32-nearest-quantized 0 against 283 and 0 against 305.  Image means: library <= 3e-8, variant <= 1.3e-4"""
    case = npc.CASES[name]
    nv, params = neural_volume(oracle, scene, case)
    for mode in (14, 15):
        sc = lambda: scene["host"].holder(oracle, mode=mode, frame_index=1)   # noqa: E731
        want, _, _ = oracle.render_pathtracing(sc(), npc.oracle_network(oracle, case, params, acc_mode=0))
        variant, _, _ = oracle.render_pathtracing(sc(), npc.oracle_network(oracle, case, params, acc_mode=1))
        assert npc.lit_share(want) >= npc.MIN_LIT
        differs = lambda a: int((np.abs(a - want).max(axis=2) > 1e-5).sum())                                # noqa: E731
        mean_diff = lambda a: abs(float(a[..., :3].mean()) - float(want[..., :3].mean()))                   # noqa: E731
        n_pixels = want.shape[0] * want.shape[1]
        assert differs(variant) < 0.5 * n_pixels, (name, mode, "the variant is another image", differs(variant))
        for kernel in (1, 0):
            img, st = library_frames(scene, nv, mode, kernel, npc.DENSITY_SCALE, 1)[0]
            print(f"\n{name} mode {mode} {KERNELS[kernel]}: pixels off the fp32 oracle frame: library {differs(img)}, fp16-accumulate oracle {differs(variant)} "
                  f"of {n_pixels}; |mean difference| library {mean_diff(img):.2e}, variant {mean_diff(variant):.2e}")
            assert (img[..., 3] == 1.0).all()
            assert differs(img) <= differs(variant), (name, mode, KERNELS[kernel], differs(img), differs(variant))
            assert mean_diff(img) <= max(2e-3, mean_diff(variant)), (name, mode, KERNELS[kernel], mean_diff(img), mean_diff(variant))


@pytest.fixture(scope="module")
def trained(oracle):
    """L8 F4 T2^15 base 8 pls 1.5 H2 trained for 300 steps on the scene's volume, seen from half the distance: the volume is a blob in a mostly
    transparent box, and from the scene's camera the oracle's frame OF THE VOLUME ITSELF is lit on 0.04 of its pixels, from here on 0.16"""
    close = make_scene(oracle, distance_scale=0.8)
    L, F, log2T, base, pls, H = 8, 4, 15, 8, 1.5, 2
    cfg = syn.model_config(n_levels=L, n_features=F, log2_hashmap_size=log2T, base_resolution=base, n_hidden_layers=H, per_level_scale=pls)
    nv = api.vnrCreateNeuralVolume(cfg, close["sv"], online_macrocell_construction=False)
    api.vnrNeuralVolumeTrain(nv, 300, True)
    return close, nv, oracle.grid_config(L, F, log2T, base, pls), H


def test_the_trained_parameters_read_back_are_the_network_that_renders(oracle, trained):
    """the parameters read back drive the oracle's network to within the inference kernel's 2^-8 of the library's values: the frames below are
    made of this trained state, and its value does vary over the volume"""
    _, nv, ocfg, H = trained
    params = api.neural_get_params_fp16(nv)
    coords = np.random.default_rng(2).uniform(0, 1, (2000, 3)).astype(np.float32)
    got = api.neural_inference(nv, coords)
    want = oracle.network_inference(ocfg, 64, H, params.view(np.uint16), coords)
    assert np.abs(got - want).max() <= 2.0 ** -8 * max(1.0, float(np.abs(want).max())), float(np.abs(got - want).max())
    assert npc.value_spread(got) >= npc.MIN_VALUE_SPREAD, npc.value_spread(got)


@pytest.mark.parametrize("mode", [14, 15])
def test_a_trained_model(oracle, trained, mode):
    """(d) the value distribution of a real model under the bars of (a).  Measured: every frame the oracle's bit for bit in both modes (0.9984 with the
    device library's logf / sincosf: a trained grid is smooth where a random one is not)"""
    close, nv, _, _ = trained
    assert_the_renderer_alone(oracle, close, "trained", lambda: nv, mode)
