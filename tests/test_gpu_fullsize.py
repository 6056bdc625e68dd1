"""Properties at BASELINE.json's full sizes (C4: 1024^2 frame, L = 16 F = 2 T = 2^22 hash grid of a 1024^3 volume, 3 x 64 MLP), where
the oracle would take minutes: results must not depend on which copy of the table is read, on how the rays are scheduled, or on how
the image is cut into shares."""
import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn
from conftest import assert_renderer_alone

pytestmark = pytest.mark.gpu


def c4_config():
    pls = float(np.exp(np.log(1024 / 16.0) / 15))
    return syn.model_config(n_levels=16, n_features=2, log2_hashmap_size=22, n_hidden_layers=3, per_level_scale=pls)


def test_brick_image_of_the_c4_model_is_bit_identical(oracle):
    """70 M parameters, 7 hashed levels up to 1025^3 grid points: the de-hashed image is 7.15 GiB and its finest level lies beyond
    32-bit byte offsets; encode and inference must be the same bits before and after it exists, for 2 M coordinates that include
    the corners of the unit cube, and must equal the oracle on a sample of them"""
    nv = api.vnrCreateNeuralVolume(c4_config(), (1024, 1024, 1024))
    info = api.neural_info(nv)
    assert info["n_params"] == 70212496
    n_mlp = oracle.mlp_n_params(info["padded_width"], 64, 2)
    params = syn.random_params(info["n_params"], n_mlp, seed=5)
    api.neural_set_params_fp16(nv, params)
    rng = np.random.default_rng(6)
    coords = rng.uniform(0, 1, (1 << 21, 3)).astype(np.float32)
    coords[:8] = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float32)
    coords[8:16] = np.nextafter(np.float32(1), np.float32(0))
    assert not api.neural_brick_image(nv)["in_use"]
    enc0 = api.neural_encode(nv, coords).view(np.uint16)
    y0 = api.neural_inference(nv, coords).view(np.uint32)
    for _ in range(30):
        api.neural_inference(nv, coords[:256])
    st = api.neural_brick_image(nv)
    assert st["in_use"] and st["bytes"] > 7 * 2**30
    assert np.array_equal(api.neural_encode(nv, coords).view(np.uint16), enc0)
    assert np.array_equal(api.neural_inference(nv, coords).view(np.uint32), y0)
    ocfg = oracle.grid_config(16, 2, 22, 16, float(np.exp(np.log(1024 / 16.0) / 15)))
    k = 4096
    assert np.array_equal(enc0[:k], oracle.grid_encode(ocfg, params[n_mlp:].view(np.uint16), coords[:k]))
    # ... and the network OUTPUT of the T = 2^22 model on the same coordinates (the bar of tests/test_gpu_network.py: 2^-8, median 2^-11)
    want = oracle.network_inference_mt(ocfg, 64, 3, params.view(np.uint16), coords[:k])
    got = y0.view(np.float32)[:k]
    err = np.abs(got - want)
    assert err.max() <= 2.0 ** -8 * max(1.0, float(np.abs(want).max())), err.max()
    assert np.median(err) <= 2.0 ** -11


@pytest.fixture(scope="module")
def big_scene():
    vol = syn.analytic_volume(160)
    sv = api.vnrCreateSimpleVolume(vol)
    cfg = syn.model_config(n_levels=12, n_features=2, log2_hashmap_size=19, n_hidden_layers=3, per_level_scale=1.4)
    nv = api.vnrCreateNeuralVolume(cfg, sv, online_macrocell_construction=False)
    api.vnrNeuralVolumeTrain(nv, 200, True)
    colors, alphas = syn.tfn_ramp_with_bumps()
    tfn = api.vnrCreateTransferFunction()
    api.vnrTransferFunctionSetColor(tfn, colors)
    api.vnrTransferFunctionSetAlpha(tfn, alphas)
    api.vnrTransferFunctionSetValueRange(tfn, (0, 1))
    cam = syn.oblique_camera((160, 160, 160), distance_scale=0.8)
    camera = api.vnrCreateCamera()
    api.vnrCameraSet(camera, cam["from"], cam["at"], cam["up"], cam["fovy"])
    return {"nv": nv, "sv": sv, "tfn": tfn, "camera": camera}


def frame(scene, mode=5, parts=None, frames=1):
    r = api.vnrCreateRenderer(scene["nv"])
    api.vnrRendererSetTransferFunction(r, scene["tfn"])
    api.vnrRendererSetCamera(r, scene["camera"])
    api.vnrRendererSetFramebufferSize(r, (1024, 1024))
    api.vnrRendererSetMode(r, mode)
    if parts:
        api.vnrRendererSetPixelInterleave(r, 8 * 1024, parts[0], parts[1])
    for _ in range(frames):
        api.vnrRender(r)
        img = api.vnrRendererMapFrame(r).copy()
    return img


@pytest.mark.parametrize("mode", [5, 11])
def test_a_1024x1024_frame_does_not_depend_on_the_schedule(big_scene, monkeypatch, mode):
    """one stream or two, the brick image coming in between frames, 8 interleaved shares or one renderer: the same frame bit for
    bit at the full frame size; a different batch size: the same frame up to the last bits of a few samples"""
    monkeypatch.setenv("VNR_RM_N_ITERS", "24")
    ref = frame(big_scene, mode, frames=3)       # three accumulated frames: the brick image comes in along the way
    assert (ref[..., 3] > 0).mean() > 0.2
    monkeypatch.setenv("VNR_AMD_RENDER_HALVES", "1")
    assert np.array_equal(frame(big_scene, mode, frames=3), ref)
    monkeypatch.delenv("VNR_AMD_RENDER_HALVES")
    # The batch size is NOT bit-neutral in general: a ray interrupted inside a macrocell resumes at t_min + (t - t_min), which can
    # differ from t in the last bit (method_raymarching.cu:555-600 keeps `next_cell_begin = t - tMin`, and so does this code), so
    # N_ITERS moves samples by an ulp exactly as it does in the reference.  The frames agree to ~1e-4.
    monkeypatch.setenv("VNR_RM_N_ITERS", "16")
    other = frame(big_scene, mode, frames=3)
    monkeypatch.setenv("VNR_RM_N_ITERS", "24")
    err = np.abs(other - ref)
    print(f"N_ITERS 16 vs 24, mode {mode}: max |diff| {err.max():.2e}, mean {err.mean():.2e}, pixels differing {(err.max(axis=2) > 0).mean():.3f}")
    # measured: max 4.1e-5, mean 2e-9, 0.2 % of the pixels differ at all.  The single-shade heuristic (mode 11) has a discontinuity of its own: the
    # sample that shades a pixel is an ARGMAX over the ray's samples (method_raymarching.cu:789-795), and a sample moved by an ulp can hand the
    # maximum to its neighbour: one pixel at 4.8e-3 in one run of five (round 6).  A handful of such pixels is allowed, the mean is not touched.
    worst = err.max(axis=2)
    assert err.mean() < 1e-7 and int((worst > 1e-3).sum()) <= (8 if mode == 11 else 0) and worst.max() < 0.05, (float(worst.max()), int((worst > 1e-3).sum()))
    if mode == 5:
        one = frame(big_scene, mode)
        full = np.zeros_like(one)
        for part in range(8):
            share = frame(big_scene, mode, parts=(8, part))
            rows = (np.arange(1024) // 8) % 8 == part
            full[rows] = share[rows]
        assert np.array_equal(full, one)


def test_eight_unpinned_shares_of_the_1024x1024_frame_equal_the_frame_at_32(big_scene, monkeypatch):
    """what the ranks of the 8-GPU bench execute, here on one renderer per share: VNR_RM_N_ITERS unset, so a share of 131 072 pixels
    marches 32 samples per ray and iteration on 4 ray parts with the packing fused into the evaluation kernel (render.hip Renderer::render,
    render_streaming, launch_tail); the 8 shares must assemble to the unsharded frame rendered with the batch size pinned to 32"""
    monkeypatch.setenv("VNR_RM_N_ITERS", "32")
    one = frame(big_scene, 5, frames=2)
    monkeypatch.delenv("VNR_RM_N_ITERS")
    full = np.zeros_like(one)
    for part in range(8):
        share = frame(big_scene, 5, parts=(8, part), frames=2)
        rows = (np.arange(1024) // 8) % 8 == part
        full[rows] = share[rows]
    assert (one[..., 3] > 0).mean() > 0.2
    assert np.array_equal(full, one)
    # an UNSHARDED frame of a small framebuffer keeps the default batch size (24), whatever its size
    monkeypatch.setenv("VNR_RM_N_ITERS", "24")
    r = small_frame(big_scene)
    monkeypatch.delenv("VNR_RM_N_ITERS")
    assert np.array_equal(small_frame(big_scene), r)


def test_the_small_cache_tier_serves_a_train_while_render_loop_bit_for_bit(big_scene, monkeypatch):
    """the reference application's loop (apps/int_dual_volume.cpp:631-672) at a frame size whose launches qualify (capacity >= 2^20 samples): after
    every training call the frame's first launch builds the SMALL tier of the inference cache (network.h), every frame of the loop is the frame
    the same parameters give with the cache switched off, the full tier's backoff is not touched, and once the parameters are left alone the
    full image replaces the small one"""
    monkeypatch.setenv("VNR_RM_N_ITERS", "24")
    from instantvnr_amd._lib import check, lib
    nv = big_scene["nv"]
    check(lib().vnrAmdNeuralVolumeSetBrickImageMode(nv.h, -1))
    r = api.vnrCreateRenderer(nv)
    api.vnrRendererSetTransferFunction(r, big_scene["tfn"])
    api.vnrRendererSetCamera(r, big_scene["camera"])
    api.vnrRendererSetFramebufferSize(r, (1024, 1024))
    api.vnrRendererSetMode(r, 5)
    st0 = api.neural_brick_image(nv)
    for i in range(4):
        api.vnrNeuralVolumeTrain(nv, 2, False)
        api.vnrRendererResetAccumulation(r)
        api.vnrRender(r)
        got = api.vnrRendererMapFrame(r).copy()
        st = api.neural_brick_image(nv)
        assert st["tier"] == 1 and st["in_use"], st
        small_image = st
        check(lib().vnrAmdNeuralVolumeSetBrickImageMode(nv.h, 0))      # the same parameters without any cache
        api.vnrRendererResetAccumulation(r)
        api.vnrRender(r)
        want = api.vnrRendererMapFrame(r).copy()
        check(lib().vnrAmdNeuralVolumeSetBrickImageMode(nv.h, -1))
        assert not api.neural_brick_image(nv)["in_use"]
        assert (want[..., 3] > 0).mean() > 0.2 and np.array_equal(got, want), i
    st = api.neural_brick_image(nv)
    assert st["small_builds"] - st0["small_builds"] == 4 and st["builds"] == st0["builds"]
    assert st["launches_before_next_build"] == st0["launches_before_next_build"]        # small images do not move the full tier's backoff
    for _ in range(2 + st["launches_before_next_build"] // 4):
        api.vnrRender(r); api.vnrRendererMapFrame(r)
    small, st = st, api.neural_brick_image(nv)
    # every bricked level of this model fits the small budget, so the small image these frames began with IS the full one: it is promoted as
    # it stands, and `builds` counts only images whose build kernels ran (csrc/brick_policy.h)
    assert st["tier"] == 2 and st["bytes"] == small_image["bytes"] and st["levels"] == small_image["levels"], (st, small_image)
    assert st["builds"] == st0["builds"] and st["small_builds"] == small["small_builds"] + 1, st


def small_frame(scene):
    r = api.vnrCreateRenderer(scene["nv"])
    api.vnrRendererSetTransferFunction(r, scene["tfn"])
    api.vnrRendererSetCamera(r, scene["camera"])
    api.vnrRendererSetFramebufferSize(r, (256, 192))
    api.vnrRender(r)
    return api.vnrRendererMapFrame(r).copy()


@pytest.fixture(scope="module")
def c4_scene():
    """BASELINE C4 as bench.py sets it up: 1024^3 Perlin volume, the 70 M-parameter model trained on it, the bench's transfer function
    and camera"""
    import os
    os.environ["VNR_AMD_INIT_SEED"] = "20240611"
    dims = (1024, 1024, 1024)
    sv = api.vnrCreateSimpleVolumePerlin(dims, seed=42, octaves=4, base_frequency=6.0)
    nv = api.vnrCreateNeuralVolume(c4_config(), sv, online_macrocell_construction=False)
    api.vnrNeuralVolumeTrain(nv, 400, True)
    colors, alphas = syn.tfn_ramp_with_bumps(opacity_scale=0.06)
    tfn = api.vnrCreateTransferFunction()
    api.vnrTransferFunctionSetColor(tfn, colors)
    api.vnrTransferFunctionSetAlpha(tfn, alphas)
    api.vnrTransferFunctionSetValueRange(tfn, (0, 1))
    cam = syn.oblique_camera(dims, distance_scale=1.1)
    camera = api.vnrCreateCamera()
    api.vnrCameraSet(camera, cam["from"], cam["at"], cam["up"], cam["fovy"])
    return {"nv": nv, "sv": sv, "tfn": tfn, "camera": camera, "cam": cam, "colors": colors, "alphas": alphas}


@pytest.mark.parametrize("n_iters", [16, 24, 32])
def test_a_band_of_the_c4_frame_equals_the_oracle(oracle, c4_scene, monkeypatch, n_iters):
    """the frame bench.py times (1024^2 of the 1024^3 volume, trained L16 F2 T2^22 + 3x64 model, de-hashed image in use), 16 scanlines
    through its middle against the oracle's streaming marcher (method_raymarching.cu:931-958 restated) driven by the oracle's network
    on all host threads: the same rays hit, the same number of iterations, the same samples up to saturation ties, and the pixels within
    1e-3 (PSNR > 90 dB); with the library's own network values in the oracle's marcher, within 1e-5 (PSNR > 120 dB).
    At the reference's batch size (N_ITERS 16, method_raymarching.cu:30-40), at the one bench.py runs (24) and at the one a rank's small share
    takes (32), and rendered the way bench.py renders: through vnrAmdRendererRenderPipelined (frame 1 is completed while the head of frame 2 is
    already enqueued).  (A band of 16 384 rays runs the decoupled loop: renderer.h decoupled_mode_; the share test below runs the coupled one.)"""
    from instantvnr_amd import dist
    monkeypatch.setenv("VNR_RM_N_ITERS", str(n_iters))    # read when a renderer is created
    nv = c4_scene["nv"]
    warm = frame(c4_scene, 5, frames=3)           # 3 frames x 2 ray parts x ~9 launches: the image is built along the way
    st_img = api.neural_brick_image(nv)
    assert st_img["in_use"] and st_img["bytes"] > 7 * 2**30
    assert (warm[..., 3] > 0).mean() > 0.4
    lo, hi = 504 * 1024, 520 * 1024
    r = api.vnrCreateRenderer(nv)
    api.vnrRendererSetTransferFunction(r, c4_scene["tfn"])
    api.vnrRendererSetCamera(r, c4_scene["camera"])
    api.vnrRendererSetFramebufferSize(r, (1024, 1024))
    api.vnrRendererSetMode(r, 5)
    api.vnrRendererSetPixelRange(r, lo, hi)
    sr = dist.ShardedRenderer(dist.Context(0, 1, 0, None), r, 1024, 1024)
    assert sr.render() is None                     # frame 1 enqueued
    first = sr.render()                            # frame 2 enqueued, frame 1 completed and handed out
    band = sr.download(first).reshape(-1, 4)[lo:hi].copy()
    st = sr.completed_stats()
    second = sr.download(sr.flush()).reshape(-1, 4)[lo:hi].copy()
    one = frame(c4_scene, 5)
    assert np.array_equal(band, one.reshape(-1, 4)[lo:hi])          # the band is the whole frame's pixels
    two = frame(c4_scene, 5, frames=2)                               # and the pipelined second frame is the plain second frame
    assert np.array_equal(second, two.reshape(-1, 4)[lo:hi]) and not np.array_equal(second, band)
    params = api.neural_get_params_fp16(nv).view(np.uint16)
    pls = float(np.exp(np.log(1024 / 16.0) / 15))
    ocfg = oracle.grid_config(16, 2, 22, 16, pls)
    mo = api.volume_macrocell(nv)["max_opacity"]
    cam = c4_scene["cam"]
    sc = oracle.SceneHolder(1024, 1024, (1024, 1024, 1024), oracle.TfnHolder(c4_scene["colors"], c4_scene["alphas"]), mo, cam["from"], cam["at"],
                            cam["up"], cam["fovy"], pixel_range=(lo, hi))
    import time
    t0 = time.perf_counter()
    ref, _, ost = oracle.render_streaming(sc, lambda c: oracle.network_inference_mt(ocfg, 64, 3, params, c), n_iters=n_iters)
    dt = time.perf_counter() - t0
    ref = ref.reshape(-1, 4)[lo:hi]
    err = np.abs(band - ref)
    psnr = 10 * np.log10(1.0 / float((err ** 2).mean()))
    print(f"\nC4 band of 16 scanlines, N_ITERS {n_iters}, pipelined: oracle {dt:.1f} s for {ost['n_slots']} slots; rays hit {st['n_rays_hit']}, "
          f"iterations {st['n_iterations']}, samples {st['n_samples']} (oracle {ost['n_samples']}), PSNR {psnr:.1f} dB, max |err| {err.max():.4f}")
    assert ost["n_rays_hit"] == st["n_rays_hit"] and ost["n_iterations"] == st["n_iterations"]
    assert abs(ost["n_samples"] - st["n_samples"]) <= 0.002 * ost["n_samples"]
    assert api.renderer_schedule(r)["n_iters"] == n_iters
    assert (ref[:, 3] > 0).mean() > 0.4
    assert psnr > 90.0, psnr           # measured 113.9 dB, max 1.0e-4 at 16 (round 2's bar for neural frames, 45 dB / 0.05, was set on random parameters)
    assert err.max() < 1e-3
    # the same band with the oracle's marcher fed by the LIBRARY's network values at the oracle's sample positions: what is left is the
    # renderer alone (ray generation, DDA, adaptive steps, classification, blending), at the bar of the ground-truth frames
    ref2, _, ost2 = oracle.render_streaming(sc, lambda c: api.neural_inference(nv, c), n_iters=n_iters)
    err2 = np.abs(band - ref2.reshape(-1, 4)[lo:hi])
    psnr2 = 10 * np.log10(1.0 / max(float((err2 ** 2).mean()), 1e-30))
    print(f"   compositor alone (oracle marcher on the library's network values): PSNR {psnr2:.1f} dB, max |err| {err2.max():.2e}, samples {ost2['n_samples']}")
    assert ost2["n_rays_hit"] == st["n_rays_hit"] and ost2["n_iterations"] == st["n_iterations"]
    assert psnr2 > 120.0, psnr2                          # measured 145.0 dB, max 5.4e-7 at 16
    assert_renderer_alone(err2, 2, "band")


@pytest.mark.parametrize("part", [3])
def test_a_rank_s_share_of_the_c4_frame_equals_the_oracle(oracle, c4_scene, monkeypatch, part):
    """the code path a rank of the 8-GPU run executes, against the oracle and not against the library's own frame.
    VNR_RM_N_ITERS is NOT set (the suite pins 16: tests/conftest.py), the renderer gets the interleaved 1/8 share of the bench frame
    (131 072 pixels in 8-scanline tile rows, global pixel indices kept), so it marches 32 samples per ray and iteration on three ray parts with
    the survivors' packing fused into the evaluation kernel (render.hip Renderer::render / render_streaming / launch_tail) -- asserted from the
    library's own record of the schedule.  The oracle renders the same pixel set with the reference's loop (method_raymarching.cu:931-958; batch
    size :30-40 set to 32; resume rule :555-600) driven by the oracle's network.  Same bars as the band test: rays hit and iterations equal, samples
    within 0.2 %, PSNR > 90 dB / 1e-3; with the library's network values in the oracle's marcher PSNR > 120 dB / 1e-5."""
    import time
    monkeypatch.delenv("VNR_RM_N_ITERS", raising=False)
    for k in ("VNR_AMD_SMALL_SHARE_PARTS", "VNR_AMD_RENDER_HALVES", "VNR_AMD_DECOUPLED"):
        monkeypatch.delenv(k, raising=False)
    nv = c4_scene["nv"]
    frame(c4_scene, 5, frames=3)                     # the de-hashed image is in use, as in the bench
    assert api.neural_brick_image(nv)["in_use"]
    block, parts = 8 * 1024, 8
    r = api.vnrCreateRenderer(nv)
    api.vnrRendererSetTransferFunction(r, c4_scene["tfn"])
    api.vnrRendererSetCamera(r, c4_scene["camera"])
    api.vnrRendererSetFramebufferSize(r, (1024, 1024))
    api.vnrRendererSetMode(r, 5)
    api.vnrRendererSetPixelInterleave(r, block, parts, part)
    api.vnrRender(r)
    img = api.vnrRendererMapFrame(r).reshape(-1, 4).copy()
    st = api.vnrRendererGetFrameStats(r)
    sched = api.renderer_schedule(r)
    assert sched == {"n_iters": 32, "n_parts": 3, "fused_pack": True, "decoupled": False}, sched
    mine = (np.arange(1024 * 1024) // block) % parts == part
    share = img[mine]
    params = api.neural_get_params_fp16(nv).view(np.uint16)
    ocfg = oracle.grid_config(16, 2, 22, 16, float(np.exp(np.log(1024 / 16.0) / 15)))
    mo = api.volume_macrocell(nv)["max_opacity"]
    cam = c4_scene["cam"]
    sc = oracle.SceneHolder(1024, 1024, (1024, 1024, 1024), oracle.TfnHolder(c4_scene["colors"], c4_scene["alphas"]), mo, cam["from"], cam["at"],
                            cam["up"], cam["fovy"], interleave=(block, parts, part))
    t0 = time.perf_counter()
    ref, _, ost = oracle.render_streaming(sc, lambda c: oracle.network_inference_mt(ocfg, 64, 3, params, c), n_iters=32)
    dt = time.perf_counter() - t0
    ref = ref.reshape(-1, 4)
    assert not ref[~mine].any()                      # the oracle rendered this rank's pixels and no others
    err = np.abs(share - ref[mine])
    psnr = 10 * np.log10(1.0 / float((err ** 2).mean()))
    print(f"\nC4 share {part} of 8 (131 072 pixels), N_ITERS 32 by the library's own rule, {sched['n_parts']} parts, fused packing: oracle {dt:.1f} s for "
          f"{ost['n_slots']} slots; rays hit {st['n_rays_hit']}, iterations {st['n_iterations']}, samples {st['n_samples']} (oracle {ost['n_samples']}), "
          f"reference slots {st['n_reference_slots']} (oracle {ost['n_slots']}), PSNR {psnr:.1f} dB, max |err| {err.max():.2e}")
    assert ost["n_rays_hit"] == st["n_rays_hit"] > 40000 and ost["n_iterations"] == st["n_iterations"]
    assert abs(ost["n_samples"] - st["n_samples"]) <= 0.002 * ost["n_samples"]
    assert (ref[mine][:, 3] > 0).mean() > 0.3
    assert psnr > 90.0 and err.max() < 1e-3, (psnr, float(err.max()))
    ref2, _, ost2 = oracle.render_streaming(sc, lambda c: api.neural_inference(nv, c), n_iters=32)
    err2 = np.abs(share - ref2.reshape(-1, 4)[mine])
    psnr2 = 10 * np.log10(1.0 / max(float((err2 ** 2).mean()), 1e-30))
    print(f"   compositor alone (oracle marcher on the library's network values): PSNR {psnr2:.1f} dB, max |err| {err2.max():.2e}")
    assert ost2["n_rays_hit"] == st["n_rays_hit"] and ost2["n_iterations"] == st["n_iterations"]
    assert psnr2 > 120.0, psnr2                          # measured 146.5 dB, max 6e-7; with one saturation tie 138.8 dB, max 4.6e-5
    assert_renderer_alone(err2, 8, "share")
    # the share in distributed mode's clothing is the same pixels: the whole frame at 32 holds them bit for bit
    monkeypatch.setenv("VNR_RM_N_ITERS", "32")
    whole = frame(c4_scene, 5).reshape(-1, 4)
    assert np.array_equal(whole[mine], share)


def test_gradients_of_the_c4_model_match_the_restatement(oracle):
    """the training step's backward pass on the FULL model (70 M parameters: hashed levels of 2^22 entries, packed fp16 atomics at byte
    offsets up to 140 MB into the gradient blob) against the numpy restatement on a batch the restatement can afford: same bars as the
    small shapes of tests/test_gpu_train.py, plus: no gradient lands outside the entries the batch touches"""
    from oracle import train_oracle as T
    nv = api.vnrCreateNeuralVolume(c4_config(), (1024, 1024, 1024))
    info = api.neural_info(nv)
    n_mlp = oracle.mlp_n_params(info["padded_width"], 64, 2)
    params = syn.random_params(info["n_params"], n_mlp, seed=9)
    api.neural_set_params_fp16(nv, params)
    rng = np.random.default_rng(10)
    B = 2000
    coords = rng.uniform(0, 1, (B, 3)).astype(np.float32)
    targets = rng.uniform(0, 1, B).astype(np.float32)
    got = api.neural_forward_backward(nv, coords, targets).astype(np.float64)
    ocfg = oracle.grid_config(16, 2, 22, 16, float(np.exp(np.log(1024 / 16.0) / 15)))
    ref = T.training_gradients(ocfg, 64, 3, params.view(np.uint16), coords, targets, loss="L1")
    want = ref["grads"]
    assert got.shape == want.shape == (70212496,)
    assert np.isclose(api.vnrNeuralVolumeGetTrainingLoss(nv), ref["loss"], rtol=2e-3)
    for name, sl in [("mlp", slice(0, n_mlp)), ("grid", slice(n_mlp, None))]:
        g, w = got[sl], want[sl]
        rel = np.linalg.norm(g - w) / np.linalg.norm(w)
        assert rel < 3e-2, (name, rel)
        assert np.abs(g - w).max() < 6e-2 * np.abs(w).max(), name
    touched = want[n_mlp:] != 0
    assert 0 < touched.sum() <= B * 16 * 8 * 2
    # an entry the batch does not touch has no gradient (a stray atomic would show here), an entry it touches nearly always has one
    assert np.count_nonzero(got[n_mlp:][~touched]) == 0
    assert np.count_nonzero(got[n_mlp:][touched]) > 0.98 * touched.sum()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_bands_of_the_c4_frame_from_random_cameras_equal_the_oracle(oracle, c4_scene, monkeypatch, seed):
    """the band test above from other places: a camera anywhere around the 1024^3 volume (direction, distance 0.7..1.6 of the bench's, field of
    view 30..60), eight scanlines at a random height: rays hit and iterations equal the oracle's, pixels within 1e-3 (PSNR > 85 dB) of the
    oracle's marcher driven by the oracle's network, within 1e-5 of it driven by the library's network values"""
    rng = np.random.default_rng(1000 + seed)
    monkeypatch.setenv("VNR_RM_N_ITERS", "24")        # read when a renderer is created (a small pixel range would otherwise take 32)
    nv = c4_scene["nv"]
    v = rng.normal(size=3); v /= np.linalg.norm(v)
    if abs(v[1]) > 0.9:
        v = np.array([0.5, 0.4, -0.77]); v /= np.linalg.norm(v)
    base = np.linalg.norm(c4_scene["cam"]["from"])
    frm = tuple(float(x) for x in v * base * rng.uniform(0.7, 1.6))
    fovy = float(rng.uniform(30, 60))
    camera = api.vnrCreateCamera()
    api.vnrCameraSet(camera, frm, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), fovy)
    row = int(rng.integers(300, 716))
    lo, hi = row * 1024, (row + 8) * 1024
    r = api.vnrCreateRenderer(nv)
    api.vnrRendererSetTransferFunction(r, c4_scene["tfn"])
    api.vnrRendererSetCamera(r, camera)
    api.vnrRendererSetFramebufferSize(r, (1024, 1024))
    api.vnrRendererSetMode(r, 5)
    api.vnrRendererSetPixelRange(r, lo, hi)
    api.vnrRender(r)
    band = api.vnrRendererMapFrame(r).reshape(-1, 4)[lo:hi].copy()
    st = api.vnrRendererGetFrameStats(r)
    params = api.neural_get_params_fp16(nv).view(np.uint16)
    ocfg = oracle.grid_config(16, 2, 22, 16, float(np.exp(np.log(1024 / 16.0) / 15)))
    mo = api.volume_macrocell(nv)["max_opacity"]
    sc = oracle.SceneHolder(1024, 1024, (1024, 1024, 1024), oracle.TfnHolder(c4_scene["colors"], c4_scene["alphas"]), mo, frm, (0, 0, 0), (0, 1, 0), fovy,
                            pixel_range=(lo, hi))
    n_iters = 24      # the frame does not depend on it, the iteration count does
    ref, _, ost = oracle.render_streaming(sc, lambda c: oracle.network_inference_mt(ocfg, 64, 3, params, c), n_iters=n_iters)
    ref = ref.reshape(-1, 4)[lo:hi]
    err = np.abs(band - ref)
    psnr = 10 * np.log10(1.0 / max(float((err ** 2).mean()), 1e-20))
    print(f"\ncamera {seed}: from {tuple(round(x) for x in frm)}, fovy {fovy:.0f}, rows {row}..{row + 8}: rays hit {st['n_rays_hit']}, max err {err.max():.2e}, PSNR {psnr:.1f} dB")
    assert st["n_rays_hit"] == ost["n_rays_hit"] > 2000
    assert st["n_iterations"] == ost["n_iterations"]
    assert (ref[:, 3] > 0).mean() > 0.2
    assert err.max() < 1e-3 and psnr > 85.0
    mine, _, _ = oracle.render_streaming(sc, lambda c: api.neural_inference(nv, c), n_iters=n_iters)
    assert_renderer_alone(np.abs(band - mine.reshape(-1, 4)[lo:hi]), 2, "random camera")


def test_adam_step_of_the_c4_model_matches_the_restatement(oracle):
    """one optimizer step on the full model: touched parameters move like the restated Adam (2^-10), the 99 % of the 70 M parameters a
    2000-sample batch does not touch keep their bits, the gradient blob is clear afterwards, and a second step on other samples
    updates per-parameter step counts independently (an entry touched for the first time in step 2 takes a FIRST step)"""
    from oracle import train_oracle as T
    nv = api.vnrCreateNeuralVolume(c4_config(), (1024, 1024, 1024))
    info = api.neural_info(nv)
    n_mlp = oracle.mlp_n_params(info["padded_width"], 64, 2)
    params = syn.random_params(info["n_params"], n_mlp, seed=11)
    api.neural_set_params_fp16(nv, params)
    rng = np.random.default_rng(12)
    master = params.astype(np.float64)
    m = np.zeros_like(master); v = np.zeros_like(master); steps = np.zeros_like(master)
    for step in range(2):
        coords = rng.uniform(0, 1, (2000, 3)).astype(np.float32)
        targets = rng.uniform(0, 1, 2000).astype(np.float32)
        before = api.neural_get_params_fp16(nv).astype(np.float64)
        grads = api.neural_forward_backward(nv, coords, targets).astype(np.float64)
        api.neural_train_end(nv)
        after = api.neural_get_params_fp16(nv).astype(np.float64)
        master, m, v, steps = T.adam_step(master, grads, m, v, steps, n_mlp)[:4]
        want = master.astype(np.float32).astype(np.float16).astype(np.float64)
        touched = grads != 0
        assert 0.001 < touched[n_mlp:].mean() < 0.02
        assert np.array_equal(after[n_mlp:][~touched[n_mlp:]], before[n_mlp:][~touched[n_mlp:]])
        d = np.abs(after - want)[touched]
        assert np.quantile(d, 0.999) <= 2.0 ** -10 * np.maximum(1.0, np.abs(want)).max(), (step, np.quantile(d, 0.999))
        assert np.all(api.neural_gradients(nv) == 0)
    assert api.vnrNeuralVolumeGetTrainingStep(nv) == 2
    assert set(np.unique(steps[n_mlp:])) == {0.0, 1.0, 2.0}     # entries untouched, touched once, touched in both steps


@pytest.mark.parametrize("n_iters", ["16", "24"])
def test_two_ranks_render_the_c4_frame_like_one(n_iters, tmp_path):
    """BASELINE C4 as it is sharded (tests/dist_gpu_worker.py::scenario_frames_c4; both ranks on this box's one GPU, host-staged
    collectives), at the reference's N_ITERS and at the library's: every frame assembled from the ranks' pipelined shares is the
    unsharded frame bit for bit, with the de-hashed image (finest level beyond 4 GiB) in use on every rank"""
    from test_gpu_dist import run_ranks
    res = run_ranks("frames_c4", 2, tmp_path, extra_env={"VNR_RM_N_ITERS": n_iters}, timeout=600)
    for r in res:
        assert bool(r["brick_in_use"]) and float(r["coverage"]) > 0.3 and int(r["samples"]) > 5_000_000
        assert bool(np.all(r["equal"])), (int(r["rank"]), r["equal"], float(r["max_diff"]), float(r["differing_pixels"]))


def test_two_ranks_train_the_c4_model_data_parallel(tmp_path):
    """the gradient exchange at the full model size (tests/dist_gpu_worker.py::scenario_train_c4): 70 212 496 parameters, ranks that start
    from different seeds hold identical parameters after the first call and after 40 steps, and the loss falls"""
    from test_gpu_dist import run_ranks
    res = run_ranks("train_c4", 2, tmp_path, timeout=600)
    a, b = res
    assert int(a["n_params"]) == 70212496 and int(a["step"]) == 40 and int(b["step"]) == 40
    assert int(a["checksum_before"]) != int(b["checksum_before"])
    assert int(a["checksum_2"]) == int(b["checksum_2"]) and int(a["checksum_40"]) == int(b["checksum_40"])
    assert int(a["checksum_40"]) != int(a["checksum_2"])
    assert float(a["loss_last"]) < 0.5 * float(a["loss_first"]), (float(a["loss_first"]), float(a["loss_last"]))
