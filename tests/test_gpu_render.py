"""GPU parity of the march path (through the C-ABI): ground-truth sampling, macrocells, the sample-streaming
renderer (mode 5) on a dense volume and on a neural volume, the monolithic marcher (mode 4), and tiles."""
import os
import sys

import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neural_pt_cases as npc  # noqa: E402

pytestmark = pytest.mark.gpu


def psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 99.0 if mse == 0 else 10 * np.log10(1.0 / mse)


@pytest.fixture(scope="module")
def scene(oracle):
    vol = syn.analytic_volume(48)
    colors, alphas = syn.tfn_ramp_with_bumps()
    sv = api.vnrCreateSimpleVolume(vol)
    tfn = api.vnrCreateTransferFunction()
    api.vnrTransferFunctionSetColor(tfn, colors)
    api.vnrTransferFunctionSetAlpha(tfn, alphas)
    api.vnrTransferFunctionSetValueRange(tfn, (0, 1))
    cam = syn.oblique_camera((48, 48, 48))
    camera = api.vnrCreateCamera()
    api.vnrCameraSet(camera, cam["from"], cam["at"], cam["up"], cam["fovy"])
    otfn = oracle.TfnHolder(colors, alphas)
    return {"vol": vol, "sv": sv, "tfn": tfn, "camera": camera, "cam": cam, "otfn": otfn}


def make_renderer(scene, volume, size=(96, 80), mode=5):
    r = api.vnrCreateRenderer(volume)
    api.vnrRendererSetTransferFunction(r, scene["tfn"])
    api.vnrRendererSetCamera(r, scene["camera"])
    api.vnrRendererSetFramebufferSize(r, size)
    api.vnrRendererSetMode(r, mode)
    return r


def oracle_scene(oracle, scene, mo, size=(96, 80), dims=(48, 48, 48)):
    cam = scene["cam"]
    return oracle.SceneHolder(size[0], size[1], dims, scene["otfn"], mo, cam["from"], cam["at"], cam["up"], cam["fovy"])


def test_trilinear_sampling_bit_exact(oracle, scene):
    rng = np.random.default_rng(0)
    c = rng.uniform(-0.05, 1.05, (5000, 3)).astype(np.float32)
    for nodal in (False, True):
        got = api.simple_volume_sample(scene["sv"], c, nodal)
        want = oracle.sample_volume(scene["vol"], c, nodal)
        assert np.array_equal(got, want)


def test_take_samples_are_uniform_and_consistent(oracle, scene):
    c, v = api.simple_volume_take_samples(scene["sv"], 65536)
    assert c.min() >= 0 and c.max() < 1
    assert abs(c.mean() - 0.5) < 0.01 and abs(c.std() - np.sqrt(1 / 12)) < 0.01
    assert np.array_equal(v, oracle.sample_volume(scene["vol"], c, nodal=False))
    c2, _ = api.simple_volume_take_samples(scene["sv"], 1024)
    assert not np.array_equal(c[:1024], c2)   # the stream advances between calls


def test_take_samples_follow_the_pcg32_stream_call_after_call(oracle):
    """StaticSampler::take_samples (neural_sampler.cu:130-164): p = lower + u (upper - lower) with u the next three floats of pcg32(seed
    1337, tcnn's default sequence); ragged batch sizes, a sub-box, a ragged volume: coordinates and values bit for bit, and the stream
    goes on where the last call stopped"""
    rng = np.random.default_rng(4)
    vol = rng.uniform(0, 1, (19, 37, 50)).astype(np.float32)
    lo_, hi_ = np.float32(vol.min()), np.float32(vol.max())
    norm = np.clip((vol - lo_) / (hi_ - lo_), np.float32(0), np.float32(1)).astype(np.float32)
    sv = api.vnrCreateSimpleVolume(vol)
    offset = 0
    for n, lower, upper in [(1000, (0, 0, 0), (1, 1, 1)), (1, (0, 0, 0), (1, 1, 1)), (4097, (0.1, 0.2, 0.3), (0.9, 0.5, 0.31)), (63, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))]:
        c, v = api.simple_volume_take_samples(sv, n, lower, upper)
        u = oracle.pcg32_floats(3 * n, offset, 1337, 0xda3e39cb94b95bdb).reshape(n, 3)
        lo, hi = np.array(lower, np.float32), np.array(upper, np.float32)
        want = (lo + u * (hi - lo)).astype(np.float32)
        assert np.array_equal(c, want), (n, offset)
        assert np.array_equal(v, oracle.sample_volume(norm, c, nodal=False))
        offset += 3 * n


def test_macrocell_bit_exact(oracle, scene):
    mc = api.volume_macrocell(scene["sv"])
    vr = oracle.macrocell_compute_implicit(scene["vol"])
    assert mc["dims"] == (3, 3, 3)
    assert np.array_equal(mc["value_range"], vr)
    api.lib().vnrAmdVolumeUpdateMaxOpacity(scene["sv"].h, scene["tfn"].h)
    mc = api.volume_macrocell(scene["sv"])
    assert np.array_equal(mc["max_opacity"], oracle.macrocell_max_opacity(scene["otfn"], vr))


def test_streaming_groundtruth_matches_oracle(oracle, scene):
    r = make_renderer(scene, scene["sv"])
    api.vnrRender(r)
    img = api.vnrRendererMapFrame(r).copy()
    st = api.vnrRendererGetFrameStats(r)
    mo = api.volume_macrocell(scene["sv"])["max_opacity"]
    sc = oracle_scene(oracle, scene, mo)
    want, _, ost = oracle.render_streaming(sc, lambda c: oracle.sample_volume(scene["vol"], c, nodal=True))
    assert st["n_rays_hit"] == ost["n_rays_hit"] > 1000
    assert st["n_iterations"] == ost["n_iterations"]
    # identical arithmetic except powf (device libm vs glibc): per-pixel error ~1e-6
    assert np.abs(img - want).max() < 2e-4, np.abs(img - want).max()
    assert psnr(img, want) > 80
    # the oracle counts samples emitted by the reference's intersect pass; sample compaction never infers more
    assert st["n_samples"] <= ost["n_samples"] <= st["n_reference_slots"] == ost["n_slots"]
    assert st["n_samples"] > 0.5 * ost["n_samples"]


@pytest.mark.parametrize("n_colors,n_alphas", [(256, 256), (64, 100), (300, 17)])
def test_transfer_function_tables_of_equal_and_of_different_lengths(oracle, scene, n_colors, n_alphas):
    """the compose kernels keep the tables in LDS; when the colour and the opacity table have the same length the opacities ride in the colour
    table's 4th component and a sample takes one index computation and one pair of reads (sampling_device.h tfn_sample_lds `merged`), else
    two of each: the same frame as the oracle's either way, for the coupled and the decoupled loop"""
    colors, _ = syn.tfn_ramp_with_bumps(n=n_colors)
    _, alphas = syn.tfn_ramp_with_bumps(n=n_alphas)
    tfn = api.vnrCreateTransferFunction()
    api.vnrTransferFunctionSetColor(tfn, colors)
    api.vnrTransferFunctionSetAlpha(tfn, alphas)
    api.vnrTransferFunctionSetValueRange(tfn, (0, 1))
    mo = None
    for size in ((96, 80), (200, 144)):   # (the small frame takes the decoupled loop)
        r = api.vnrCreateRenderer(scene["sv"])
        api.vnrRendererSetTransferFunction(r, tfn)
        api.vnrRendererSetCamera(r, scene["camera"])
        api.vnrRendererSetFramebufferSize(r, size)
        api.vnrRender(r)
        img = api.vnrRendererMapFrame(r).copy()
        if mo is None:
            mo = api.volume_macrocell(scene["sv"])["max_opacity"]
        cam = scene["cam"]
        sc = oracle.SceneHolder(size[0], size[1], (48, 48, 48), oracle.TfnHolder(colors, alphas), mo, cam["from"], cam["at"], cam["up"], cam["fovy"])
        want, _, _ = oracle.render_streaming(sc, lambda c: oracle.sample_volume(scene["vol"], c, nodal=True))
        assert (img[..., 3] > 0).mean() > 0.02
        assert np.abs(img - want).max() < 2e-4, (size, float(np.abs(img - want).max()))


def test_frames_do_not_depend_on_n_iters_or_tile_shape(scene, monkeypatch):
    """the batch size of the streaming loop (VNR_RM_N_ITERS; library default 24, reference default 16) and the shape of the ray
    tiles are scheduling choices.  On this scene the frames are the same bit for bit; in general the batch size moves a sample
    by an ulp where a ray is interrupted inside a macrocell (it resumes at t_min + (t - t_min), as in the reference), which
    tests/test_gpu_fullsize.py measures at 1024 x 1024: max 4e-5, 0.2 % of the pixels"""
    frames = []
    for n_iters, tile_w in (("16", "8"), ("24", "8"), ("5", "8"), ("16", "32"), ("24", "16"), ("16", "64")):
        monkeypatch.setenv("VNR_RM_N_ITERS", n_iters)
        monkeypatch.setenv("VNR_AMD_TILE_W", tile_w)
        r = make_renderer(scene, scene["sv"])
        api.vnrRender(r)
        frames.append(api.vnrRendererMapFrame(r).copy())
    for f in frames[1:]:
        assert np.array_equal(f, frames[0])


@pytest.fixture(scope="module")
def small_network(scene):
    import os
    os.environ["VNR_AMD_INIT_SEED"] = "515"
    nv = api.vnrCreateNeuralVolume(syn.model_config(n_levels=6, n_features=2, log2_hashmap_size=14, base_resolution=4, n_hidden_layers=2),
                                   scene["sv"], online_macrocell_construction=False)
    api.vnrNeuralVolumeTrain(nv, 60, True)
    return nv


@pytest.mark.parametrize("volume_kind", ["dense", "neural"])
def test_decoupled_walks_give_the_coupled_loop_s_frames_and_statistics(scene, small_network, monkeypatch, volume_kind):
    """csrc/decoupled.h: walk / evaluate / compose as three kernels on three streams with the walks up to A batches ahead of the
    composes, against march_kernel's loop (walk, evaluate, compose in turn): the same frames bit for bit over accumulated frames (the
    per-ray arithmetic and its order are the same; a saturated ray's batches emitted ahead are evaluated and dropped), the same
    statistics (samples are counted where a ray was alive when it emitted them), for every look-ahead and number of ray parts, through
    the synchronous and the pipelined calls, with a transfer function opaque enough that most rays saturate early"""
    from instantvnr_amd._lib import check, lib
    import ctypes as C
    volume = scene["sv"] if volume_kind == "dense" else small_network
    colors, alphas = syn.tfn_ramp_with_bumps(opacity_scale=3.0)
    opaque = api.vnrCreateTransferFunction()
    api.vnrTransferFunctionSetColor(opaque, colors)
    api.vnrTransferFunctionSetAlpha(opaque, alphas)
    api.vnrTransferFunctionSetValueRange(opaque, (0, 1))
    size = (200, 144)
    n_frames = 3

    def run(tfn, pipelined):
        r = api.vnrCreateRenderer(volume)
        api.vnrRendererSetTransferFunction(r, tfn)
        api.vnrRendererSetCamera(r, scene["camera"])
        api.vnrRendererSetFramebufferSize(r, size)
        frames, stats = [], []
        if not pipelined:
            for _ in range(n_frames):
                api.vnrRender(r)
                frames.append(api.vnrRendererMapFrame(r).copy())
                stats.append(api.vnrRendererGetFrameStats(r))
            return frames, stats
        api.vnrRendererSetOutputAsDeviceFramebuffer(r, True)
        out = C.c_void_p()
        n = size[0] * size[1]

        def grab(ptr):
            a = np.empty((size[1], size[0], 4), np.float32)
            check(lib().vnrAmdMemcpyD2H(a.ctypes.data_as(C.c_void_p), ptr, a.nbytes))
            return a
        for k in range(n_frames):
            check(lib().vnrAmdRendererRenderPipelined(r.h, C.byref(out)))
            if k:
                frames.append(grab(out))
        check(lib().vnrAmdRendererFlushPipeline(r.h, C.byref(out)))
        frames.append(grab(out))
        return frames, [api.vnrRendererGetFrameStats(r)]

    keys = ("n_samples", "n_reference_slots", "n_iterations", "n_rays_hit")
    for tfn in (scene["tfn"], opaque):
        monkeypatch.setenv("VNR_AMD_DECOUPLED", "0")
        want, want_stats = run(tfn, False)
        assert want_stats[0]["n_iterations"] >= 2 and want_stats[0]["n_samples"] > 10000
        for ahead, parts in (("1", "1"), ("2", "2"), ("2", "1"), ("3", "4"), ("5", "2"), ("3", "1")):
            monkeypatch.setenv("VNR_AMD_DECOUPLED", "2")
            monkeypatch.setenv("VNR_AMD_DECOUPLED_AHEAD", ahead)
            monkeypatch.setenv("VNR_AMD_DECOUPLED_PARTS", parts)
            got, got_stats = run(tfn, False)
            for k in range(n_frames):
                assert np.array_equal(got[k], want[k]), (volume_kind, ahead, parts, k, float(np.abs(got[k] - want[k]).max()))
                assert {q: got_stats[k][q] for q in keys} == {q: want_stats[k][q] for q in keys}, (ahead, parts, k)
            piped, piped_stats = run(tfn, True)
            for k in range(n_frames):
                assert np.array_equal(piped[k], want[k]), (volume_kind, ahead, parts, k, "pipelined")
            assert {q: piped_stats[0][q] for q in keys} == {q: want_stats[-1][q] for q in keys}


def test_decoupled_walk_at_every_batch_size(scene, monkeypatch):
    """the decoupled loop (walk_kernel / compose_kernel on streams of their own, csrc/decoupled.h) cuts a ray's batch where the sample count
    reaches VNR_RM_N_ITERS: inside a cell or at a cell's last sample.  Small and odd batch sizes put the cut everywhere; frames and
    statistics equal the coupled loop's at the same batch size, bit for bit"""
    keys = ("n_samples", "n_reference_slots", "n_iterations", "n_rays_hit")
    for n_iters in ("1", "3", "5", "8", "16", "17", "32", "40"):
        monkeypatch.setenv("VNR_RM_N_ITERS", n_iters)
        out = []
        for mode in ("0", "2"):
            monkeypatch.setenv("VNR_AMD_DECOUPLED", mode)
            r = make_renderer(scene, scene["sv"])
            api.vnrRender(r)
            out.append((api.vnrRendererMapFrame(r).copy(), api.vnrRendererGetFrameStats(r)))
        for frame, st in out[1:]:
            assert np.array_equal(frame, out[0][0]), (n_iters, float(np.abs(frame - out[0][0]).max()))
            assert {q: st[q] for q in keys} == {q: out[0][1][q] for q in keys}, n_iters


def test_accumulation_over_frames(oracle, scene):
    r = make_renderer(scene, scene["sv"])
    mo = api.volume_macrocell(scene["sv"])["max_opacity"]
    sc = oracle_scene(oracle, scene, mo)
    f = lambda c: oracle.sample_volume(scene["vol"], c, nodal=True)
    acc = None
    for frame in (1, 2, 3):
        api.vnrRender(r)
        img = api.vnrRendererMapFrame(r).copy()
        sc.c.frame_index = frame
        want, acc, _ = oracle.render_streaming(sc, f, accumulation=acc)
        assert np.abs(img - want).max() < 3e-4
    api.vnrRendererResetAccumulation(r)
    api.vnrRender(r)
    img = api.vnrRendererMapFrame(r).copy()
    sc.c.frame_index = 1
    want, _, _ = oracle.render_streaming(sc, f)
    assert np.abs(img - want).max() < 2e-4


def test_tiles_compose_exactly(scene):
    r = make_renderer(scene, scene["sv"])
    api.vnrRender(r)
    full = api.vnrRendererMapFrame(r).copy()
    n = full.shape[0] * full.shape[1]
    out = np.zeros((n, 4), np.float32)
    for lo, hi in [(0, 1000), (1000, 5000), (5000, n)]:
        api.vnrRendererSetPixelRange(r, lo, hi)
        api.vnrRender(r)
        out[lo:hi] = api.vnrRendererMapFrame(r).reshape(-1, 4)[lo:hi]
    assert np.array_equal(out.reshape(full.shape), full)


def test_monolithic_mode4_matches_oracle(oracle, scene):
    r = make_renderer(scene, scene["sv"], mode=4)
    api.vnrRender(r)
    img = api.vnrRendererMapFrame(r).copy()
    mo = api.volume_macrocell(scene["sv"])["max_opacity"]
    want, _ = oracle.render_monolithic(oracle_scene(oracle, scene, mo), scene["vol"])
    assert np.abs(img - want).max() < 2e-4
    assert psnr(img, want) > 80


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 16, -1])
def test_unsupported_modes_fail_loudly(scene, mode):
    """the OptiX modes (0-3) are not built and there is nothing beyond 15: no silent fallback"""
    r = make_renderer(scene, scene["sv"], mode=mode)
    with pytest.raises(api.VnrAmdError, match="not implemented"):
        api.vnrRender(r)


def test_the_denoiser_flag_is_accepted_with_a_warning_or_refused_on_request(scene, monkeypatch, capfd):
    """vnrRendererSetDenoiser (api.cpp:466): the reference's is OptiX's trained denoiser, which has no counterpart here.  One behaviour: the
    call is accepted (the reference's GUI apps make it from a checkbox; an unchanged app must not die there), switching it ON says once on
    stderr that frames stay undenoised, and the frame is the frame without the flag; VNR_AMD_DENOISER_STRICT=1 refuses instead"""
    r = make_renderer(scene, scene["sv"])
    api.vnrRender(r)
    plain = api.vnrRendererMapFrame(r).copy()
    r2 = make_renderer(scene, scene["sv"])
    api.vnrRendererSetDenoiser(r2, False)
    api.vnrRendererSetDenoiser(r2, True)
    api.vnrRender(r2)
    assert np.array_equal(api.vnrRendererMapFrame(r2), plain)
    assert "NOT denoised" in capfd.readouterr().err
    monkeypatch.setenv("VNR_AMD_DENOISER_STRICT", "1")
    with pytest.raises(api.VnrAmdError, match="denoiser is not available"):
        api.vnrRendererSetDenoiser(r2, True)
    api.vnrRendererSetDenoiser(r2, False)


NEURAL_FRAME_MODELS = [
    # (L, F, log2T, base, per_level_scale, hidden layers): each takes a different gather path of the fused kernel's queue mode
    (8, 4, 14, 4, None, 2),        # F = 4: paired 16-byte corner loads
    (8, 8, 19, 16, None, 2),       # BASELINE C2 model shape, F = 8: one 16-byte load per corner, 64-wide first layer
    (16, 2, 19, 16, 1.3195, 3),    # BASELINE C4 model shape (T = 2^19), F = 2: paired 8-byte loads, 3 hidden layers
]


@pytest.mark.parametrize("model", NEURAL_FRAME_MODELS)
def test_neural_streaming_matches_oracle(oracle, scene, model):
    """mode 5 on a neural volume with random (seeded) parameters and the ground-truth macrocell"""
    L, F, log2T, base, pls, H = model
    cfg = syn.model_config(n_levels=L, n_features=F, log2_hashmap_size=log2T, base_resolution=base, n_hidden_layers=H,
                           per_level_scale=pls)
    nv = api.vnrCreateNeuralVolume(cfg, scene["sv"], online_macrocell_construction=False)
    info = api.neural_info(nv)
    ocfg = oracle.grid_config(L, F, log2T, base, 2.0 if pls is None else pls)
    n_mlp = oracle.mlp_n_params(info["padded_width"], 64, H - 1)
    params = syn.random_params(info["n_params"], n_mlp, seed=21)
    # bias the network output into the TFN's visible range
    api.neural_set_params_fp16(nv, params)
    r = make_renderer(scene, nv, size=(64, 56))
    api.vnrRender(r)
    img = api.vnrRendererMapFrame(r).copy()
    st = api.vnrRendererGetFrameStats(r)
    mo = api.volume_macrocell(scene["sv"])["max_opacity"]
    sc = oracle_scene(oracle, scene, mo, size=(64, 56))
    want, _, ost = oracle.render_streaming(sc, lambda c: oracle.network_inference(ocfg, 64, H, params.view(np.uint16), c))
    assert st["n_rays_hit"] == ost["n_rays_hit"]
    assert img[..., 3].max() > 0.05
    # stated tolerance: network outputs differ by <= 2^-8, which the TFN + compositing can amplify slightly
    assert psnr(img, want) > 75, psnr(img, want)       # measured 87.6 - 102.5 dB on the three shapes (round 2's bar was 40 dB)
    l2 = np.sqrt(((img - want) ** 2).sum(-1))
    assert l2.mean() < 2e-4 and np.quantile(l2, 0.99) < 2e-3
    # the renderer alone: the oracle's marcher fed by the library's network values at the oracle's own sample positions (the network's
    # 2^-8 per sample is tests/test_gpu_network.py's subject): the bar of the ground-truth frames
    want2, _, ost2 = oracle.render_streaming(sc, lambda c: api.neural_inference(nv, c))
    assert st["n_iterations"] == ost2["n_iterations"]
    print(f"\nneural frame {model}: vs oracle network PSNR {psnr(img, want):.1f} dB; compositor alone PSNR {psnr(img, want2):.1f} dB, max |err| {np.abs(img - want2).max():.2e}")
    assert np.abs(img - want2).max() < 5e-6 and psnr(img, want2) > 130, (float(np.abs(img - want2).max()), psnr(img, want2))   # measured 2.4e-7, 157 dB


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("kind", ["groundtruth", "neural"])
def test_interleaved_shares_assemble_to_the_unsharded_frame(scene, world, kind):
    """the multi-GPU render path on ONE device: every rank's share (vnrRendererSetPixelInterleave, 8-scanline blocks,
    rendered as two halves on two streams inside the library) packed and assembled exactly as instantvnr_amd.dist does
    must equal the unsharded frame bit for bit.  80 scanlines = 10 tile rows: ragged for every world size here."""
    from instantvnr_amd import dist as vdist
    size = (96, 80)
    n_pixels = size[0] * size[1]
    block = 8 * size[0]
    if kind == "neural":
        cfg = syn.model_config(n_levels=8, n_features=4, log2_hashmap_size=14, base_resolution=4, n_hidden_layers=2)
        volume = api.vnrCreateNeuralVolume(cfg, scene["sv"], online_macrocell_construction=False)
        info = api.neural_info(volume)
        n_mlp = (info["padded_width"] * 64) + 64 * 64 + 16 * 64   # first + 1 hidden + padded last layer
        api.neural_set_params_fp16(volume, syn.random_params(info["n_params"], n_mlp, seed=21))
    else:
        volume = scene["sv"]
    # a close camera, so that the volume fills most of the frame and (almost) every share has content
    cam = syn.oblique_camera((48, 48, 48), distance_scale=0.95)
    camera = api.vnrCreateCamera()
    api.vnrCameraSet(camera, cam["from"], cam["at"], cam["up"], cam["fovy"])

    def renderer():
        rr = make_renderer(scene, volume, size=size)
        api.vnrRendererSetCamera(rr, camera)
        return rr

    r = renderer()
    api.vnrRender(r)
    want = api.vnrRendererMapFrame(r).reshape(-1, 4).copy()
    # not vacuous: visible pixels exist and are spread over most 8-scanline blocks, so most shares have content
    rows_with_content = [bool((want[b * block:(b + 1) * block, 3] > 0).any()) for b in range(n_pixels // block)]
    assert (want[:, 3] > 0).mean() > 0.2 and sum(rows_with_content) >= 8, ((want[:, 3] > 0).mean(), rows_with_content)
    shares = []
    for part in range(world):
        rp = renderer()   # one renderer per rank
        api.vnrRendererSetPixelInterleave(rp, block, world, part)
        api.vnrRender(rp)
        frame = api.vnrRendererMapFrame(rp).reshape(-1, 4).copy()
        shares.append(vdist.pack_share(frame, block, world, part, n_pixels))
    full = vdist.assemble_shares(np.stack(shares), block, world, n_pixels)
    assert np.array_equal(full, want)


def test_non_cubic_ragged_volume_matches_oracle(oracle):
    """50 x 37 x 21 voxels (x fastest): not a cube and not a multiple of the 16-voxel macrocell in any axis, so an x/y/z
    mix-up or a ragged-edge error anywhere (sampling, macrocell kernels, object->world transform, DDA bounds, camera) shows.
    Same bars as the cubic tests: sampling and macrocells bit-exact, frames within 2e-4 (device powf vs glibc)."""
    nx, ny, nz = 50, 37, 21
    z, y, x = np.meshgrid(np.linspace(0, 1, nz), np.linspace(0, 1, ny), np.linspace(0, 1, nx), indexing="ij")
    vol = (0.5 + 0.5 * np.sin(5.0 * x + 1.0) * np.cos(3.0 * y) * np.sin(2.0 * z + 0.5)).astype(np.float32)   # asymmetric in x, y, z
    vol[:, :, :6] *= 0.1                                                                                    # an empty-ish slab on one x side only
    dims = (nx, ny, nz)
    assert vol.min() > 0.0 and vol.max() < 1.0           # so the load-time normalisation is NOT the identity (it is for analytic_volume)
    sv = api.vnrCreateSimpleVolume(vol)                  # the library gets the RAW data and normalises it itself
    # restatement of the reference's load-time normalisation, convert_volume (neural_sampler.cpp:176-210):
    # clamp((v - vmin) / (vmax - vmin), 0, 1) in fp32 with a true division; the oracle samples this array
    lo, hi = np.float32(vol.min()), np.float32(vol.max())
    vol = np.clip((vol - lo) / (hi - lo), np.float32(0), np.float32(1)).astype(np.float32)
    assert api.vnrVolumeGetValueRange(sv) == (0.0, 1.0)
    rng = np.random.default_rng(3)
    c = rng.uniform(-0.05, 1.05, (4000, 3)).astype(np.float32)
    for nodal in (False, True):
        assert np.array_equal(api.simple_volume_sample(sv, c, nodal), oracle.sample_volume(vol, c, nodal))
    colors, alphas = syn.tfn_ramp_with_bumps()
    tfn = api.vnrCreateTransferFunction()
    api.vnrTransferFunctionSetColor(tfn, colors)
    api.vnrTransferFunctionSetAlpha(tfn, alphas)
    api.vnrTransferFunctionSetValueRange(tfn, (0, 1))
    otfn = oracle.TfnHolder(colors, alphas)
    cam = syn.oblique_camera(dims, distance_scale=1.2)
    camera = api.vnrCreateCamera()
    api.vnrCameraSet(camera, cam["from"], cam["at"], cam["up"], cam["fovy"])
    size = (88, 72)
    images = {}
    for mode in (5, 4):
        r = api.vnrCreateRenderer(sv)
        api.vnrRendererSetTransferFunction(r, tfn)
        api.vnrRendererSetCamera(r, camera)
        api.vnrRendererSetFramebufferSize(r, size)
        api.vnrRendererSetMode(r, mode)
        api.vnrRender(r)
        images[mode] = api.vnrRendererMapFrame(r).copy()
        if mode == 5:
            st = api.vnrRendererGetFrameStats(r)
    mc = api.volume_macrocell(sv)
    assert mc["dims"] == (4, 3, 2)                       # ceil(50/16), ceil(37/16), ceil(21/16)
    vr = oracle.macrocell_compute_implicit(vol)
    assert np.array_equal(mc["value_range"], vr)
    mo = oracle.macrocell_max_opacity(otfn, vr)
    assert np.array_equal(mc["max_opacity"], mo)
    sc = oracle.SceneHolder(size[0], size[1], dims, otfn, mo, cam["from"], cam["at"], cam["up"], cam["fovy"])
    want5, _, ost = oracle.render_streaming(sc, lambda q: oracle.sample_volume(vol, q, nodal=True))
    want4, _ = oracle.render_monolithic(sc, vol)
    assert st["n_rays_hit"] == ost["n_rays_hit"] > 500 and st["n_iterations"] == ost["n_iterations"]
    assert (want5[..., 3] > 0).mean() > 0.1
    assert np.abs(images[5] - want5).max() < 2e-4, np.abs(images[5] - want5).max()
    assert np.abs(images[4] - want4).max() < 2e-4, np.abs(images[4] - want4).max()
    # the left/right asymmetry of the volume is visible, so a mirrored axis could not pass by symmetry
    a = want5[..., 3]
    assert abs(a[:, : size[0] // 2].mean() - a[:, size[0] // 2:].mean()) > 0.01


# --------------------------------------------------------------------------- gradient shading (modes 7 / 8)
def _camera(frm):
    cam = api.vnrCreateCamera()
    api.vnrCameraSet(cam, frm, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0)
    return cam


@pytest.mark.parametrize("side", ["light not flipped", "light flipped"])
@pytest.mark.parametrize("mode", [8, 7])
def test_gradient_shading_groundtruth_matches_oracle(oracle, scene, mode, side):
    """VNR_RAYMARCHING_GRADIENT_SHADING_{SAMPLE_STREAMING = 8, DECODING = 7} on a dense volume: 4 evaluations per sample
    (streaming) / sampleGradient with its boundary flip (monolithic), shade_scivis_light, light flipped towards the viewer."""
    frm = scene["cam"]["from"] if side == "light not flipped" else tuple(-v for v in scene["cam"]["from"])
    light = oracle.flipped_light_dir(frm, (0, 0, 0))
    assert bool(np.allclose(light, oracle.DEFAULT_LIGHT_DIR)) == (side == "light not flipped")   # the two cases do differ
    r = make_renderer(scene, scene["sv"], mode=mode)
    api.vnrRendererSetCamera(r, _camera(frm))
    api.vnrRender(r)
    img = api.vnrRendererMapFrame(r).copy()
    mo = api.volume_macrocell(scene["sv"])["max_opacity"]
    f = lambda c: oracle.sample_volume(scene["vol"], c, nodal=True)
    sc = oracle.SceneHolder(96, 80, (48, 48, 48), scene["otfn"], mo, frm, fovy=45.0, shading_mode=1)
    plain = oracle.SceneHolder(96, 80, (48, 48, 48), scene["otfn"], mo, frm, fovy=45.0, shading_mode=0)
    if mode == 8:
        want, _, ost = oracle.render_streaming(sc, f)
        unshaded, _, _ = oracle.render_streaming(plain, f)
        st = api.vnrRendererGetFrameStats(r)
        assert st["n_rays_hit"] == ost["n_rays_hit"] > 1000 and st["n_iterations"] == ost["n_iterations"]
        assert st["n_samples"] <= ost["n_samples"]      # shading samples (each is 4 evaluations), as in mode 5
    else:
        want, _ = oracle.render_monolithic(sc, scene["vol"])
        unshaded, _ = oracle.render_monolithic(plain, scene["vol"])
    assert np.abs(want[..., :3] - unshaded[..., :3]).mean() > 2e-3     # the shading is visible, so the comparison is not vacuous
    assert np.array_equal(want[..., 3], unshaded[..., 3])              # and changes colour only
    # identical arithmetic except powf (opacity correction, specular term): measured max |err| 2e-7 .. 4e-7, PSNR 160 dB
    # (tools/gradient_mode_numbers.py); the bar leaves two orders of magnitude and would still catch any real difference
    assert np.abs(img - want).max() < 2e-5, np.abs(img - want).max()
    assert psnr(img, want) > 110


def test_gradient_shading_neural_streaming_matches_oracle(oracle, scene):
    """mode 8 on a neural volume: the four coordinates of every sample go through the network (C4 model shape)"""
    L, F, log2T, base, pls, H = 16, 2, 19, 16, 1.3195, 3
    cfg = syn.model_config(n_levels=L, n_features=F, log2_hashmap_size=log2T, base_resolution=base, n_hidden_layers=H, per_level_scale=pls)
    nv = api.vnrCreateNeuralVolume(cfg, scene["sv"], online_macrocell_construction=False)
    info = api.neural_info(nv)
    ocfg = oracle.grid_config(L, F, log2T, base, pls)
    params = syn.random_params(info["n_params"], oracle.mlp_n_params(info["padded_width"], 64, H - 1), seed=21)
    api.neural_set_params_fp16(nv, params)
    r = make_renderer(scene, nv, size=(64, 56), mode=8)
    api.vnrRender(r)
    img = api.vnrRendererMapFrame(r).copy()
    st = api.vnrRendererGetFrameStats(r)
    mo = api.volume_macrocell(scene["sv"])["max_opacity"]
    cam = scene["cam"]
    sc = oracle.SceneHolder(64, 56, (48, 48, 48), scene["otfn"], mo, cam["from"], cam["at"], cam["up"], cam["fovy"], shading_mode=1)
    want, _, ost = oracle.render_streaming(sc, lambda c: oracle.network_inference(ocfg, 64, H, params.view(np.uint16), c))
    assert st["n_rays_hit"] == ost["n_rays_hit"]
    assert img[..., 3].max() > 0.05
    # measured (tools/gradient_mode_numbers.py): 88.6 dB against this fp32-accumulate oracle (87.6 dB for the unshaded mode 5
    # frame), while the oracle's own fp16-accumulate variant is only 66 dB from it: the MFMA path accumulates in fp32.
    # Bar: above what the fp16-accumulate variant reaches, with margin below the measured value.
    assert psnr(img, want) > 70, psnr(img, want)
    # the renderer alone (gradient shading included): the oracle's marcher fed by the library's network values
    want_lib, _, _ = oracle.render_streaming(sc, lambda c: api.neural_inference(nv, c))
    print(f"\nmode 8 neural: vs oracle network {psnr(img, want):.1f} dB; compositor alone max |err| {np.abs(img - want_lib).max():.2e}")
    assert np.abs(img - want_lib).max() < 1e-5
    # mode 5 on the same renderer afterwards still works on the larger (gradient-sized) queues
    api.vnrRendererSetMode(r, 5)
    api.vnrRendererResetAccumulation(r)
    api.vnrRender(r)
    img5 = api.vnrRendererMapFrame(r).copy()
    plain = oracle.SceneHolder(64, 56, (48, 48, 48), scene["otfn"], mo, cam["from"], cam["at"], cam["up"], cam["fovy"])
    want5, _, _ = oracle.render_streaming(plain, lambda c: oracle.network_inference(ocfg, 64, H, params.view(np.uint16), c))
    assert psnr(img5, want5) > 75


@pytest.mark.parametrize("side", ["light not flipped", "light flipped"])
@pytest.mark.parametrize("mode", [11, 10])
def test_single_shade_heuristic_groundtruth_matches_oracle(oracle, scene, mode, side):
    """VNR_RAYMARCHING_SINGLE_SHADE_HEURISTIC_{SAMPLE_STREAMING = 11, DECODING = 10} on a dense volume: the camera ray remembers
    the sample that contributed most, one shadow ray from there towards the light gives a transmittance, and the pixel becomes
    lerp(0.95, colour, highest colour x alpha x transmittance) (method_raymarching.cu:455-484 monolithic; :789-833, 877-900 and
    the two loops of :968-971 streaming).  Accumulation over two frames included: both passes write through writePixelColor."""
    frm = scene["cam"]["from"] if side == "light not flipped" else tuple(-v for v in scene["cam"]["from"])
    r = make_renderer(scene, scene["sv"], mode=mode)
    api.vnrRendererSetCamera(r, _camera(frm))
    mo = api.volume_macrocell(scene["sv"])["max_opacity"]
    f = lambda c: oracle.sample_volume(scene["vol"], c, nodal=True)
    acc = None
    for frame_index in (1, 2):
        api.vnrRender(r)
        img = api.vnrRendererMapFrame(r).copy()
        sc = oracle.SceneHolder(96, 80, (48, 48, 48), scene["otfn"], mo, frm, fovy=45.0, shading_mode=2, frame_index=frame_index)
        plain = oracle.SceneHolder(96, 80, (48, 48, 48), scene["otfn"], mo, frm, fovy=45.0, shading_mode=0, frame_index=frame_index)
        if mode == 11:
            want, acc, ost = oracle.render_streaming(sc, f, accumulation=acc)
            st = api.vnrRendererGetFrameStats(r)
            assert st["n_rays_hit"] == ost["n_rays_hit"] > 1000
            assert st["n_iterations"] == ost["n_iterations"]         # camera pass + shadow pass
            assert st["n_samples"] <= ost["n_samples"]
        else:
            want, acc = oracle.render_monolithic(sc, scene["vol"], accumulation=acc)
        if frame_index == 1:
            unshaded = oracle.render_streaming(plain, f)[0] if mode == 11 else oracle.render_monolithic(plain, scene["vol"])[0]
            assert np.abs(want[..., :3] - unshaded[..., :3]).mean() > 2e-3     # the shadows are visible
            assert np.array_equal(want[..., 3], unshaded[..., 3])              # and change colour only
        assert np.abs(img - want).max() < 2e-5, (frame_index, np.abs(img - want).max())
        assert psnr(img, want) > 110


def test_single_shade_heuristic_neural_streaming_matches_oracle(oracle, scene):
    """mode 11 on a neural volume: both passes evaluate the network (C4 model shape); same bar as mode 8"""
    L, F, log2T, base, pls, H = 16, 2, 19, 16, 1.3195, 3
    cfg = syn.model_config(n_levels=L, n_features=F, log2_hashmap_size=log2T, base_resolution=base, n_hidden_layers=H, per_level_scale=pls)
    nv = api.vnrCreateNeuralVolume(cfg, scene["sv"], online_macrocell_construction=False)
    info = api.neural_info(nv)
    ocfg = oracle.grid_config(L, F, log2T, base, pls)
    params = syn.random_params(info["n_params"], oracle.mlp_n_params(info["padded_width"], 64, H - 1), seed=22)
    api.neural_set_params_fp16(nv, params)
    r = make_renderer(scene, nv, size=(64, 56), mode=11)
    api.vnrRender(r)
    img = api.vnrRendererMapFrame(r).copy()
    st = api.vnrRendererGetFrameStats(r)
    mo = api.volume_macrocell(scene["sv"])["max_opacity"]
    cam = scene["cam"]
    sc = oracle.SceneHolder(64, 56, (48, 48, 48), scene["otfn"], mo, cam["from"], cam["at"], cam["up"], cam["fovy"], shading_mode=2)
    want, _, ost = oracle.render_streaming(sc, lambda c: oracle.network_inference(ocfg, 64, H, params.view(np.uint16), c))
    assert st["n_rays_hit"] == ost["n_rays_hit"]
    assert img[..., 3].max() > 0.05
    assert psnr(img, want) > 70, psnr(img, want)
    want_lib, _, _ = oracle.render_streaming(sc, lambda c: api.neural_inference(nv, c))
    print(f"\nmode 11 neural: vs oracle network {psnr(img, want):.1f} dB; compositor alone max |err| {np.abs(img - want_lib).max():.2e}")
    assert np.abs(img - want_lib).max() < 1e-5
    # modes 5 and 8 on the same renderer afterwards (queues, ray lists and predictions are shared between the modes)
    for m, sm in ((5, 0), (8, 1)):
        api.vnrRendererSetMode(r, m)
        api.vnrRendererResetAccumulation(r)
        api.vnrRender(r)
        got = api.vnrRendererMapFrame(r).copy()
        s2 = oracle.SceneHolder(64, 56, (48, 48, 48), scene["otfn"], mo, cam["from"], cam["at"], cam["up"], cam["fovy"], shading_mode=sm)
        w2, _, _ = oracle.render_streaming(s2, lambda c: oracle.network_inference(ocfg, 64, H, params.view(np.uint16), c))
        assert psnr(got, w2) > 70


def test_path_tracing_streaming_matches_oracle(oracle, scene):
    """VNR_PATHTRACING_SAMPLE_STREAMING (mode 14) on a dense volume against the oracle's restatement of
    method_pathtracing.cu:532-813, two accumulated frames.  A path is a chain of decisions on random numbers (collision or not,
    Russian roulette), so a last-bit difference in logf / sincosf between the device and glibc can send a pixel down another
    path: the bar is on how many pixels agree, and the rest must still be plausible radiance.  (Since csrc/pt_device.h restates glibc's logf and
    sincosf the two do agree; the bar stays where it was.)"""
    r = make_renderer(scene, scene["sv"], mode=14)
    api.vnrRendererSetVolumeDensityScale(r, 6.0)
    mo = api.volume_macrocell(scene["sv"])["max_opacity"]
    f = lambda c: oracle.sample_volume(scene["vol"], c, nodal=True)
    acc = None
    for frame_index in (1, 2):
        api.vnrRender(r)
        img = api.vnrRendererMapFrame(r).copy()
        st = api.vnrRendererGetFrameStats(r)
        cam = scene["cam"]
        sc = oracle.SceneHolder(96, 80, (48, 48, 48), scene["otfn"], mo, cam["from"], cam["at"], cam["up"], cam["fovy"],
                                frame_index=frame_index, density_scale=6.0)
        want, acc, ost = oracle.render_pathtracing(sc, f, accumulation=acc)
        assert st["n_rays_hit"] == ost["n_rays_hit"] > 1000
        assert np.array_equal(img[..., 3], want[..., 3]) and (want[..., 3] == 1.0).all()
        assert want[..., :3].max() > 0.5 and (want[..., :3].sum(axis=2) > 0).mean() > 0.03      # light does arrive
        same = np.abs(img - want).max(axis=2) < 1e-5
        assert same.mean() > 0.995, same.mean()
        assert abs(float(img[..., :3].mean()) - float(want[..., :3].mean())) < 2e-3
        assert abs(st["n_samples"] - ost["n_samples"]) < 0.01 * ost["n_samples"]
        assert abs(st["n_iterations"] - ost["n_iterations"]) <= max(4, 0.2 * ost["n_iterations"])


def test_path_tracing_on_a_neural_volume_runs_and_converges(oracle, scene):
    """mode 14 with the network as the sampler: many frames accumulate towards the oracle's many-frame mean"""
    L, F, log2T, base, pls, H = 8, 4, 15, 8, 1.5, 2
    cfg = syn.model_config(n_levels=L, n_features=F, log2_hashmap_size=log2T, base_resolution=base, n_hidden_layers=H, per_level_scale=pls)
    nv = api.vnrCreateNeuralVolume(cfg, scene["sv"], online_macrocell_construction=False)
    api.vnrNeuralVolumeTrain(nv, 300, True)
    r = make_renderer(scene, nv, size=(48, 40), mode=14)
    frames = 24
    for _ in range(frames):
        api.vnrRender(r)
        img = api.vnrRendererMapFrame(r).copy()
    mo = api.volume_macrocell(scene["sv"])["max_opacity"]
    cam = scene["cam"]
    acc = None
    for k in range(frames):
        sc = oracle.SceneHolder(48, 40, (48, 48, 48), scene["otfn"], mo, cam["from"], cam["at"], cam["up"], cam["fovy"], frame_index=k + 1)
        want, acc, _ = oracle.render_pathtracing(sc, lambda c: oracle.sample_volume(scene["vol"], c, nodal=True), accumulation=acc)
    # the network approximates the volume (PSNR > 30 dB after 300 steps) and individual paths differ, so compare the images coarsely
    assert (img[..., 3] == 1.0).all()
    assert abs(float(img[..., :3].mean()) - float(want[..., :3].mean())) < 0.15 * float(want[..., :3].mean())
    assert np.corrcoef(img[..., :3].reshape(-1), want[..., :3].reshape(-1))[0, 1] > 0.8


def test_path_tracing_decoding_mode_matches_oracle(oracle, scene):
    """VNR_PATHTRACING_DECODING (mode 13): the path tracer in one loop per pixel on dense data (method_pathtracing.cu:258-292,
    420-510); same kind of bar as mode 14.  The two estimators are not the same random walk (the interval is reset before a
    bounce here), but they estimate the same image."""
    r = make_renderer(scene, scene["sv"], mode=13)
    api.vnrRendererSetVolumeDensityScale(r, 6.0)
    mo = api.volume_macrocell(scene["sv"])["max_opacity"]
    cam = scene["cam"]
    acc = None
    for frame_index in (1, 2):
        api.vnrRender(r)
        img = api.vnrRendererMapFrame(r).copy()
        sc = oracle.SceneHolder(96, 80, (48, 48, 48), scene["otfn"], mo, cam["from"], cam["at"], cam["up"], cam["fovy"],
                                frame_index=frame_index, density_scale=6.0)
        want, acc = oracle.render_pathtracing_monolithic(sc, scene["vol"], accumulation=acc)
        assert np.array_equal(img[..., 3], want[..., 3]) and (want[..., 3] == 1.0).all()
        assert (want[..., :3].sum(axis=2) > 0).mean() > 0.03
        same = np.abs(img - want).max(axis=2) < 1e-5
        assert same.mean() > 0.995, same.mean()
        assert abs(float(img[..., :3].mean()) - float(want[..., :3].mean())) < 2e-3


def test_in_shader_mode_6_is_the_uninterrupted_march(oracle, scene):
    """VNR_RAYMARCHING_NO_SHADING_IN_SHADER (mode 6) marches a ray in one loop (network_raymarching_iterator,
    method_raymarching.cu:310-356); its arithmetic is the streaming loop's without interruptions, which the oracle reproduces with a
    batch size no ray reaches.  The library runs it on the streaming path: same frame within the resume rounding."""
    r = make_renderer(scene, scene["sv"], mode=6)
    api.vnrRender(r)
    img = api.vnrRendererMapFrame(r).copy()
    mo = api.volume_macrocell(scene["sv"])["max_opacity"]
    want, _, ost = oracle.render_streaming(oracle_scene(oracle, scene, mo), lambda c: oracle.sample_volume(scene["vol"], c, nodal=True), n_iters=512)
    assert ost["n_iterations"] == 1      # nothing was interrupted in the oracle run
    assert np.abs(img - want).max() < 2e-4 and psnr(img, want) > 80


def test_in_shader_mode_12_single_shade_heuristic(oracle, scene):
    """VNR_RAYMARCHING_SINGLE_SHADE_HEURISTIC_IN_SHADER: camera march as in mode 11 but uninterrupted, shadow ray at twice the
    step with the pixel's third random number (network_raymarching_transmittance, method_raymarching.cu:981-1035)"""
    r = make_renderer(scene, scene["sv"], mode=12)
    api.vnrRender(r)
    img = api.vnrRendererMapFrame(r).copy()
    mo = api.volume_macrocell(scene["sv"])["max_opacity"]
    cam = scene["cam"]
    f = lambda c: oracle.sample_volume(scene["vol"], c, nodal=True)
    sc = oracle.SceneHolder(96, 80, (48, 48, 48), scene["otfn"], mo, cam["from"], cam["at"], cam["up"], cam["fovy"], shading_mode=3)
    want, _, _ = oracle.render_streaming(sc, f, n_iters=512)
    assert np.abs(img - want).max() < 2e-4 and psnr(img, want) > 80
    sc11 = oracle.SceneHolder(96, 80, (48, 48, 48), scene["otfn"], mo, cam["from"], cam["at"], cam["up"], cam["fovy"], shading_mode=2)
    other, _, _ = oracle.render_streaming(sc11, f, n_iters=512)
    assert np.abs(want[..., :3] - other[..., :3]).mean() > 1e-4      # modes 11 and 12 are different estimates of the shadow


def test_in_shader_mode_9_gradient_shading(oracle):
    """VNR_RAYMARCHING_GRADIENT_SHADING_IN_SHADER: mode 8 whose forward differences flip at the far faces of the volume
    (sampleGradient, raytracing.h:128-143), uninterrupted.  The volume is a ramp that is densest at its +x, +y, +z faces and the
    camera looks at those faces, so the first samples of every ray lie in the last voxel, where the flip applies."""
    n = 40
    g = (np.arange(n, dtype=np.float32) + 0.5) / n
    vol = np.clip(0.15 + 0.85 * np.maximum.reduce(np.meshgrid(g, g, g, indexing="ij")) ** 3, 0, 1).astype(np.float32)
    sv = api.vnrCreateSimpleVolume(vol, (0.0, 1.0))
    colors, alphas = syn.tfn_ramp_with_bumps()
    tfn = api.vnrCreateTransferFunction()
    api.vnrTransferFunctionSetColor(tfn, colors)
    api.vnrTransferFunctionSetAlpha(tfn, alphas)
    api.vnrTransferFunctionSetValueRange(tfn, (0, 1))
    frm = (70.0, 55.0, 62.0)
    camera = api.vnrCreateCamera()
    api.vnrCameraSet(camera, frm, (0, 0, 0), (0, 1, 0), 45.0)
    otfn = oracle.TfnHolder(colors, alphas)
    frames = {}
    for mode in (9, 8):
        r = api.vnrCreateRenderer(sv)
        api.vnrRendererSetTransferFunction(r, tfn)
        api.vnrRendererSetCamera(r, camera)
        api.vnrRendererSetFramebufferSize(r, (96, 80))
        api.vnrRendererSetMode(r, mode)
        api.vnrRender(r)
        frames[mode] = api.vnrRendererMapFrame(r).copy()
    mo = api.volume_macrocell(sv)["max_opacity"]
    f = lambda c: oracle.sample_volume(vol, c, nodal=True)
    want = {}
    for mode, sm in ((9, 4), (8, 1)):
        sc = oracle.SceneHolder(96, 80, (n, n, n), otfn, mo, frm, fovy=45.0, shading_mode=sm)
        want[mode], _, _ = oracle.render_streaming(sc, f, n_iters=512)
    changed = int((np.abs(want[9] - want[8]).max(axis=2) > 1e-6).sum())
    assert changed > 200, changed                   # the flip is visible in this scene, so the comparison below means something
    for mode in (9, 8):
        assert np.abs(frames[mode] - want[mode]).max() < 2e-4 and psnr(frames[mode], want[mode]) > 80
    assert int((np.abs(frames[9] - frames[8]).max(axis=2) > 1e-6).sum()) > 200


def test_in_shader_mode_15_path_tracing(oracle, scene):
    """VNR_PATHTRACING_IN_SHADER: the estimator of mode 13 on the streaming loop: the interval is reset before a bounce and a bounce
    that leaves the volume at once still collects the ambient light (mode 14 drops that term, method_pathtracing.cu:631-635 vs
    447-452).  On a dense volume it must agree with BOTH oracle programs, the streaming one with that flag and the monolithic
    one, which agree with each other bit for bit; a thin medium makes the two differences from mode 14 visible."""
    r = make_renderer(scene, scene["sv"], mode=15)
    api.vnrRendererSetVolumeDensityScale(r, 0.25)
    mo = api.volume_macrocell(scene["sv"])["max_opacity"]
    cam = scene["cam"]
    f = lambda c: oracle.sample_volume(scene["vol"], c, nodal=True)
    acc = acc_mono = acc14 = None
    for frame_index in (1, 2, 3, 4):
        api.vnrRender(r)
        img = api.vnrRendererMapFrame(r).copy()
        mk = lambda sm: oracle.SceneHolder(96, 80, (48, 48, 48), scene["otfn"], mo, cam["from"], cam["at"], cam["up"], cam["fovy"],
                                           density_scale=0.25, shading_mode=sm, frame_index=frame_index)
        want, acc, _ = oracle.render_pathtracing(mk(5), f, accumulation=acc)
        mono, acc_mono = oracle.render_pathtracing_monolithic(mk(5), scene["vol"], accumulation=acc_mono)
        other, acc14, _ = oracle.render_pathtracing(mk(0), f, accumulation=acc14)
        assert np.array_equal(want, mono)                                  # one estimator, two programs
        assert (np.abs(img - want).max(axis=2) < 1e-5).mean() > 0.995
    assert (np.abs(other - want).max(axis=2) > 1e-6).sum() > 10            # and it is not mode 14's


# ---- the in-shader kernel on neural volumes (in_shader.h): one launch per frame, the network evaluated inside the marching loop ----
def _neural_c4_shape(oracle, scene, seed):
    L, F, log2T, base, pls, H = 16, 2, 19, 16, 1.3195, 3
    cfg = syn.model_config(n_levels=L, n_features=F, log2_hashmap_size=log2T, base_resolution=base, n_hidden_layers=H, per_level_scale=pls)
    nv = api.vnrCreateNeuralVolume(cfg, scene["sv"], online_macrocell_construction=False)
    info = api.neural_info(nv)
    params = syn.random_params(info["n_params"], oracle.mlp_n_params(info["padded_width"], 64, H - 1), seed=seed)
    api.neural_set_params_fp16(nv, params)
    return nv, oracle.grid_config(L, F, log2T, base, pls), params, H


def _set_in_shader(r, mode):
    from instantvnr_amd._lib import check, lib
    check(lib().vnrAmdRendererSetInShaderKernel(r.h, mode))


@pytest.mark.parametrize("mode,shading_mode", [(6, 0), (9, 4), (12, 3)])
def test_in_shader_kernel_on_a_neural_volume(oracle, scene, mode, shading_mode):
    """modes 6 / 9 / 12 on a neural volume run in_shader_kernel (the network inside the marching loop, method_raymarching.cu:981-1249).
    Against the oracle's uninterrupted march driven by the oracle network: the bars of the streaming modes 5 / 8 / 11.  Against the
    library's own streaming path on the same parameters (vnrAmdRendererSetInShaderKernel(0)): the network values are the same bits, so
    the two frames differ only by the streaming path's resume rounding; hit rays equal, and no more evaluations than the streaming path."""
    nv, ocfg, params, H = _neural_c4_shape(oracle, scene, seed=20 + mode)
    size = (64, 56)
    frames, stats = {}, {}
    for kernel in (1, 0):
        r = make_renderer(scene, nv, size=size, mode=mode)
        _set_in_shader(r, kernel)
        api.vnrRender(r)
        first = api.vnrRendererMapFrame(r).copy()
        stats[kernel] = api.vnrRendererGetFrameStats(r)
        api.vnrRender(r)                                  # a second, accumulated frame (other jitter)
        frames[kernel] = (first, api.vnrRendererMapFrame(r).copy())
    assert stats[1]["n_iterations"] == 1 and stats[0]["n_iterations"] >= 1
    assert stats[1]["n_rays_hit"] == stats[0]["n_rays_hit"] > 1000
    # the streaming path evaluates a whole batch before it composes it, i.e. also the samples behind the one that saturates a ray;
    # the in-shader loop stops there
    assert 0.5 * stats[0]["n_samples"] < stats[1]["n_samples"] <= stats[0]["n_samples"]
    for k in (0, 1):
        d = np.abs(frames[1][k] - frames[0][k])
        assert d.max() < 2e-3 and psnr(frames[1][k], frames[0][k]) > 70, (k, d.max(), psnr(frames[1][k], frames[0][k]))
    assert not np.array_equal(frames[1][0], frames[1][1])     # the second frame did add something
    mo = api.volume_macrocell(scene["sv"])["max_opacity"]
    cam = scene["cam"]
    sc = oracle.SceneHolder(size[0], size[1], (48, 48, 48), scene["otfn"], mo, cam["from"], cam["at"], cam["up"], cam["fovy"], shading_mode=shading_mode)
    want, _, ost = oracle.render_streaming(sc, lambda c: oracle.network_inference(ocfg, 64, H, params.view(np.uint16), c), n_iters=512)
    assert ost["n_rays_hit"] == stats[1]["n_rays_hit"]
    assert frames[1][0][..., 3].max() > 0.05
    assert psnr(frames[1][0], want) > (40 if mode == 6 else 70), psnr(frames[1][0], want)


def test_in_shader_kernel_shares_and_pixel_ranges(oracle, scene):
    """the in-shader kernel under the multi-GPU interleave and under a pixel range: every pixel is the unsharded frame's, bit for bit
    (a pixel's ray does not depend on which rays share its wave)"""
    nv, _, _, _ = _neural_c4_shape(oracle, scene, seed=31)
    size = (96, 80)
    r = make_renderer(scene, nv, size=size, mode=6)
    api.vnrRender(r)
    full = api.vnrRendererMapFrame(r).copy().reshape(-1, 4)
    got = np.zeros_like(full)
    for part in range(3):
        rp = make_renderer(scene, nv, size=size, mode=6)
        api.vnrRendererSetPixelInterleave(rp, 8 * size[0], 3, part)
        api.vnrRender(rp)
        share = api.vnrRendererMapFrame(rp).reshape(-1, 4)
        rows = np.arange(size[1]) // 8 % 3 == part
        mask = np.repeat(rows, size[0])
        got[mask] = share[mask]
    assert np.array_equal(got, full)
    lo, hi = 17 * size[0] + 5, 41 * size[0] + 90
    rr = make_renderer(scene, nv, size=size, mode=6)
    api.vnrRendererSetPixelRange(rr, lo, hi)
    api.vnrRender(rr)
    assert np.array_equal(api.vnrRendererMapFrame(rr).reshape(-1, 4)[lo:hi], full[lo:hi])


def test_in_shader_kernel_falls_back_where_it_has_no_instance(oracle, scene):
    """what is left without an in-shader instance after round 5 -- an encoded width outside the kernels' shape list (20 levels x 4 features =
    80), a network whose weight image exceeds the LDS (128 neurons x 7 hidden layers: its weights stay in global memory) -- and a dense
    volume take the streaming path: mode 6 still renders, and it is mode 5's frame"""
    shapes = [dict(n_levels=20, n_features=4, log2_hashmap_size=12, base_resolution=4, n_hidden_layers=2, per_level_scale=1.3),
              dict(n_levels=4, n_features=2, log2_hashmap_size=12, base_resolution=4, n_hidden_layers=7, n_neurons=128)]
    volumes = [scene["sv"]]
    for kw in shapes:
        W = kw.get("n_neurons", 64)
        cfg = syn.model_config(**kw)
        nv = api.vnrCreateNeuralVolume(cfg, scene["sv"], online_macrocell_construction=False)
        info = api.neural_info(nv)
        api.neural_set_params_fp16(nv, syn.random_params(info["n_params"], oracle.mlp_n_params(info["padded_width"], W, kw["n_hidden_layers"] - 1), seed=5,
                                                         mlp_scale=0.5 if W == 128 else 1.0))
        volumes.append(nv)
    for volume in volumes:
        r6, r5 = make_renderer(scene, volume, size=(64, 56), mode=6), make_renderer(scene, volume, size=(64, 56), mode=5)
        _set_in_shader(r6, 1)
        api.vnrRender(r6); api.vnrRender(r5)
        assert api.vnrRendererGetFrameStats(r6)["n_iterations"] >= 1
        assert np.array_equal(api.vnrRendererMapFrame(r6), api.vnrRendererMapFrame(r5))


# every FullyFusedMLP width the reference's in-shader dispatch instantiates and models of the GENERAL kind: tests/neural_pt_cases.py
IN_SHADER_MODELS = npc.IN_SHADER_MODELS
MARCHING_MLP_SCALE = {"w128": 0.5, "w64-sigmoid-exp": 0.5}   # (the ray-marching modes keep the parameters they have always been run on)


def _in_shader_model(oracle, scene, name, seed=None, mlp_scale=None):
    """a model of the case table; its own seed and weight scale (searched for a lit path-traced frame) unless others are given"""
    case = npc.CASES[name]
    nv = api.vnrCreateNeuralVolume(npc.model_config(case), scene["sv"], online_macrocell_construction=False)
    params = npc.parameters(oracle, case, seed, mlp_scale)
    assert api.neural_info(nv)["n_params"] == params.size
    api.neural_set_params_fp16(nv, params)
    return nv


@pytest.mark.parametrize("name", sorted(IN_SHADER_MODELS))
def test_in_shader_kernels_of_every_width_and_kind(oracle, scene, name):
    """modes 6 / 9 / 12 / 14 / 15 on models of 16, 32 and 128 neurons and of the GENERAL kind take the in-shader kernel (ONE launch per frame:
    n_iterations == 1) and give the streaming path's frame: bit for bit in the path-tracing modes (the same chain of decisions on the same
    network bits), to the streaming path's resume rounding in the marching modes (the bars of the 64-neuron test above); hit rays equal.
    The path-tracing modes run on the case table's parameters, on which the frame is lit (tests/test_neural_pt_cases_host.py): two black
    frames are equal whatever the scatter and shadow code does"""
    marching = _in_shader_model(oracle, scene, name, seed=77, mlp_scale=MARCHING_MLP_SCALE.get(name, 1.0))
    lit = _in_shader_model(oracle, scene, name)
    size = (64, 48)
    for mode in (6, 9, 12, 14, 15):
        frames, stats = {}, {}
        nv = lit if mode >= 14 else marching
        for kernel in (1, 0):
            r = make_renderer(scene, nv, size=size, mode=mode)
            if mode >= 14: api.vnrRendererSetVolumeDensityScale(r, 0.5)
            _set_in_shader(r, kernel)
            api.vnrRender(r); api.vnrRender(r)          # the second frame accumulates (other random numbers)
            frames[kernel] = api.vnrRendererMapFrame(r).copy()
            stats[kernel] = api.vnrRendererGetFrameStats(r)
        assert stats[1]["n_iterations"] == 1, (name, mode, "the in-shader kernel was not taken")
        assert stats[1]["n_rays_hit"] == stats[0]["n_rays_hit"] > 500
        assert np.isfinite(frames[1]).all()
        if mode >= 14:
            assert stats[1]["n_samples"] == stats[0]["n_samples"]
            assert np.array_equal(frames[1], frames[0]), (name, mode)
            assert npc.lit_share(frames[1]) >= npc.MIN_LIT, (name, mode, npc.lit_share(frames[1]))
        else:
            d = np.abs(frames[1] - frames[0])
            assert d.max() < 2e-3 and psnr(frames[1], frames[0]) > 70, (name, mode, d.max(), psnr(frames[1], frames[0]))


@pytest.mark.parametrize("mode", [14, 15])
def test_in_shader_path_tracing_kernel_equals_the_streaming_path_tracer(oracle, scene, mode):
    """modes 14 / 15 on a neural volume through in_shader_pt_kernel (the default for path tracing: it is the faster of the two) (one launch, the network inside the delta-tracking loop): per pixel the
    same chain of decisions on the same random numbers with the same network bits as the streaming path tracer, so the frames are
    equal BIT FOR BIT over accumulated frames, hit rays and evaluations equal"""
    nv = _in_shader_model(oracle, scene, "c4")      # the C4 shape on the case table's parameters: a lit frame
    size = (96, 80)
    frames, stats = {}, {}
    for kernel in (1, 0):
        r = make_renderer(scene, nv, size=size, mode=mode)
        api.vnrRendererSetVolumeDensityScale(r, 0.5)
        _set_in_shader(r, kernel)
        acc, n = [], 0
        for _ in range(3):
            api.vnrRender(r)
            acc.append(api.vnrRendererMapFrame(r).copy())
            n += api.vnrRendererGetFrameStats(r)["n_samples"]
        frames[kernel], stats[kernel] = acc, (n, api.vnrRendererGetFrameStats(r)["n_rays_hit"], api.vnrRendererGetFrameStats(r)["n_iterations"])
    assert stats[1][2] == 1 and stats[0][2] > 3                     # one launch against a chain of iterations
    assert stats[1][0] == stats[0][0] > 10000 and stats[1][1] == stats[0][1]
    for k in range(3):
        assert np.array_equal(frames[1][k], frames[0][k])
    assert frames[1][2][..., 3].min() == 1.0 and frames[1][2][..., :3].max() > 0.1
    assert npc.lit_share(frames[1][0]) >= npc.MIN_LIT, npc.lit_share(frames[1][0])      # scatter, shadow rays and accumulation did run


def test_parameters_that_would_never_finish_a_frame_are_refused_by_name(scene):
    """a ray whose direction is NaN in every component passes the slab test (fminf / fmaxf drop NaNs) with t in [0, 1e30] and its DDA never
    advances: a frame that does not end.  A camera at its own focus, an up vector along the view, a NaN field of view, a NaN clipping
    box, a sampling rate without a step: refused on the host, for every rendering mode, before anything is launched"""
    nan = float("nan")
    for frm, at, up, fovy in [((1.0, 2.0, 3.0), (1.0, 2.0, 3.0), (0.0, 1.0, 0.0), 45.0), ((0.0, 0.0, -90.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 45.0),
                              ((0.0, 0.0, -90.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), nan), ((nan, 0.0, -90.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0)]:
        for mode in (5, 6, 14):
            r = make_renderer(scene, scene["sv"], size=(16, 8), mode=mode)
            cam = api.vnrCreateCamera()
            api.vnrCameraSet(cam, frm, at, up, fovy)
            api.vnrRendererSetCamera(r, cam)
            with pytest.raises(api.VnrAmdError, match="degenerate camera"):
                api.vnrRender(r)
    r = make_renderer(scene, scene["sv"], size=(16, 8))
    for rate in (0.0, -1.0, nan, float("inf")):
        with pytest.raises(api.VnrAmdError, match="sampling rate"):
            api.vnrRendererSetVolumeSamplingRate(r, rate)
    api.vnrRendererSetVolumeDensityScale(r, nan)
    with pytest.raises(api.VnrAmdError, match="density"):
        api.vnrRender(r)
    api.vnrRendererSetVolumeDensityScale(r, 1.0)
    api.vnrVolumeSetClippingBox(scene["sv"], (0.0, nan, 0.0), (1.0, 1.0, 1.0))
    try:
        with pytest.raises(api.VnrAmdError, match="clipping box"):
            api.vnrRender(r)
    finally:
        api.vnrVolumeSetClippingBox(scene["sv"], (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    api.vnrRender(r)                                   # and the renderer is still good
    # odd but finite: a field of view of zero, an inverted clipping box, a camera inside the volume looking out
    cam = api.vnrCreateCamera()
    api.vnrCameraSet(cam, (0.0, 0.0, -90.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.0)
    api.vnrRendererSetCamera(r, cam)
    api.vnrRender(r)
    assert np.isfinite(api.vnrRendererMapFrame(r)).all()
