"""The cases of tests/test_gpu_ray_lists.py, shared with the script that recorded their expected digests from the commit before the ray lists were
indexed instead of packed (tests/golden/make_ray_lists_parent.py): small frames whose 64-ray groups are mostly empty from the first march on, rays
that end at different iterations or all live long, the three streaming passes with a ray list of their own (no shading, gradient shading, single
shade heuristic + its shadow pass), with and without a network, with the survivors numbered inside the evaluation kernel and behind it."""
import ctypes as C
import hashlib

import numpy as np

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

DIM = 96
SCENES = ("groundtruth", "neural64", "neural128")   # the kernel of its own, the evaluation kernel's prologue, the kernel of its own (8-wave blocks)
SIZES = ((72, 40), (128, 128))                      # partial 8 x 8 tiles; 256 groups
TFNS = ("opaque", "faint")
MODES = (5, 8, 11)
N_FRAMES = 2
# samples per voxel edge before the adaptive step, which is 13 x the base step where a transfer function is faint: the longest rays of the
# faint cases then take about a hundred samples, a dozen batches of 8
SAMPLING_RATE = 8.0
STAT_KEYS = ("n_samples", "n_reference_slots", "n_iterations", "n_rays_hit")
# a short batch (more iterations, i.e. more turns of the two lists), the coupled loop also for frames small enough for the decoupled one,
# and the seed of the untrained networks
ENV = {"VNR_RM_N_ITERS": "8", "VNR_AMD_DECOUPLED": "0", "VNR_AMD_INIT_SEED": "4242"}


def corner_camera(size):
    """looks past the volume so that it covers one corner of the image, less than 1/8 of it: most 64-ray groups (8 x 8 pixel tiles) are empty
    from the first march on, in runs of many groups"""
    w, h = size
    d = float(DIM)
    dist = 2.5 * d
    half_v = np.tan(np.radians(30.0)) * dist
    half_h = half_v * w / h
    return {"from": (0.0, 0.0, -dist), "at": (float(half_h - 0.2 * d), float(half_v - 0.2 * d), 0.0), "up": (0.0, 1.0, 0.0), "fovy": 60.0}


def transfer_function(kind):
    n = 256
    t = np.linspace(0.0, 1.0, n, dtype=np.float32)
    colors, _ = syn.tfn_ramp_with_bumps(n=n)
    if kind == "opaque":   # nowhere transparent, 0.12 .. 0.62 per step: a ray saturates after 10 .. 50 samples, depending on what it meets
        alphas = (0.12 + 0.5 * np.sin(25.0 * t) ** 2).astype(np.float32)
    else:                  # faint: no ray saturates, every ray lives until it leaves the volume
        alphas = np.full(n, 0.004, np.float32)
    tfn = api.vnrCreateTransferFunction()
    api.vnrTransferFunctionSetColor(tfn, colors)
    api.vnrTransferFunctionSetAlpha(tfn, alphas)
    api.vnrTransferFunctionSetValueRange(tfn, (0, 1))
    return tfn


def make_volume(kind, sv):
    """`sv`: the 96^3 ground truth; the networks are untrained (VNR_AMD_INIT_SEED, read when the volume is created)"""
    if kind == "groundtruth":
        return sv
    cfg = syn.model_config(n_levels=4, n_features=2, log2_hashmap_size=12, base_resolution=4, n_neurons=64 if kind == "neural64" else 128,
                           n_hidden_layers=2)
    return api.vnrCreateNeuralVolume(cfg, sv, online_macrocell_construction=False)


def render(volume, tfn, size, mode, pipelined):
    """N_FRAMES accumulated frames of a fresh renderer -> (frames, statistics of the last, schedule of the last)"""
    from instantvnr_amd._lib import check, lib
    cam = corner_camera(size)
    camera = api.vnrCreateCamera()
    api.vnrCameraSet(camera, cam["from"], cam["at"], cam["up"], cam["fovy"])
    r = api.vnrCreateRenderer(volume)
    api.vnrRendererSetTransferFunction(r, tfn)
    api.vnrRendererSetCamera(r, camera)
    api.vnrRendererSetFramebufferSize(r, size)
    api.vnrRendererSetMode(r, mode)
    api.vnrRendererSetVolumeSamplingRate(r, SAMPLING_RATE)
    frames = []
    if not pipelined:
        for _ in range(N_FRAMES):
            api.vnrRender(r)
            frames.append(api.vnrRendererMapFrame(r).copy())
    else:
        api.vnrRendererSetOutputAsDeviceFramebuffer(r, True)
        out = C.c_void_p()

        def grab(ptr):
            a = np.empty((size[1], size[0], 4), np.float32)
            check(lib().vnrAmdMemcpyD2H(a.ctypes.data_as(C.c_void_p), ptr, a.nbytes))
            return a
        for k in range(N_FRAMES):
            check(lib().vnrAmdRendererRenderPipelined(r.h, C.byref(out)))
            if k:
                frames.append(grab(out))
        check(lib().vnrAmdRendererFlushPipeline(r.h, C.byref(out)))
        frames.append(grab(out))
    st = api.vnrRendererGetFrameStats(r)
    return frames, {k: int(st[k]) for k in STAT_KEYS}, api.renderer_schedule(r)


def digest(frames):
    h = hashlib.sha256()
    for f in frames:
        h.update(np.ascontiguousarray(f, dtype=np.float32).tobytes())
    return h.hexdigest()


def case_id(scene, size, tfn, mode):
    return f"{scene}-{size[0]}x{size[1]}-{tfn}-mode{mode}"
