"""Neural models on which path tracing (rendering modes 14 / 15) has something to show, for the tests that hold the two path-tracing kernels
to the oracle (tests/test_gpu_neural_path_tracing.py) and to each other (tests/test_gpu_render.py, tests/test_gpu_fuzz.py).

The transfer function of the render scene is transparent below 0.15 and a network with seeded random parameters answers around 0 (or one
constant) for most seeds: every collision is a null collision, the frame is black, and a comparison of two black frames says nothing about
scatter, shadow rays or the accumulation of radiance.  Every case here names a parameter seed and a scale of the MLP weights that were
searched on the host, with the oracle alone, until the oracle's own path-traced frame is lit and the network's value varies in space;
tests/test_neural_pt_cases_host.py asserts both for every case, so a case that stops being lit fails there, without a GPU."""
import numpy as np

from instantvnr_amd import synthetic as syn

INTERPOLATIONS = {"Linear": 0, "Smoothstep": 1, "Nearest": 2}

# the frame every path-tracing comparison renders: the scene of tests/test_gpu_render.py in small
SIZE = (64, 48)
VOLUME_N = 48
DENSITY_SCALE = 0.5
MIN_LIT = 0.10          # share of pixels with non-zero radiance in the reference frame (frame 1)
MIN_VALUE_SPREAD = 0.3  # q95 - q05 of the network's values on 4000 uniform coordinates


def _case(L, F, H, seed, mlp_scale=1.0, W=64, log2T=14, base=4, pls=1.4, act="ReLU", out_act="None", interp="Linear", gtype="Hash", qt=0.0):
    return dict(L=L, F=F, H=H, W=W, log2T=log2T, base=base, pls=pls, act=act, out_act=out_act, interp=interp, gtype=gtype, qt=qt, seed=seed,
                mlp_scale=mlp_scale)


# every FullyFusedMLP width the reference's in-shader dispatch instantiates (16 / 32 / 64, method_raymarching.cu:1192-1244; 128, refused
# there at :1210, comes with the template here) and models of the GENERAL kind (grid_device.h), F = 1 .. 8.  The narrow networks sum few
# terms per neuron and need larger weights than U(-0.35, 0.35) to leave the neighbourhood of 0 (MLP_SCALE_BY_WIDTH); Sigmoid hidden layers
# answer in (0, 1), so the Sigmoid-then-Exponential model needs large weights for its exponent to move at all.
MLP_SCALE_BY_WIDTH = {16: 2.0, 32: 1.5, 64: 1.0, 128: 0.75}

IN_SHADER_MODELS = {
    "w16": _case(16, 2, 3, seed=41, mlp_scale=2.0, W=16),
    "w32": _case(16, 2, 3, seed=77, mlp_scale=1.5, W=32),
    "w128": _case(8, 4, 2, seed=0, mlp_scale=0.75, W=128),
    "w16-f1": _case(16, 1, 2, seed=77, mlp_scale=2.0, W=16),
    "w32-f8": _case(8, 8, 2, seed=41, mlp_scale=1.5, W=32),
    "w64-sigmoid-exp": _case(8, 2, 2, seed=45, mlp_scale=3.0, act="Sigmoid", out_act="Exponential"),
    "w32-nearest-quantized": _case(16, 2, 2, seed=5, mlp_scale=1.5, W=32, interp="Nearest", qt=0.05),
    "w16-tiled-smoothstep": _case(8, 4, 3, seed=41, mlp_scale=2.0, W=16, gtype="Tiled", interp="Smoothstep", act="Squareplus"),
}

CASES = {
    # BASELINE C4 model shape (T = 2^19): F = 2, paired 8-byte loads, 3 hidden layers
    "c4": _case(16, 2, 3, seed=77, log2T=19, base=16, pls=1.3195),
    **IN_SHADER_MODELS,
    # the (F, padded encoded width) pairs of VNR_IN_SHADER_SHAPES that no model above reaches; per_level_scale keeps the finest level < 512
    "f1-k32": _case(20, 1, 2, seed=77, pls=1.25),     # (1, 32): 4 x 1.25^19 = 277
    "f2-k64": _case(28, 2, 2, seed=5, pls=1.18),     # (2, 64): 4 x 1.18^27 = 349
    "f4-k64": _case(14, 4, 2, seed=5, pls=1.4),      # (4, 64): 4 x 1.4^13 = 317
    "f8-k128": _case(16, 8, 2, seed=0, pls=1.35),    # (8, 128): 4 x 1.35^15 = 361 (15 or 16 levels: 13 and 14 pad to 112)
}
GENERAL_CASE = "w32-nearest-quantized"   # the GENERAL kind that the end-to-end test takes beside "c4"


def model_config(case):
    cfg = syn.model_config(n_levels=case["L"], n_features=case["F"], log2_hashmap_size=case["log2T"], base_resolution=case["base"],
                           n_hidden_layers=case["H"], per_level_scale=case["pls"], n_neurons=case["W"])
    cfg["network"]["activation"] = case["act"]
    cfg["network"]["output_activation"] = case["out_act"]
    cfg["encoding"]["interpolation"] = case["interp"]
    if case["gtype"] != "Hash":
        cfg["encoding"]["type"] = case["gtype"]
    if case["qt"]:
        cfg["encoding"]["quantize_threshold"] = case["qt"]
    return cfg


def grid_config(oracle, case):
    return oracle.grid_config(case["L"], case["F"], case["log2T"], case["base"], case["pls"], INTERPOLATIONS[case["interp"]], case["qt"],
                              grid_type=case["gtype"])


def parameters(oracle, case, seed=None, mlp_scale=None):
    """the seeded fp16 parameter blob of a case (MLP weights first, then the grid), sized by the oracle's own layout"""
    ocfg = grid_config(oracle, case)
    n_mlp = oracle.mlp_n_params(oracle.padded_width(ocfg), case["W"], case["H"] - 1)
    return syn.random_params(oracle.n_params(ocfg, case["W"], case["H"]), n_mlp, seed=case["seed"] if seed is None else seed,
                             mlp_scale=case["mlp_scale"] if mlp_scale is None else mlp_scale)


def oracle_network(oracle, case, params, acc_mode=0):
    """the oracle's network on a case's parameters, as the value function of its renderers"""
    ocfg = grid_config(oracle, case)
    code = oracle.act_code(case["act"], case["out_act"])
    return lambda c: oracle.network_inference(ocfg, case["W"], case["H"], params.view(np.uint16), c, activation=code, acc_mode=acc_mode)


class HostScene:
    """the render scene of tests/test_gpu_render.py on the host: volume, transfer function, camera, and the ground-truth macrocell's majorants
    from the oracle (the library's are the same bits: test_macrocell_bit_exact)"""

    def __init__(self, oracle, distance_scale=1.6):
        self.vol = syn.analytic_volume(VOLUME_N)
        self.colors, self.alphas = syn.tfn_ramp_with_bumps()
        self.cam = syn.oblique_camera((VOLUME_N,) * 3, distance_scale)
        self.otfn = oracle.TfnHolder(self.colors, self.alphas)
        self.max_opacity = oracle.macrocell_max_opacity(self.otfn, oracle.macrocell_compute_implicit(self.vol))

    def holder(self, oracle, mode=14, frame_index=1, density_scale=DENSITY_SCALE, size=SIZE):
        """the oracle's scene for rendering mode 14 (shading_mode 0) or 15 (shading_mode 5: interval reset and ambient term after a bounce)"""
        cam = self.cam
        return oracle.SceneHolder(size[0], size[1], (VOLUME_N,) * 3, self.otfn, self.max_opacity, cam["from"], cam["at"], cam["up"], cam["fovy"],
                                  frame_index=frame_index, density_scale=density_scale, shading_mode=5 if mode == 15 else 0)


def lit_share(frame):
    """share of pixels with non-zero radiance"""
    return float((frame[..., :3].sum(axis=-1) > 0).mean())


def value_spread(values):
    q05, q95 = np.quantile(values, [0.05, 0.95])
    return float(q95 - q05)
