"""The model and the points of tests/test_gpu_eval_five_waves.py, shared with the recorder of its stored outputs
(tests/golden/make_eval_five_waves_parent.py).

One small model whose levels take all three paths of the evaluation kernel's encode (csrc/grid_device.h): L 8, F 2, 2^12 entries per hashed
level, base resolution 4, per_level_scale 1.5: resolutions 4, 6, 9, 14 (dense) and 21, 31, 46, 69 (hashed; read from the brick image when
there is one).  64 neurons, 2 hidden layers: the instance family of the bench model (F 2, 64 neurons, common kind)."""
import numpy as np

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

L, F, LOG2_T, BASE, PLS, NEURONS, HIDDEN = 8, 2, 12, 4, 1.5, 64, 2
PADDED_WIDTH = 16
N_MLP = NEURONS * PADDED_WIDTH + (HIDDEN - 1) * NEURONS * NEURONS + 16 * NEURONS   # first, hidden, last (16 padded rows)
PARAM_SEED, POINT_SEED = 808, 809
BIG_LAUNCH = 1 << 20   # samples of a launch that counts as a frame for the small tier of the brick image (csrc/brick_policy.h kSmallMinLaunch)


def make_volume():
    cfg = syn.model_config(n_levels=L, n_features=F, log2_hashmap_size=LOG2_T, base_resolution=BASE, n_neurons=NEURONS,
                           n_hidden_layers=HIDDEN, per_level_scale=PLS)
    vol = api.vnrCreateNeuralVolume(cfg, (64, 64, 64))
    info = api.neural_info(vol)
    assert info["padded_width"] == PADDED_WIDTH and info["n_neurons"] == NEURONS and info["n_params"] > N_MLP, info
    api.neural_set_params_fp16(vol, syn.random_params(info["n_params"], N_MLP, seed=PARAM_SEED))
    return vol


def points():
    """4 096 uniform points, the 27 points of {0, 0.5, 1}^3 (the domain's faces: a wave with one of them leaves the brick path and the dense fast
    path for the exact index arithmetic) and 256 points with one, two or three coordinates on a cell face of the finest level"""
    rng = np.random.default_rng(POINT_SEED)
    uniform = rng.uniform(0.0, 1.0, (4096, 3)).astype(np.float32)
    g = np.array([0.0, 0.5, 1.0], dtype=np.float32)
    corners = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    scale = np.float32(np.exp2(np.float32(L - 1) * np.log2(np.float32(PLS))) * BASE - 1.0)   # the finest level's (grid_make_layout)
    res = int(np.ceil(scale)) + 1
    faces = rng.uniform(0.0, 1.0, (256, 3)).astype(np.float32)
    k = rng.integers(1, res - 1, (256, 3)).astype(np.float32)
    on_face = rng.integers(1, 8, 256)   # bit d: coordinate d sits on a face (x scale + 0.5 is a whole number, up to rounding)
    for d in range(3):
        sel = (on_face >> d & 1) == 1
        faces[sel, d] = ((k[sel, d] - np.float32(0.5)) / scale).astype(np.float32)
    out = np.concatenate([uniform, corners, faces]).astype(np.float32)
    assert out.shape == (4096 + 27 + 256, 3) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    return out


def big_launch_points():
    """a launch large enough to count as a frame (values do not matter)"""
    return np.random.default_rng(POINT_SEED + 1).uniform(0.0, 1.0, (BIG_LAUNCH, 3)).astype(np.float32)
