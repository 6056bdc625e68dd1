"""Deterministic training (vnrAmdNeuralVolumeSetDeterministicTraining): the hash-grid part of the gradient summed in 64-bit
fixed point, the same bits whatever order the scatter's atomics arrive in.

The exact sum is the float64 scatter of the library's OWN dL/dfeatures (vnrAmdNeuralVolumeTrainingBuffer 1) over the corners and weights of
oracle.train_oracle.corner_indices_and_weights.  Per entry the deterministic result must lie within

    1 fp16 ulp + n_adds * 2^-(e+1) + 2^-24 * sum |terms|

of fp16(exact): one rounding of the sum to half, one rounding per fixed-point term (e = floor(62 - log2(8 n M)), M = max |dL/dfeature| over
the batch and the active levels' columns), and the fp32 rounding of each product w * g (which matters only where terms cancel)."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTERP = {"Linear": 0, "Smoothstep": 1, "Nearest": 2}


@pytest.fixture(autouse=True)
def _mode_default_off(monkeypatch):
    monkeypatch.delenv("VNR_AMD_DETERMINISTIC", raising=False)
    monkeypatch.delenv("VNR_AMD_TRAIN_OVERLAP", raising=False)


training_buffer = api.neural_training_buffer          # (vol, which, dtype) -> what the last ForwardBackward kept, downloaded


def blob(vol):
    """the fp16 gradient blob as it is on the device (loss-scaled)"""
    return training_buffer(vol, 0, np.float16)


def rescatter(vol, coords):
    d = api.DeviceArray.from_numpy(np.ascontiguousarray(coords, np.float32))
    api.check(api.lib().vnrAmdNeuralVolumeRescatterGridGradients(vol.h, coords.shape[0], d.ptr))
    api.check(api.lib().vnrAmdSynchronize())


def make_model(oracle, L, F, log2T, base, pls=2.0, interp="Linear", gtype="Hash", max_level=None, W=64, H=2, seed=0):
    cfg = syn.model_config(n_levels=L, n_features=F, log2_hashmap_size=log2T, base_resolution=base, n_hidden_layers=H, per_level_scale=pls)
    cfg["network"]["n_neurons"] = W
    cfg["encoding"]["interpolation"] = interp
    if gtype != "Hash":
        cfg["encoding"]["type"] = gtype
    if max_level is not None:
        cfg["encoding"]["max_level"] = max_level
    vol = api.vnrCreateNeuralVolume(cfg, (32, 32, 32))
    info = api.neural_info(vol)
    ocfg = oracle.grid_config(L, F, log2T, base, pls, INTERP[interp], 0.0, 1000.0 if max_level is None else max_level, gtype)
    n_mlp = oracle.mlp_n_params(info["padded_width"], W, H - 1)
    params = syn.random_params(info["n_params"], n_mlp, seed=seed)
    api.neural_set_params_fp16(vol, params)
    return vol, ocfg, info, n_mlp, params


def batch(n, seed, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, (n, 3)).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)


def exact_scatter(oracle, ocfg, dfeat, coords, exclude=None):
    """float64 sum, sum of |terms| and number of nonzero terms per grid element (tcnn order: level by level, entry-major, F features);
    exclude = (level, first sample, last sample): leave that unit out of the sum"""
    from oracle import train_oracle as T
    lay = oracle.grid_layout(ocfg)
    F = ocfg.n_features
    n_el = int(lay["offsets"][ocfg.n_levels]) * F
    S, A, K = np.zeros(n_el), np.zeros(n_el), np.zeros(n_el)
    for l, (idx, w) in enumerate(T.corner_indices_and_weights(ocfg, lay, coords)):
        base = int(lay["offsets"][l]) * F
        for f in range(F):
            g = dfeat[:, l * F + f].astype(np.float32)
            t = (w * g[:, None]).astype(np.float64)          # the fp32 product would differ by at most 2^-24 |t|: the bound's last term
            if exclude is not None and exclude[0] == l:
                t[exclude[1]:exclude[2]] = 0.0
            el = base + idx.ravel() * F + f
            S += np.bincount(el, weights=t.ravel(), minlength=n_el)
            A += np.bincount(el, weights=np.abs(t).ravel(), minlength=n_el)
            K += np.bincount(el, weights=(t != 0).ravel().astype(np.float64), minlength=n_el)
    return S, A, K, lay


def exponent(dfeat, n_cols):
    """the library's e: floor(62 - log2(8 n M)) from M = max |dL/dfeature| over the active columns; None when M = 0"""
    M = float(np.abs(dfeat[:, :n_cols].astype(np.float64)).max()) if n_cols else 0.0
    if M == 0.0:
        return None
    f, k = math.frexp(8.0 * dfeat.shape[0] * M)
    return 62 - (k - 1 if f == 0.5 else k)


def ulp16(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float16)).astype(np.float64)


def deterministic_bound(S, A, K, e):
    return ulp16(S) + K * 2.0 ** -(e + 1) + 2.0 ** -24 * A


def check_exact(got, S, A, K, e, what):
    want = S.astype(np.float16).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want)
    bound = np.maximum(deterministic_bound(S, A, K, e), ulp16(got))
    bad = np.nonzero(err > bound)[0]
    assert bad.size == 0, (what, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist(), bound[bad[:8]].tolist())


EXACT_CASES = [
    # (name, model kwargs, batch, coordinate range)
    ("F1 hash linear", dict(L=6, F=1, log2T=12, base=4), 2048, (0.0, 1.0)),
    ("F2 hash smoothstep", dict(L=8, F=2, log2T=13, base=4, pls=1.5, interp="Smoothstep"), 2048, (0.0, 1.0)),
    ("F4 dense linear", dict(L=3, F=4, log2T=14, base=4, pls=2.0, gtype="Dense"), 2048, (0.0, 1.0)),
    ("F8 tiled nearest", dict(L=4, F=8, log2T=11, base=6, pls=1.5, gtype="Tiled", interp="Nearest"), 2048, (0.0, 1.0)),
    ("F2 max_level", dict(L=8, F=2, log2T=12, base=4, pls=1.5, max_level=3.5), 2048, (0.0, 1.0)),
    ("F2 outside [0,1]", dict(L=6, F=2, log2T=12, base=4, pls=1.5), 2048, (-0.3, 1.3)),
    ("F4 ragged 1000", dict(L=6, F=4, log2T=12, base=3, pls=1.5, interp="Smoothstep"), 1000, (0.0, 1.0)),
    ("example model L8 F8 T2^19 4x64", dict(L=8, F=8, log2T=19, base=16, pls=2.0, H=4), 2048, (0.0, 1.0)),
]


@pytest.mark.parametrize("name,kw,n,rng_", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_deterministic_grid_gradient_is_the_exact_sum(oracle, name, kw, n, rng_):
    vol, ocfg, info, n_mlp, _ = make_model(oracle, seed=3, **kw)
    api.neural_set_deterministic_training(vol, True)
    coords, targets = batch(n, 7, *rng_)
    g = api.neural_forward_backward(vol, coords, targets)
    dfeat = training_buffer(vol, 1, np.float16).reshape(n, info["padded_width"])
    n_active = ocfg.n_levels if kw.get("max_level") is None else sum(1 for l in range(ocfg.n_levels) if l < kw["max_level"] + 1e-3)
    e = exponent(dfeat, n_active * ocfg.n_features)
    assert e is not None
    S, A, K, _ = exact_scatter(oracle, ocfg, dfeat, coords)
    assert np.abs(S).max() > 0
    check_exact(g[n_mlp:], S, A, K, e, name)
    assert not training_buffer(vol, 4, np.int64).any(), "the int64 image is zero after the fold"


def test_lds_tiles_of_a_65536_sample_batch_give_the_exact_sum(oracle):
    kw = dict(L=6, F=2, log2T=15, base=8, pls=1.5)
    vol, ocfg, info, n_mlp, _ = make_model(oracle, seed=5, **kw)
    api.neural_set_deterministic_training(vol, True)
    plan = api.neural_grid_backward_plan(vol, 65536)
    assert plan["lds_levels"] >= 2 and plan["tile_entries"] == (24 * 1024 // (8 * 2)) & ~15, plan
    coords, targets = batch(65536, 11)
    g = api.neural_forward_backward(vol, coords, targets)
    dfeat = training_buffer(vol, 1, np.float16).reshape(65536, info["padded_width"])
    S, A, K, _ = exact_scatter(oracle, ocfg, dfeat, coords)
    check_exact(g[n_mlp:], S, A, K, exponent(dfeat, 6 * 2), "lds 65536")


# ------------------------------------------------------------------------------------------------ every form of the scatter, every F
# One model per F on which a step takes all three kinds of level: dense levels through LDS tiles, a dense level with more than 64 tiles
# (global atomics on a dense index) and a hashed level; 8 192 samples, the smallest batch at which VNR_AMD_TRAIN_OVERLAP=1 takes the
# persistent forms.  Production and deterministic mode, one stream and side by side: the six kernel forms of that F in one case.
ALL_FORMS_MODELS = {1: dict(L=6, F=1, log2T=19, base=5), 2: dict(L=6, F=2, log2T=18, base=4), 4: dict(L=5, F=4, log2T=17, base=6),
                    8: dict(L=5, F=8, log2T=16, base=5)}
ALL_FORMS_BATCH = 8192


def _faces_and_just_outside(coords):
    """the domain's faces and corners, and values just outside [0, 1], in the first rows (the LDS kernels' early drop must keep them)"""
    eps = np.float32(2.0 ** -20)
    lo, hi = np.nextafter(np.float32(0), np.float32(-1)), np.nextafter(np.float32(1), np.float32(2))
    special = [(0, 0, 0), (1, 1, 1), (1, 0, 0.5), (0.5, 1, 0), (0, 0.25, 1), (lo, lo, lo), (hi, hi, hi), (-eps, 0.5, 0.5), (0.5, 1 + eps, 0.5),
               (0.5, 0.5, -1e-3), (0.3, 0.7, 1.001), (1.001, -1e-3, 1), (0, hi, lo), (1 - eps, 1 - eps, 1 - eps)]
    coords[:len(special)] = np.array(special, np.float32)
    return coords


@pytest.mark.parametrize("interp", ["Linear", "Smoothstep", "Nearest"])
@pytest.mark.parametrize("F", [1, 2, 4, 8])
def test_every_form_of_the_scatter_gives_the_exact_sum_or_stays_within_the_production_bound(oracle, monkeypatch, F, interp):
    kw = ALL_FORMS_MODELS[F]
    n = ALL_FORMS_BATCH
    vol, ocfg, info, n_mlp, params = make_model(oracle, seed=40 + F, interp=interp, **kw)
    levels = api.neural_level_table(vol)
    plans = {}
    for det in (False, True):                                 # the model is chosen by what the library plans for it, in either mode
        api.neural_set_deterministic_training(vol, det)
        plan = plans[det] = api.neural_grid_backward_plan(vol, n)
        assert plan["n_levels"] == kw["L"] and 1 <= plan["lds_levels"] < plan["n_levels"], plan
        assert levels[plan["lds_levels"]]["kind"] == 0, ("a dense level beyond the LDS levels", plan, levels)
        assert any(lv["kind"] == 1 for lv in levels[plan["lds_levels"]:]), ("a hashed level", levels)
    coords, targets = batch(n, 50 + F)
    coords = _faces_and_just_outside(coords)

    def run(det, overlap):
        api.neural_set_deterministic_training(vol, det)
        monkeypatch.setenv("VNR_AMD_TRAIN_OVERLAP", "1" if overlap else "0")
        api.neural_forward_backward(vol, coords, targets)
        g = blob(vol)[n_mlp:info["n_params"]].copy()
        dfeat = training_buffer(vol, 1, np.float16).reshape(n, info["padded_width"]).copy()
        api.neural_train_end(vol, grad_scale=0.0)            # clears the blob for the next run ...
        api.neural_set_params_fp16(vol, params)                # ... and the same parameters again
        return g, dfeat

    det_one, dfeat = run(True, False)
    S, A, K, lay = exact_scatter(oracle, ocfg, dfeat, coords)
    e = exponent(dfeat, kw["L"] * F)
    assert e is not None and np.abs(S).max() > 0
    check_exact(det_one, S, A, K, e, ("deterministic, one stream", F, interp))
    det_side, dfeat2 = run(True, True)
    assert np.array_equal(dfeat2.view(np.uint16), dfeat.view(np.uint16))
    assert np.array_equal(det_side.view(np.uint16), det_one.view(np.uint16)), ("side by side", F, interp, int((det_side != det_one).sum()))
    assert not training_buffer(vol, 4, np.int64).any(), "the int64 image is zero after the fold"
    bound = production_bound(S, A, K, F, _lds_slices_per_element(vol, plans[False], lay, F, S.size))
    for overlap in (False, True):
        prod, dfeat3 = run(False, overlap)
        assert np.array_equal(dfeat3.view(np.uint16), dfeat.view(np.uint16))
        err = np.abs(prod.astype(np.float64) - S)
        assert (err <= bound).all(), ("production", "side by side" if overlap else "one stream", F, interp, np.nonzero(err > bound)[0][:8].tolist())


# ------------------------------------------------------------------------------------------------ bit-reproducible training
def _train_run(cfg, params, steps, overlap, per_step_params):
    os.environ["VNR_AMD_TRAIN_OVERLAP"] = "1" if overlap else "0"
    try:
        sv = api.vnrCreateSimpleVolume(syn.analytic_volume(32))   # (a fresh ground truth: its sampler starts at the same offset)
        vol = api.vnrCreateNeuralVolume(cfg, sv, online_macrocell_construction=False)
        api.neural_set_params_fp16(vol, params)
        api.neural_set_deterministic_training(vol, True)
        losses, snaps = [], []
        for s in range(steps):
            api.vnrNeuralVolumeTrain(vol, 1, True)
            losses.append(api.vnrNeuralVolumeGetTrainingLoss(vol))
            if per_step_params(s):
                snaps.append(api.neural_get_params_fp16(vol).view(np.uint16).copy())
        return np.array(losses, np.float64), snaps
    finally:
        os.environ.pop("VNR_AMD_TRAIN_OVERLAP", None)


@pytest.mark.parametrize("shape", ["F2 hash", "example model"])
def test_training_is_bit_reproducible_with_and_without_overlap(shape):
    if shape == "F2 hash":
        cfg = syn.model_config(n_levels=8, n_features=2, log2_hashmap_size=14, base_resolution=4, n_hidden_layers=2, per_level_scale=1.5)
        every = lambda s: True                                  # noqa: E731  (small: the parameter bytes after every step)
    else:
        cfg = syn.model_config(n_levels=8, n_features=8, log2_hashmap_size=19, base_resolution=16, n_hidden_layers=4)
        every = lambda s: s % 50 == 49                          # noqa: E731  (33 M parameters: every 50th step, and the loss of every step)
    init = api.vnrCreateNeuralVolume(cfg, (32, 32, 32))
    params = api.neural_get_params_fp16(init).view(np.uint16).copy()
    a = _train_run(cfg, params, 200, False, every)
    b = _train_run(cfg, params, 200, False, every)
    c = _train_run(cfg, params, 200, True, every)
    assert np.isfinite(a[0]).all() and a[0][-1] < a[0][0]
    for other, what in ((b, "a second run"), (c, "VNR_AMD_TRAIN_OVERLAP=1")):
        assert np.array_equal(a[0].view(np.uint64), other[0].view(np.uint64)), (what, np.nonzero(a[0] != other[0])[0][:5])
        assert len(a[1]) == len(other[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], other[1])), what
    assert not np.array_equal(a[1][-1], params), "training moved the parameters"


# ------------------------------------------------------------------------------------------------ tripwire for the production scatter
def production_bound(S, A, K, F, lds_slices):
    """worst case of the production scatter against the exact sum, per element.  Atomic (hashed and fine dense) levels, F >= 2: each of the
    element's K terms is rounded to half (<= 2^-11 |t|) and each packed fp16 add rounds the running sum (<= 2^-11 of at most sum |t|), with
    the subnormal floor of half an fp16 ulp (2^-25) per operation.  F = 1: fp32 adds into the float image (<= 2^-24 sum |t| each: the terms,
    and on LDS levels the slices' flushes, at most as many again) and one rounding to half.  LDS levels, F >= 2: fp32 LDS adds, then per
    batch slice that touched the element (its tile's slices: one fp16 add per slice, not one per sample) a rounding of the slice's sum to half
    and a packed fp16 add."""
    u = 2.0 ** -11
    if F == 1:
        return 2 * K * 2.0 ** -24 * A + ulp16(S) + 2.0 ** -25
    n16 = np.where(lds_slices > 0, np.minimum(lds_slices, K), K)          # fp16 adds of the element
    n_round = 2 * n16                                                      # ... and as many roundings of what they add
    return n_round * (u * A + 2.0 ** -25) + K * 2.0 ** -24 * A + ulp16(S)


def _lds_slices_per_element(vol, plan_prod, lay, F, n_el):
    """batch slices of each element's tile on the production LDS levels (network_train.hip scatter_grid_gradients); 0 elsewhere"""
    out = np.zeros(n_el)
    levels = api.neural_level_table(vol)
    for l in range(plan_prod["lds_levels"]):
        tiles = -(-levels[l]["entries"] // plan_prod["tile_entries"])
        slices = max(4, min(128, plan_prod["lds_blocks"] // tiles))
        out[int(lay["offsets"][l]) * F:int(lay["offsets"][l + 1]) * F] = slices
    return out


def test_production_scatter_stays_within_its_worst_case_on_random_models(oracle):
    rng = np.random.default_rng(2024)
    caught = 0                                                # draws whose finest hashed level had a unit to lose (each one must be caught)
    for draw in range(20):
        F = int(rng.choice([1, 2, 4, 8]))
        gtype = str(rng.choice(["Hash", "Hash", "Dense", "Tiled"]))
        L = int(rng.integers(2, 4 if gtype == "Dense" else 9))
        kw = dict(L=L, F=F, log2T=int(rng.integers(10, 15)), base=int(rng.integers(2, 9)), pls=float(rng.choice([1.3, 1.5, 2.0])),
                  interp=str(rng.choice(["Linear", "Smoothstep", "Nearest"])), gtype=gtype)
        vol, ocfg, info, n_mlp, _ = make_model(oracle, seed=100 + draw, **kw)
        n = int(rng.choice([1000, 2048, 4096]))
        coords, targets = batch(n, 200 + draw)
        plan_prod = api.neural_grid_backward_plan(vol, n)
        prod = api.neural_forward_backward(vol, coords, targets)[n_mlp:].astype(np.float64)
        dfeat = training_buffer(vol, 1, np.float16).reshape(n, info["padded_width"])
        api.neural_set_deterministic_training(vol, True)
        rescatter(vol, coords)
        det = blob(vol)[n_mlp:info["n_params"]].astype(np.float64)
        S, A, K, lay = exact_scatter(oracle, ocfg, dfeat, coords)
        e = exponent(dfeat, L * F)
        check_exact(det, S, A, K, e, ("deterministic", draw, kw))
        bound = production_bound(S, A, K, F, _lds_slices_per_element(vol, plan_prod, lay, F, S.size))
        err = np.abs(prod - S)
        assert (err <= bound).all(), ("production", draw, kw, np.nonzero(err > bound)[0][:8].tolist())
        # the bound is tight enough to see a (level, 64-sample) unit lost on a hashed level: take one out of the exact result, in numpy
        hashed = [l for l, lv in enumerate(api.neural_level_table(vol)) if lv["kind"] == 1]
        if hashed:
            l = hashed[-1]
            s0 = 64 * int(rng.integers(0, n // 64))
            S2, _, _, _ = exact_scatter(oracle, ocfg, dfeat, coords, exclude=(l, s0, s0 + 64))
            lost = S2.astype(np.float16).astype(np.float64)
            if np.abs(S2 - S).max() > 0:
                assert (np.abs(lost - S) > bound).any(), ("a lost unit passes the production bound", draw, kw)
                caught += 1
    assert caught >= 3


def test_mlp_gradient_and_loss_do_not_depend_on_the_mode(oracle):
    kw = dict(L=8, F=2, log2T=13, base=4, pls=1.5)
    a, _, info, n_mlp, params = make_model(oracle, seed=9, **kw)
    b = make_model(oracle, seed=9, **kw)[0]
    api.neural_set_deterministic_training(b, True)
    coords, targets = batch(4096, 13)
    api.neural_forward_backward(a, coords, targets)
    api.neural_forward_backward(b, coords, targets)
    assert np.array_equal(blob(a)[:n_mlp].view(np.uint16), blob(b)[:n_mlp].view(np.uint16))
    la, lb = api.vnrNeuralVolumeGetTrainingLoss(a), api.vnrNeuralVolumeGetTrainingLoss(b)
    assert np.float64(la).view(np.uint64) == np.float64(lb).view(np.uint64), (la, lb)


def test_micro_batches_accumulate_to_the_same_bits(oracle):
    kw = dict(L=6, F=4, log2T=12, base=4, pls=1.5)
    vols = [make_model(oracle, seed=21, **kw) for _ in range(2)]
    coords, targets = batch(2048, 17)
    blobs = []
    for vol, ocfg, info, n_mlp, _ in vols:
        api.neural_set_deterministic_training(vol, True)
        api.neural_forward_backward(vol, coords, targets)
        assert not training_buffer(vol, 4, np.int64).any()
        api.neural_forward_backward(vol, coords, targets)
        assert not training_buffer(vol, 4, np.int64).any()
        blobs.append(blob(vol))
    assert np.array_equal(blobs[0].view(np.uint16), blobs[1].view(np.uint16))
    vol, ocfg, info, n_mlp, _ = vols[0]
    dfeat = training_buffer(vol, 1, np.float16).reshape(2048, info["padded_width"])
    S, A, K, _ = exact_scatter(oracle, ocfg, dfeat, coords)
    e = exponent(dfeat, 6 * 4)
    got = blobs[0][n_mlp:info["n_params"]].astype(np.float64)
    want = (2 * S).astype(np.float16).astype(np.float64)
    bound = 2 * ulp16(2 * S) + 2 * (K * 2.0 ** -(e + 1) + 2.0 ** -24 * A)
    assert (np.abs(got - want) <= bound).all()
    api.neural_train_end(vol)
    assert not blob(vol).view(np.uint16)[n_mlp:info["n_params"]].any(), "TrainEnd clears the grid part of the blob"


def test_mode_is_off_by_default_set_by_the_environment_and_switches_back(oracle):
    kw = dict(L=6, F=2, log2T=15, base=8, pls=1.5)
    vol = make_model(oracle, **kw)[0]
    assert api.neural_get_deterministic_training(vol) is False
    prod = api.neural_grid_backward_plan(vol, 65536)
    api.neural_set_deterministic_training(vol, True)
    assert api.neural_get_deterministic_training(vol) is True
    det = api.neural_grid_backward_plan(vol, 65536)
    assert det["tile_entries"] == prod["tile_entries"] // 2 and det["atomic_requests"] > 0
    api.neural_set_deterministic_training(vol, False)
    assert api.neural_grid_backward_plan(vol, 65536) == prod
    child = ("import sys; sys.path.insert(0, %r)\n"
             "from instantvnr_amd import api, synthetic as syn\n"
             "v = api.vnrCreateNeuralVolume(syn.model_config(n_levels=4, n_features=2, log2_hashmap_size=12, base_resolution=4), (16, 16, 16))\n"
             "print('MODE', int(api.neural_get_deterministic_training(v)))\n" % ROOT)
    env = dict(os.environ, VNR_AMD_DETERMINISTIC="1")
    out = subprocess.run([sys.executable, "-c", child], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "MODE 1" in out.stdout, out.stdout + out.stderr


def test_all_zero_feature_gradients_leave_the_grid_part_untouched(oracle):
    kw = dict(L=6, F=2, log2T=12, base=4, pls=1.5)
    vol, ocfg, info, n_mlp, params = make_model(oracle, **kw)
    params = params.copy()
    params[:n_mlp] = 0                                   # no weights: dL/dfeatures = W1^T d = 0
    api.neural_set_params_fp16(vol, params)
    api.neural_set_deterministic_training(vol, True)
    coords, targets = batch(2048, 19)
    api.neural_forward_backward(vol, coords, targets)
    assert not training_buffer(vol, 1, np.uint16).any()
    assert not blob(vol).view(np.uint16)[n_mlp:info["n_params"]].any()
    assert not training_buffer(vol, 4, np.int64).any()


# ------------------------------------------------------------------------------------------------ two ranks over shm
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch_two_ranks(tmp_path, tag):
    worker = os.path.join(ROOT, "tests", "dist_deterministic_worker.py")
    port = _free_port()
    procs, outs = [], []
    for rank in range(2):
        env = dict(os.environ)
        env.update({"RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": "2", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                    "VNR_AMD_DIST_TRANSPORT": "shm", "VNR_AMD_DIST_TIMEOUT": "120", "VNR_AMD_DIST_FORCE": "1", "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
        out = str(tmp_path / f"det_{tag}_{rank}.npz")
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, worker, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=240)[0].decode("utf-8", "replace"))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for rank, (p, log) in enumerate(zip(procs, logs)):
        assert p.returncode == 0, f"rank {rank} failed:\n{log[-3000:]}"
    return [dict(np.load(o, allow_pickle=False)) for o in outs]


def test_data_parallel_deterministic_training_over_shm_repeats_bit_for_bit(tmp_path):
    first = _launch_two_ranks(tmp_path, "a")
    second = _launch_two_ranks(tmp_path, "b")
    for r in first + second:
        assert bool(r["deterministic"]) and int(r["step"]) == 20 and str(r["transport"]) == "shm"
    p = first[0]["params"]
    for r in first[1:] + second:
        assert np.array_equal(r["params"], p)
    assert float(first[0]["loss"]) == float(second[0]["loss"])
