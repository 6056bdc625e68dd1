"""GPU parity on randomly drawn models: the hand-picked rows of tests/test_gpu_network.py::ACCEPTED cover every axis of the reference's
dispatch once; this file draws whole model descriptions at random (seeded) from the same space -- level count, features per level, table
size, base resolution, growth, interpolation, grid type, quantize_threshold, max_level, width, depth, activation, output activation --
and holds each draw to the same bars: encode bit-exact, network output within 2^-8 of the oracle, gradients within 3 % of the numpy
restatement.  VNR_FUZZ_DRAWS / VNR_FUZZ_SEED widen the sweep from a shell (tools/r06_fuzz.sh).

Deep networks with growing activations (six hidden layers of Exponential at 128 neurons ...) are legal and numerically poor: the fp16
rounding of the activations alone moves their output by more than 2^-8.  Where that is so the bar is the oracle's OWN distance from an fp64
evaluation of the same fp16 parameters (fp64_network below): the HIP path may be as far from the oracle as the oracle is from the unrounded
network (twice that, for the maximum over samples or entries), never farther.  The first sweeps of 3000 + 2500 draws
(profiles/r04_fuzz.txt) found fourteen draws past the fixed bars, every one of this kind (one sample of 1025) or sitting on a discontinuity of
the FUNCTION: an output on its L1 target (the gradient is a sign), or a ReLU unit whose fp32 sum is within rounding of zero (the mask follows
the order of the sum).  Targets and training coordinates are therefore drawn away from both (away_from_relu_kinks).  The 2^-8 bar holds the
independent oracle end to end; the inference kernel itself is held layer by layer, at rounding level, by tests/test_gpu_inference_stages.py."""
import os
import sys

import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neural_pt_cases as npc  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_ABS = 2.0 ** -8
INTERP = {"Linear": 0, "Smoothstep": 1, "Nearest": 2}
MAX_LEVELS = {1: 32, 2: 32, 4: 32, 8: 16}          # the padded encoded widths the kernels are instantiated for (infer_kernel.h dispatch)


def _act64(x, a, oracle):
    a = oracle.ACTIVATIONS.get(a, a)
    with np.errstate(over="ignore", invalid="ignore"):
        if a == 0: return x
        if a == 1: return np.maximum(x, 0)
        if a == 2: return np.exp(x)
        if a == 3: return 1 / (1 + np.exp(-x))
        if a == 4: t = 10 * x; return 0.5 * (t + np.sqrt(t * t + 4)) / 10
        if a == 5: return np.logaddexp(0, 10 * x) / 10
    raise ValueError(a)


def _dact64(x, y, a, oracle):
    a = oracle.ACTIVATIONS.get(a, a)
    with np.errstate(over="ignore", invalid="ignore"):
        if a == 0: return np.ones_like(x)
        if a == 1: return (x > 0).astype(np.float64)
        if a == 2: return y
        if a == 3: return y * (1 - y)
        if a == 4: t = 10 * x; return 0.5 * (1 + t / np.sqrt(t * t + 4))
        if a == 5: return 1 / (1 + np.exp(-10 * x))
    raise ValueError(a)


def away_from_relu_kinks(oracle, ocfg, W, H, params, n_mlp, coords, act, out_act, margin=1e-5, margin_deep=2.0 ** -10):
    """mask of the samples none of whose ReLU units sums to (nearly) zero: a pre-activation within fp32 rounding of zero gets its sign,
    hence its backward mask, from the ORDER of the fp32 sum, which the MFMA and the oracle's loop do not share (found by the first
    sweeps: tests/diag/fuzz_diag.py shows |sum| / sum|terms| of 3e-9 and 4e-7 on the samples behind the two draws that failed).  Like
    the L1 sign this is a discontinuity of the function, not of an implementation; gradient checks stay away from it.
    `margin` holds for the FIRST layer, whose inputs (the encode) are bit-identical on both sides.  Every later layer and the output
    read fp16 activations, and a handful of those per batch differ by one fp16 ulp between the two sides (an fp32 sum rounded once against an
    fp64 sum rounded once: 2 + 5 + 11 + 31 of 4 x 20 480 in the draw below), which moves the next pre-activation by up to 2^-11 of
    the sum of its |terms|: `margin_deep` = 2^-10.  Round 5, 4 500 draws of seed 424242 (tests/diag/mlp_grad_diag.py): draw 1761, one
    sample of 320 whose OUTPUT ReLU sums to +7.7e-7 here and to <= 0 in the restatement (the whole sample enters one gradient and not the
    other: 3.9 % of the norm), and draw 3303, one hidden unit of two identical samples at 7.9e-5 against 0 (3.03 %)."""
    from oracle import train_oracle as T
    relu = oracle.ACTIVATIONS["ReLU"]
    a, oa = oracle.ACTIVATIONS.get(act, act), oracle.ACTIVATIONS.get(out_act, out_act)
    keep = np.ones(coords.shape[0], bool)
    if a != relu and oa != relu:
        return keep
    in_w = oracle.padded_width(ocfg)
    w1, wh, wl, _ = T.split_mlp(params, in_w, W, H - 1)
    feat = oracle.grid_encode(ocfg, params[n_mlp:].view(np.uint16), coords)
    _, acts = oracle.mlp_forward(params[:n_mlp].view(np.uint16), in_w, W, H - 1, feat, activation=oracle.act_code(act, out_act),
                                 want_activations=True)
    acts = acts.view(np.float16).astype(np.float64)
    ins = [feat.view(np.float16).astype(np.float64)] + [acts[j] for j in range(H - 1)]
    mats = [w1.astype(np.float64)] + [m.astype(np.float64) for m in wh]
    if a == relu:
        for j, (x, m) in enumerate(zip(ins, mats)):
            sums, terms = np.abs(x @ m.T), np.abs(x) @ np.abs(m).T
            keep &= ((sums > (margin if j == 0 else margin_deep) * terms) | (terms == 0)).all(axis=1)      # (all terms zero: zero in any order)
    if oa == relu:
        x, m = acts[H - 1], wl[0].astype(np.float64)
        sums, terms = np.abs(x @ m), np.abs(x) @ np.abs(m)
        keep &= (sums > margin_deep * terms) | (terms == 0)
    return keep


def fp64_network(oracle, ocfg, W, H, params, coords, act, out_act, targets=None):
    """the network on the same fp16 parameters and the oracle's (bit-exact) encode, in fp64 without any rounding of activations or
    gradients: the yardstick for how much of a difference is fp16 noise.  Returns the outputs and, with targets, the loss-scaled L1
    gradients of all parameters."""
    from oracle import train_oracle as T
    in_w = oracle.padded_width(ocfg)
    w1, wh, wl, n_mlp = T.split_mlp(params, in_w, W, H - 1)
    w1, wh, wl0 = w1.astype(np.float64), [m.astype(np.float64) for m in wh], wl[0].astype(np.float64)
    feat = oracle.grid_encode(ocfg, params[n_mlp:].view(np.uint16), coords).view(np.float16).astype(np.float64)
    pre = [feat @ w1.T]; post = [_act64(pre[0], act, oracle)]
    for m in wh:
        pre.append(post[-1] @ m.T); post.append(_act64(pre[-1], act, oracle))
    z = post[-1] @ wl0
    y = _act64(z, out_act, oracle)
    if targets is None:
        return y
    B = coords.shape[0]
    F = ocfg.n_features
    g = np.zeros(params.size)
    with np.errstate(over="ignore", invalid="ignore"):
        dy = T.LOSS_SCALE * np.sign(y - targets) / B * _dact64(z, y, out_act, oracle)
        off = W * in_w + len(wh) * W * W
        g[off:off + W] = dy @ post[-1]
        d = dy[:, None] * wl0[None, :] * _dact64(pre[-1], post[-1], act, oracle)
        for l in range(len(wh) - 1, -1, -1):
            o_l = W * in_w + l * W * W
            g[o_l:o_l + W * W] = (d.T @ post[l]).ravel()
            d = (d @ wh[l]) * _dact64(pre[l], post[l], act, oracle)
        g[0:W * in_w] = (d.T @ feat).ravel()
        dfeat = d @ w1
    lay = oracle.grid_layout(ocfg)
    for l, (idxs, ws) in enumerate(T.corner_indices_and_weights(ocfg, lay, coords)):
        base = n_mlp + int(lay["offsets"][l]) * F
        for f in range(F):
            np.add.at(g, base + idxs.ravel() * F + f, (ws.astype(np.float64) * dfeat[:, l * F + f][:, None]).ravel())
    return y, g


def draw(rng):
    F = int(rng.choice([1, 2, 4, 8]))
    gtype = str(rng.choice(["Hash", "Hash", "Hash", "Dense", "Tiled"]))
    base = int(rng.integers(2, 10))
    if gtype == "Dense":                              # every level is stored whole: keep the finest one at <= 48^3 entries
        L = int(rng.integers(1, 6))
        pls = float(rng.choice([1.25, 1.5, 2.0]))
        while L > 1 and base * pls ** (L - 1) > 48:
            L -= 1
    else:
        L = int(rng.integers(1, MAX_LEVELS[F] + 1))
        # finest resolution <= 2^16: positions stay far inside the range where float -> uint conversions are defined
        hi = (65536.0 / base) ** (1.0 / max(1, L - 1))
        pls = float(min(2.0, rng.choice([1.2, 1.3195, 1.5, 1.75, 2.0]), hi))
    log2T = int(rng.integers(8, 15))
    W = int(rng.choice([16, 32, 64, 128]))
    H = int(rng.integers(1, 5)) if W < 128 else int(rng.integers(1, 7))
    interp = str(rng.choice(["Linear", "Linear", "Smoothstep", "Nearest"]))
    act = str(rng.choice(["ReLU", "ReLU", "ReLU", "None", "Sigmoid", "Squareplus", "Softplus", "Exponential"]))
    out_act = str(rng.choice(["None", "None", "None", "ReLU", "Sigmoid", "Exponential", "Squareplus", "Softplus"]))
    qt = float(rng.choice([0.0, 0.0, 0.02, 0.05]))
    max_level = None if rng.uniform() < 0.7 else float(np.round(rng.uniform(0.0, L), 2))
    return dict(L=L, F=F, log2T=log2T, base=base, pls=pls, H=H, W=W, interp=interp, act=act, out_act=out_act, gtype=gtype, qt=qt,
                max_level=max_level)


def check(oracle, d, seed):
    """returns the list of checks that could not be made on this draw (vacuous: non-finite or all-zero expectations)"""
    from oracle import train_oracle as T
    L, F, W, H = d["L"], d["F"], d["W"], d["H"]
    cfg = syn.model_config(n_levels=L, n_features=F, log2_hashmap_size=d["log2T"], base_resolution=d["base"], n_hidden_layers=H,
                           per_level_scale=d["pls"])
    cfg["encoding"]["interpolation"] = d["interp"]
    cfg["network"]["n_neurons"] = W
    cfg["network"]["activation"] = d["act"]
    cfg["network"]["output_activation"] = d["out_act"]
    if d["gtype"] != "Hash":
        cfg["encoding"]["type"] = d["gtype"]
    if d["qt"]:
        cfg["encoding"]["quantize_threshold"] = d["qt"]
    if d["max_level"] is not None:
        cfg["encoding"]["max_level"] = d["max_level"]
    sv = api.vnrCreateSimpleVolume(syn.analytic_volume(16))
    vol = api.vnrCreateNeuralVolume(cfg, sv)
    info = api.neural_info(vol)
    ocfg = oracle.grid_config(L, F, d["log2T"], d["base"], d["pls"], INTERP[d["interp"]], d["qt"],
                              1000.0 if d["max_level"] is None else d["max_level"], d["gtype"])
    assert info["n_params"] == oracle.n_params(ocfg, W, H), "n_params"
    assert info["padded_width"] == oracle.padded_width(ocfg), "padded width"
    assert info["mfma_kernels"] == 1 and info["mfma_training_kernels"] == 1
    n_mlp = oracle.mlp_n_params(info["padded_width"], W, H - 1)
    grows = d["act"] in ("Exponential", "Softplus") or d["out_act"] == "Exponential"
    params = syn.random_params(info["n_params"], n_mlp, seed=seed, mlp_scale=(0.35 if grows else 1.0) * (0.7 if H > 3 else 1.0))
    api.neural_set_params_fp16(vol, params)
    rng = np.random.default_rng(seed + 1)
    coords = rng.uniform(0, 1, (1025, 3)).astype(np.float32)
    coords[0] = (0, 0, 0); coords[1] = (1, 1, 1); coords[2] = (0.5, 0.5, 0.5); coords[3] = (1, 0, 0.999999)
    vacuous = []
    enc = api.neural_encode(vol, coords)
    want_enc = oracle.grid_encode(ocfg, params[n_mlp:].view(np.uint16), coords)
    assert np.array_equal(enc.view(np.uint16), want_enc), "encode"
    got = api.neural_inference(vol, coords)
    code = oracle.act_code(d["act"], d["out_act"])
    want = oracle.network_inference(ocfg, W, H, params.view(np.uint16), coords, activation=code)
    if not np.isfinite(want).all() or np.abs(want).max() > 6.0e4:
        vacuous.append("inference")
    else:
        assert np.isfinite(got).all(), "inference finite"
        err = np.abs(got - want).max()
        exact = fp64_network(oracle, ocfg, W, H, params, coords, d["act"], d["out_act"])
        noise = float(np.abs(want - exact).max())            # what fp16 activations cost this model on these samples
        assert err <= max(TOL_ABS * max(1.0, np.abs(want).max()), 2 * noise), ("inference", err, np.abs(want).max(), noise)
    B = 320
    tc = rng.uniform(0, 1, (2 * B, 3)).astype(np.float32)
    tc = tc[away_from_relu_kinks(oracle, ocfg, W, H, params, n_mlp, tc, d["act"], d["out_act"])][:B]
    for _ in range(2):                              # a deep, wide ReLU network keeps few samples clear of every unit's kink: draw more before giving up
        if tc.shape[0] >= B:
            break
        more = rng.uniform(0, 1, (8 * B, 3)).astype(np.float32)
        tc = np.concatenate([tc, more[away_from_relu_kinks(oracle, ocfg, W, H, params, n_mlp, more, d["act"], d["out_act"])]])[:B]
    B = tc.shape[0]
    if B < 64:                                      # (a network whose output is a cancellation everywhere)
        return vacuous + ["gradients: every sample on a kink"]
    # targets at least 0.05 from the network's outputs: the L1 gradient is a sign, and a sample whose output sits on its target flips it
    y_tc = oracle.network_inference(ocfg, W, H, params.view(np.uint16), tc, activation=code)
    y_tc = np.where(np.isfinite(y_tc), y_tc, 0).astype(np.float32)
    # (round 6, seed 7117 draw 243: an Exponential output of 31 has an fp16 ulp of 0.03; the two paths' outputs differed by two ulps around a
    # target 0.053 away and ONE flipped sign of 320 moved the MLP gradient by 76 %, tests/diag/mlp_grad_diag.py -- so the margin grows with |y|)
    tt = (y_tc + rng.choice([-1.0, 1.0], B) * (rng.uniform(0.05, 0.6, B) + 2.0 ** -7 * np.abs(y_tc))).astype(np.float32)
    grads = api.neural_forward_backward(vol, tc, tt).astype(np.float64)
    ref = T.training_gradients(ocfg, W, H, params.view(np.uint16), tc, tt, loss="L1", activation=d["act"], output_activation=d["out_act"])
    w_all = ref["grads"]
    if "inference" in vacuous or not np.isfinite(w_all).all() or np.abs(w_all).max() > 3.0e4:
        vacuous.append("gradients")
    else:
        y64, x_all = fp64_network(oracle, ocfg, W, H, params, tc, d["act"], d["out_act"], targets=tt)
        y_noise = float(np.abs(ref["y"] - y64).mean()) if np.isfinite(y64).all() else 0.0      # the L1 loss is a mean of |y - t|
        assert np.isclose(api.vnrNeuralVolumeGetTrainingLoss(vol), ref["loss"], rtol=2e-3, atol=1e-5 + 2 * y_noise), ("loss", y_noise)
        assert np.isfinite(grads).all(), "gradients finite"
        for name, sl in [("mlp", slice(0, n_mlp)), ("grid", slice(n_mlp, None))]:
            g, w, x = grads[sl], w_all[sl], x_all[sl]
            if np.abs(w).max() < 1e-3:      # a saturated output activation or a mask over every level: nothing to compare against
                vacuous.append("gradients " + name)
                assert np.abs(g).max() < 1e-2, name
                continue
            # the restatement's own distance from the unrounded gradients (fp16 activations and fp16 gradient chain of a deep network)
            noise_rel = np.linalg.norm(w - x) / np.linalg.norm(w) if np.isfinite(x).all() else 0.0
            noise_abs = np.abs(w - x).max() if np.isfinite(x).all() else 0.0
            rel = np.linalg.norm(g - w) / np.linalg.norm(w)
            if os.environ.get("VNR_FUZZ_VERBOSE") and name == "grid" and rel >= 3e-2:
                lay = oracle.grid_layout(ocfg)
                print("draw", d, "grid rel", rel, "max |w|", np.abs(w).max(), "max |g - w|", np.abs(g - w).max())
                for l in range(d["L"]):
                    a0, a1 = int(lay["offsets"][l]) * F, int(lay["offsets"][l + 1]) * F
                    wl_, gl_ = w[a0:a1], g[a0:a1]
                    print("   level", l, "entries", (a1 - a0) // F, "|w|", float(np.linalg.norm(wl_)), "rel", float(np.linalg.norm(gl_ - wl_) / max(np.linalg.norm(wl_), 1e-30)),
                          "max|w|", float(np.abs(wl_).max()), "max|g|", float(np.abs(gl_).max()))
            if name == "grid" and not rel < max(3e-2, noise_rel):
                grid_gradient_post_mortem(vol, tc, grads, w_all, ref, n_mlp, d)     # (round 4's transient: take it apart while the state is there)
            assert rel < max(3e-2, noise_rel), (name, rel, noise_rel)
            assert np.abs(g - w).max() < max(6e-2 * np.abs(w).max(), 2 * noise_abs), (name, np.abs(g - w).max(), np.abs(w).max(), noise_abs)
        last = grads[n_mlp - 16 * W:n_mlp].reshape(16, W)
        assert np.all(last[1:] == 0), "padded rows of the last layer"
    # params.json round trip (network.cu:827-857): the file carries the model description; the loaded network is the same network
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "params.json")
        api.vnrNeuralVolumeSerializeParams(vol, path)
        vol2 = api.vnrCreateNeuralVolume(path)
    info2 = api.neural_info(vol2)
    for k in ("n_neurons", "n_hidden_layers", "activation", "output_activation", "grid_type", "interpolation", "n_params", "padded_width"):
        assert info2[k] == info[k], ("params.json", k, info2[k], info[k])
    assert np.array_equal(api.neural_get_params_fp16(vol2).view(np.uint16), params.view(np.uint16)), "params.json parameters"
    a, b = api.neural_inference(vol, coords[:257]), api.neural_inference(vol2, coords[:257])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "params.json inference"       # (max_level and quantize_threshold survived)
    api.neural_train_end(vol)
    api.vnrNeuralVolumeTrain(vol, 3, True)
    return vacuous


def grid_gradient_post_mortem(vol, tc, grads, w_all, ref, n_mlp, d):
    """a gradient batch whose GRID part misses the restatement (once in ~28 000 draws in round 4, never again in 1.9 M repetitions of
    tests/diag/grad_hammer.py): before the assertion ends the draw, separate the three suspects with what is still on the device --
    the blob downloaded again (a download that raced the stream), dL/dfeatures against the restatement's (the MLP backward's side), the
    grid backward alone repeated on the stored dL/dfeatures (a scatter that lost or double-counted updates).  Printed, and kept in
    gpurun_out/ as an .npz"""
    L = api.lib()

    def buf(which):
        return api.neural_training_buffer(vol, which, np.float16)

    w = w_all[n_mlp:]
    again = buf(0).astype(np.float64)
    print("\nGRID GRADIENT POST-MORTEM, draw", d)
    print("  the blob read again from the device: rel to the restatement %.4f (first download: %.4f); equal to the first download: %s"
          % (np.linalg.norm(again[n_mlp:] - w) / np.linalg.norm(w), np.linalg.norm(grads[n_mlp:] - w) / np.linalg.norm(w), np.array_equal(again, grads)))
    dfeat = buf(1).astype(np.float32).reshape(tc.shape[0], -1)
    want = ref["dfeat"]
    bad_rows = np.nonzero(np.abs(dfeat - want).max(1) > 2.0 ** -7 * max(np.abs(want).max(), 1e-30))[0]
    print("  dL/dfeatures against the restatement: max |d| %.3e of max %.3e; rows off by more than 2^-7 of the maximum: %d %s"
          % (np.abs(dfeat - want).max(), np.abs(want).max(), bad_rows.size, bad_rows[:16].tolist()))
    d_tc = api.DeviceArray.from_numpy(tc)
    api.check(L.vnrAmdNeuralVolumeRescatterGridGradients(vol.h, tc.shape[0], d_tc.ptr))
    re = buf(0).astype(np.float64)
    print("  the grid backward alone, repeated on the stored dL/dfeatures: rel to the restatement %.4f -> %s"
          % (np.linalg.norm(re[n_mlp:] - w) / np.linalg.norm(w),
             "the first scatter lost or double-counted updates" if np.linalg.norm(re[n_mlp:] - w) / np.linalg.norm(w) < 3e-2 else "the scatter reproduces the miss: its inputs are off"))
    os.makedirs("gpurun_out", exist_ok=True)
    np.savez(os.path.join("gpurun_out", "grid_gradient_post_mortem.npz"), first=grads, again=again, rescatter=re, want=w_all, dfeat=dfeat, want_dfeat=want, coords=tc)


def test_randomly_drawn_models_equal_the_oracle(oracle):
    n = int(os.environ.get("VNR_FUZZ_DRAWS", "40"))
    seed0 = int(os.environ.get("VNR_FUZZ_SEED", "20260410"))
    rng = np.random.default_rng(seed0)
    failures, vacuous_draws = [], 0
    for i in range(n):
        d = draw(rng)
        try:
            v = check(oracle, d, seed0 % 1000 + i)
            vacuous_draws += bool(v)
        except Exception as e:  # collect every failing draw of the sweep, then fail once with all of them
            failures.append((i, d, repr(e)[:300]))
        if os.environ.get("VNR_FUZZ_LOG"):
            with open(os.environ["VNR_FUZZ_LOG"], "a") as f:
                f.write(f"{i} {d} {'FAIL ' + failures[-1][2] if failures and failures[-1][0] == i else ('vacuous ' + str(v) if v else 'ok')}\n")
    assert not failures, failures
    assert vacuous_draws <= n // 3, vacuous_draws


DEEP = [   # weight images beyond the 160 KiB of LDS at every width (tcnn's FullyFusedMLP has no depth limit): the A operands come from global memory
    dict(L=8, F=2, log2T=12, base=4, pls=2.0, H=21, W=64, interp="Linear", act="ReLU", out_act="None", gtype="Hash", qt=0.0, max_level=None),
    dict(L=6, F=4, log2T=11, base=4, pls=1.5, H=24, W=64, interp="Smoothstep", act="Sigmoid", out_act="Sigmoid", gtype="Hash", qt=0.0, max_level=None),
    dict(L=8, F=2, log2T=12, base=4, pls=2.0, H=81, W=32, interp="Linear", act="Sigmoid", out_act="None", gtype="Hash", qt=0.0, max_level=None),
    dict(L=4, F=8, log2T=10, base=4, pls=2.0, H=90, W=32, interp="Nearest", act="Squareplus", out_act="None", gtype="Tiled", qt=0.0, max_level=None),
    dict(L=8, F=1, log2T=12, base=4, pls=2.0, H=321, W=16, interp="Linear", act="Sigmoid", out_act="None", gtype="Dense", qt=0.0, max_level=None),
]


@pytest.mark.parametrize("d", DEEP)
def test_networks_too_deep_for_the_lds_at_every_width(oracle, d):
    info_checks = check(oracle, d, 900 + d["H"])
    assert "inference" not in info_checks, info_checks          # (gradients of the first layers of a 300-layer Sigmoid network are zero on both sides)


# ------------------------------------------------------------------------------------------------ the same, behind the renderer
def draw_scene(rng):
    d = draw(rng)
    # a frame through the oracle costs a network evaluation per sample on the host: small grids, shallow networks
    d["L"] = min(d["L"], 6); d["log2T"] = min(d["log2T"], 12); d["H"] = min(d["H"], 3)
    if d["gtype"] == "Dense":
        d["L"] = min(d["L"], 3)
    d["max_level"] = None if d["max_level"] is None else min(d["max_level"], float(d["L"]))
    if d["act"] in ("Exponential", "Softplus"):
        d["act"] = "ReLU"
    if d["out_act"] in ("Exponential", "Softplus", "Squareplus"):      # values far outside the transfer function's range: nothing to see
        d["out_act"] = "None"
    v = rng.normal(size=3); v /= np.linalg.norm(v)
    if abs(v[1]) > 0.95:                                               # not along the up vector
        v = np.array([0.6, 0.5, -0.62]); v /= np.linalg.norm(v)
    d.update(mode=int(rng.choice([5, 5, 8])), size=(int(rng.integers(17, 141)), int(rng.integers(9, 101))),
             cam_from=tuple(float(x) for x in v * 32 * rng.uniform(1.1, 2.6)), fovy=float(rng.uniform(25, 70)),
             sampling_rate=float(rng.choice([0.5, 1.0, 1.0, 2.0])), density_scale=float(rng.choice([1.0, 1.0, 0.5, 3.0])))
    d["scale"] = tuple(float(np.float32(q)) for q in rng.uniform(0.6, 1.7, 3)) if rng.uniform() < 0.5 else (1.0, 1.0, 1.0)
    lo = rng.uniform(0, 0.5, 3); hi = np.minimum(lo + rng.uniform(0.3, 0.8, 3), 1.0)
    d["clip"] = (tuple(float(np.float32(q * 32)) for q in lo), tuple(float(np.float32(q * 32)) for q in hi)) if rng.uniform() < 0.4 else None
    return d


def check_frame(oracle, d, seed):
    L, F, W, H = d["L"], d["F"], d["W"], d["H"]
    cfg = syn.model_config(n_levels=L, n_features=F, log2_hashmap_size=d["log2T"], base_resolution=d["base"], n_hidden_layers=H,
                           per_level_scale=d["pls"])
    cfg["encoding"]["interpolation"] = d["interp"]
    cfg["network"]["n_neurons"] = W
    cfg["network"]["activation"] = d["act"]
    cfg["network"]["output_activation"] = d["out_act"]
    if d["gtype"] != "Hash":
        cfg["encoding"]["type"] = d["gtype"]
    if d["qt"]:
        cfg["encoding"]["quantize_threshold"] = d["qt"]
    if d["max_level"] is not None:
        cfg["encoding"]["max_level"] = d["max_level"]
    sv = api.vnrCreateSimpleVolume(syn.analytic_volume(32))
    nv = api.vnrCreateNeuralVolume(cfg, sv, online_macrocell_construction=False)
    info = api.neural_info(nv)
    n_mlp = oracle.mlp_n_params(info["padded_width"], W, H - 1)
    params = syn.random_params(info["n_params"], n_mlp, seed=seed)
    api.neural_set_params_fp16(nv, params)
    colors, alphas = syn.tfn_ramp_with_bumps()
    tfn = api.vnrCreateTransferFunction()
    api.vnrTransferFunctionSetColor(tfn, colors); api.vnrTransferFunctionSetAlpha(tfn, alphas); api.vnrTransferFunctionSetValueRange(tfn, (0, 1))
    camera = api.vnrCreateCamera()
    api.vnrCameraSet(camera, d["cam_from"], (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), d["fovy"])
    ren = api.vnrCreateRenderer(nv)
    api.vnrRendererSetTransferFunction(ren, tfn); api.vnrRendererSetCamera(ren, camera); api.vnrRendererSetFramebufferSize(ren, d["size"])
    api.vnrRendererSetMode(ren, d["mode"])
    api.vnrRendererSetVolumeSamplingRate(ren, d["sampling_rate"])
    api.vnrRendererSetVolumeDensityScale(ren, d["density_scale"])
    # the neural volume scaled per axis and clipped to a box (the march is the dense volumes'; the sweep of dense scenes holds both to 2e-4)
    fd = np.array((32, 32, 32), np.float32)
    xfm = np.array([fd[0] * d["scale"][0], 0, 0, 0, fd[1] * d["scale"][1], 0, 0, 0, fd[2] * d["scale"][2],
                    d["scale"][0] * (-fd[0] / 2), d["scale"][1] * (-fd[1] / 2), d["scale"][2] * (-fd[2] / 2)], np.float32)
    bbox = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    if d["scale"] != (1.0, 1.0, 1.0):
        api.vnrVolumeSetScaling(nv, d["scale"])
    if d["clip"] is not None:
        api.vnrVolumeSetClippingBox(nv, d["clip"][0], d["clip"][1])
        bbox = tuple(tuple(float(q) for q in c) for c in _clipbox_as_the_library_computes_it(xfm, d["clip"][0], d["clip"][1], (32, 32, 32)))
    api.vnrRender(ren)
    img = api.vnrRendererMapFrame(ren).copy()
    ocfg = oracle.grid_config(L, F, d["log2T"], d["base"], d["pls"], INTERP[d["interp"]], d["qt"],
                              1000.0 if d["max_level"] is None else d["max_level"], d["gtype"])
    mo = api.volume_macrocell(nv)["max_opacity"]
    code = oracle.act_code(d["act"], d["out_act"])
    net = lambda c: oracle.network_inference(ocfg, W, H, params.view(np.uint16), c, activation=code)   # noqa: E731
    sc = oracle.SceneHolder(d["size"][0], d["size"][1], (32, 32, 32), oracle.TfnHolder(colors, alphas), mo, d["cam_from"], (0, 0, 0), (0, 1, 0),
                            d["fovy"], sampling_rate=d["sampling_rate"], density_scale=d["density_scale"], shading_mode=1 if d["mode"] == 8 else 0,
                            bbox=bbox, xfm=xfm)
    ref, _, _ = oracle.render_streaming(sc, net)
    assert img.shape == ref.shape, (img.shape, ref.shape)
    assert np.isfinite(img).all(), "frame finite"
    mse = float(((img - ref) ** 2).mean())
    psnr = 10 * np.log10(1.0 / max(mse, 1e-20))
    assert psnr > 40.0, ("psnr", psnr)
    return [] if ref[..., 3].max() > 0.002 else ["nothing visible"]


def test_randomly_drawn_models_render_like_the_oracle(oracle):
    n = int(os.environ.get("VNR_FUZZ_FRAMES", "12"))
    seed0 = int(os.environ.get("VNR_FUZZ_SEED", "20260410")) + 17
    rng = np.random.default_rng(seed0)
    failures, vacuous_draws = [], 0
    for i in range(n):
        d = draw_scene(rng)
        v = None
        try:
            v = check_frame(oracle, d, seed0 % 1000 + i)
            vacuous_draws += bool(v)
        except Exception as e:
            failures.append((i, d, repr(e)[:300]))
        if os.environ.get("VNR_FUZZ_LOG"):
            with open(os.environ["VNR_FUZZ_LOG"], "a") as f:
                f.write(f"frame {i} {d} {'FAIL ' + failures[-1][2] if v is None else ('vacuous ' + str(v) if v else 'ok')}\n")
    assert not failures, failures
    assert vacuous_draws <= n // 2, vacuous_draws


# ------------------------------------------------------------------------------------------------ in-shader kernels against the streaming path
def test_randomly_drawn_models_render_alike_through_the_in_shader_and_the_streaming_kernels(oracle):
    """rendering modes 6 / 9 / 12 / 14 / 15 on a neural volume have two implementations (in_shader.h: one launch with the network inside the
    marching loop; the streaming path: march / evaluate / compose per iteration).  On random models of every width (16 / 32 / 64 / 128) and
    kind (round 5: the in-shader kernels are instantiated for all of them; shapes outside their list take the streaming path either way)
    the network values are the same bits, so ray marching differs only by the streaming path's resume rounding (PSNR > 70 dB) and path
    tracing not at all.  Two black frames are equal whatever the path tracer does after a real collision, so the draws of modes 14 / 15 scale
    their MLP weights by width as the lit models of tests/neural_pt_cases.py do (on the host, with the oracle alone, 4 of the 4 such draws of
    the default seed are lit that way and 2 of 4 without), the lit share of each goes into the log, and a third of them must be lit."""
    from instantvnr_amd._lib import check, lib
    n = int(os.environ.get("VNR_FUZZ_IN_SHADER", "16"))
    rng = np.random.default_rng(int(os.environ.get("VNR_FUZZ_SEED", "20260410")) + 31)
    colors, alphas = syn.tfn_ramp_with_bumps()
    failures, pt_draws, lit_draws = [], 0, 0
    for i in range(n):
        lit = None
        F = int(rng.choice([1, 2, 4, 8]))
        L = int(rng.integers(2, min(MAX_LEVELS[F], 12) + 1))
        base = int(rng.integers(2, 9))
        pls = float(min(2.0, rng.choice([1.3195, 1.5, 2.0]), (4096.0 / base) ** (1.0 / max(1, L - 1))))
        H = int(rng.integers(1, 5))
        interp = str(rng.choice(["Linear", "Smoothstep", "Nearest"], p=[0.5, 0.3, 0.2]))
        mode = int(rng.choice([6, 9, 12, 14, 15]))
        size = (int(rng.integers(17, 200)), int(rng.integers(9, 130)))
        W = int(rng.choice([16, 32, 64, 128]))
        act = str(rng.choice(["ReLU", "None", "Sigmoid", "Squareplus", "Softplus"], p=[0.5, 0.1, 0.15, 0.15, 0.1]))
        out_act = str(rng.choice(["None", "Sigmoid", "ReLU"], p=[0.7, 0.2, 0.1]))
        gtype = str(rng.choice(["Hash", "Dense", "Tiled"], p=[0.6, 0.2, 0.2]))
        qt = float(rng.choice([0.0, 0.0, 0.05]))
        while gtype == "Dense" and L > 1 and base * pls ** (L - 1) > 48:     # every level of a Dense grid is stored whole
            L -= 1
        d = dict(i=i, L=L, F=F, base=base, pls=pls, H=H, W=W, interp=interp, act=act, out_act=out_act, gtype=gtype, qt=qt, mode=mode, size=size)
        try:
            cfg = syn.model_config(n_levels=L, n_features=F, log2_hashmap_size=int(rng.integers(9, 16)), base_resolution=base, n_hidden_layers=H,
                                   per_level_scale=pls, n_neurons=W)
            cfg["encoding"]["interpolation"] = interp
            cfg["network"]["activation"] = act; cfg["network"]["output_activation"] = out_act
            if gtype != "Hash": cfg["encoding"]["type"] = gtype
            if qt: cfg["encoding"]["quantize_threshold"] = qt
            sv = api.vnrCreateSimpleVolume(syn.analytic_volume(32))
            nv = api.vnrCreateNeuralVolume(cfg, sv, online_macrocell_construction=False)
            info = api.neural_info(nv)
            api.neural_set_params_fp16(nv, syn.random_params(info["n_params"], oracle.mlp_n_params(info["padded_width"], W, H - 1), seed=100 + i,
                                                             mlp_scale=(npc.MLP_SCALE_BY_WIDTH[W] if mode in (14, 15) else 0.5 if W == 128 else 1.0) * (0.7 if H > 3 else 1.0)))
            tfn = api.vnrCreateTransferFunction()
            api.vnrTransferFunctionSetColor(tfn, colors); api.vnrTransferFunctionSetAlpha(tfn, alphas); api.vnrTransferFunctionSetValueRange(tfn, (0, 1))
            v = rng.normal(size=3); v /= np.linalg.norm(v)
            if abs(v[1]) > 0.95:
                v = np.array([0.6, 0.5, -0.62]); v /= np.linalg.norm(v)
            camera = api.vnrCreateCamera()
            api.vnrCameraSet(camera, tuple(float(x) for x in v * 32 * rng.uniform(1.1, 2.6)), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), float(rng.uniform(25, 70)))
            rate, density = float(rng.choice([0.5, 1.0, 2.0])), float(rng.choice([0.5, 1.0, 3.0]))
            frames, hits = {}, {}
            for kernel in (1, 0):
                r = api.vnrCreateRenderer(nv)
                api.vnrRendererSetTransferFunction(r, tfn); api.vnrRendererSetCamera(r, camera); api.vnrRendererSetFramebufferSize(r, size)
                api.vnrRendererSetMode(r, mode)
                api.vnrRendererSetVolumeSamplingRate(r, rate); api.vnrRendererSetVolumeDensityScale(r, density)
                check(lib().vnrAmdRendererSetInShaderKernel(r.h, kernel))
                acc = []
                for _ in range(2):
                    api.vnrRender(r)
                    acc.append(api.vnrRendererMapFrame(r).copy())
                frames[kernel], hits[kernel] = acc, api.vnrRendererGetFrameStats(r)["n_rays_hit"]
            assert hits[1] == hits[0], ("rays hit", hits)
            if mode in (14, 15):
                lit = npc.lit_share(frames[1][0])
                pt_draws += 1
                lit_draws += lit >= 0.03          # the floor of the dense-volume path-tracing tests (tests/test_gpu_render.py)
            for k in range(2):
                a, b = frames[1][k], frames[0][k]
                assert np.isfinite(a).all() and np.isfinite(b).all()
                if mode in (14, 15):
                    assert np.array_equal(a, b), ("path tracing", k, float(np.abs(a - b).max()))
                else:
                    mse = float(((a.astype(np.float64) - b) ** 2).mean())
                    assert mse == 0 or 10 * np.log10(1.0 / mse) > 70, ("psnr", k, 10 * np.log10(1.0 / mse))
        except Exception as e:
            failures.append((d, repr(e)[:300]))
        if os.environ.get("VNR_FUZZ_LOG"):
            with open(os.environ["VNR_FUZZ_LOG"], "a") as f:
                f.write(f"in-shader {d} {'' if lit is None else f'lit {lit:.3f} '}{'FAIL ' + failures[-1][1] if failures and failures[-1][0] is d else 'ok'}\n")
    assert not failures, failures
    assert 3 * lit_draws >= pt_draws, ("path-tracing draws that are lit", lit_draws, pt_draws)


# ------------------------------------------------------------------------------------------------ dense volumes: sampling, macrocells, DDA, camera

def _clipbox_as_the_library_computes_it(xfm, lower, upper, dims):
    """vnrVolumeSetClippingBox (api.cpp:322-338): xfmPoint(transform.inverse(), corner - dims / 2), in fp32 and in the library's order of
    operations (csrc/common.h affine_inverse / xfm_point, built with -ffp-contract=off), so that the oracle clips at the same planes"""
    f = np.float32
    vx, vy, vz, p = (np.array(xfm[3 * i:3 * i + 3], f) for i in range(4))
    cross = lambda a, b: np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f)     # noqa: E731
    dot = lambda a, b: f(f(a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])                                                          # noqa: E731
    c0, c1, c2 = cross(vy, vz), cross(vz, vx), cross(vx, vy)
    r = f(1.0) / dot(vx, c0)
    ox, oy, oz = r * np.array([c0[0], c1[0], c2[0]], f), r * np.array([c0[1], c1[1], c2[1]], f), r * np.array([c0[2], c1[2], c2[2]], f)
    xv = lambda v: (v[0] * ox + v[1] * oy) + v[2] * oz                                                                           # noqa: E731
    op = -xv(p)
    half = np.array(dims, f) / f(2.0)
    return tuple((xv(np.array(c, f) - half) + op).astype(f) for c in (lower, upper))

def scene_draw(oracle, seed, i, verbose=False):
    """one draw of the dense-scene sweep, from its own generator (replayable alone: VNR_FUZZ_ONLY=<i>,<i> with -s prints what differs)"""
    rng = np.random.default_rng([seed, i])
    dims = tuple(int(v) if rng.uniform() < 0.9 else int(rng.integers(1, 5)) for v in rng.integers(5, 71, 3))          # (nx, ny, nz); one axis in ten of 1..4 voxels
    mode = int(rng.choice([4, 5, 7, 8, 4, 5, 7, 8, 10, 11, 13, 14]))
    size = (int(rng.integers(9, 150)), int(rng.integers(9, 110)))
    inside = rng.uniform() < 0.2
    d = dict(i=i, dims=dims, mode=mode, size=size, inside=bool(inside))
    scene_draw.last = d
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.linspace(0, 1, nz), np.linspace(0, 1, ny), np.linspace(0, 1, nx), indexing="ij")
    k = rng.uniform(1.0, 7.0, 6); ph = rng.uniform(0, 6.28, 3)
    vol = (0.5 + 0.5 * np.sin(k[0] * x + k[1] * y + ph[0]) * np.cos(k[2] * y + k[3] * z + ph[1]) * np.sin(k[4] * z + k[5] * x + ph[2])).astype(np.float32)
    vol += rng.normal(0, 0.02, vol.shape).astype(np.float32)
    if rng.uniform() < 0.5 and nx >= 4:                       # an empty slab on one side
        vol[:, :, : max(1, nx // 4)] = vol.min()
    sv = api.vnrCreateSimpleVolume(vol)
    lo, hi = np.float32(vol.min()), np.float32(vol.max())     # the reference's load-time normalisation (neural_sampler.cpp:176-210)
    vol = np.clip((vol - lo) / (hi - lo), np.float32(0), np.float32(1)).astype(np.float32)
    c = rng.uniform(-0.05, 1.05, (1500, 3)).astype(np.float32)
    for nodal in (False, True):
        assert np.array_equal(api.simple_volume_sample(sv, c, nodal), oracle.sample_volume(vol, c, nodal)), "sampling"
    nc, na = int(rng.integers(2, 300)), int(rng.integers(2, 300))
    colors = rng.uniform(0, 1, (nc, 3)).astype(np.float32)
    alphas = (np.clip(rng.uniform(-0.6, 1.0, na), 0, 1) * (np.linspace(0, 1, na) ** rng.uniform(0.3, 3.0))).astype(np.float32)
    tfn = api.vnrCreateTransferFunction()
    api.vnrTransferFunctionSetColor(tfn, colors); api.vnrTransferFunctionSetAlpha(tfn, alphas); api.vnrTransferFunctionSetValueRange(tfn, (0, 1))
    otfn = oracle.TfnHolder(colors, alphas)
    v = rng.normal(size=3); v /= np.linalg.norm(v)
    if abs(v[1]) > 0.95:
        v = np.array([0.6, 0.5, -0.62]); v /= np.linalg.norm(v)
    dist = max(dims) * (rng.uniform(0.05, 0.3) if inside else rng.uniform(0.9, 2.6))
    frm = tuple(float(q) for q in v * dist)
    at = tuple(float(q) for q in rng.uniform(-0.15, 0.15, 3) * max(dims))
    fovy = float(rng.uniform(20, 90))
    camera = api.vnrCreateCamera()
    api.vnrCameraSet(camera, frm, at, (0.0, 1.0, 0.0), fovy)
    rate, density = float(rng.choice([0.5, 1.0, 1.0, 2.0, 3.0])), float(rng.choice([0.3, 1.0, 1.0, 4.0]))
    d.update(frm=frm, at=at, fovy=fovy, rate=rate, density=density, tfn=(nc, na))
    # vnrVolumeSetScaling (api.cpp:340-351: transform = scale(s) * transform) and vnrVolumeSetClippingBox (api.cpp:322-338: the box
    # is given in voxels of the centred volume and taken through the inverse of the CURRENT transform), in either order
    fdims = np.array(dims, np.float32)
    scale = np.ones(3, np.float32)
    bbox = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    T = lambda sc_: np.array([sc_[0] * fdims[0], 0, 0, 0, sc_[1] * fdims[1], 0, 0, 0, sc_[2] * fdims[2],                   # noqa: E731
                              sc_[0] * (-fdims[0] / 2), sc_[1] * (-fdims[1] / 2), sc_[2] * (-fdims[2] / 2)], np.float32)
    order = int(rng.integers(0, 4))        # 0 neither, 1 scaling, 2 box then scaling, 3 scaling then box
    if order in (2, 3) or rng.uniform() < 0.2:
        a_, b_ = np.sort(rng.uniform(0, 1, (2, 3)), axis=0)
        b_ = np.maximum(b_, a_ + 0.15)
        lower, upper = (a_ * fdims).astype(np.float32), (np.minimum(b_, 1.0) * fdims).astype(np.float32)
    if order == 2:
        api.vnrVolumeSetClippingBox(sv, tuple(lower), tuple(upper))
        bbox = tuple(tuple(float(q) for q in c) for c in _clipbox_as_the_library_computes_it(T(scale), lower, upper, dims))
    if order in (1, 2, 3):
        scale = rng.uniform(0.5, 2.0, 3).astype(np.float32)
        api.vnrVolumeSetScaling(sv, tuple(float(q) for q in scale))
    if order == 3:      # the same box of the volume, said in the coordinates of the scaled volume
        half = fdims / np.float32(2)
        lo_w, hi_w = ((lower - half) * scale + half).astype(np.float32), ((upper - half) * scale + half).astype(np.float32)
        api.vnrVolumeSetClippingBox(sv, tuple(lo_w), tuple(hi_w))
        bbox = tuple(tuple(float(q) for q in c) for c in _clipbox_as_the_library_computes_it(T(scale), lo_w, hi_w, dims))
    xfm = T(scale)
    d.update(order=order, scale=tuple(float(q) for q in scale), bbox=bbox)
    r = api.vnrCreateRenderer(sv)
    api.vnrRendererSetTransferFunction(r, tfn); api.vnrRendererSetCamera(r, camera); api.vnrRendererSetFramebufferSize(r, size)
    api.vnrRendererSetMode(r, mode)
    api.vnrRendererSetVolumeSamplingRate(r, rate); api.vnrRendererSetVolumeDensityScale(r, density)
    api.vnrRender(r)
    img = api.vnrRendererMapFrame(r).copy()
    st = api.vnrRendererGetFrameStats(r)
    mc = api.volume_macrocell(sv)
    vr = oracle.macrocell_compute_implicit(vol)
    assert mc["dims"] == tuple((q + 15) // 16 for q in dims), "macrocell dims"
    assert np.array_equal(mc["value_range"], vr), "macrocell value ranges"
    mo = oracle.macrocell_max_opacity(otfn, vr)
    assert np.array_equal(mc["max_opacity"], mo), "macrocell opacities"
    sc = oracle.SceneHolder(size[0], size[1], dims, otfn, mo, frm, at, (0, 1, 0), fovy, sampling_rate=rate, density_scale=density,
                            shading_mode=1 if mode in (7, 8) else 2 if mode in (10, 11) else 0, bbox=bbox, xfm=xfm)
    sample = lambda q: oracle.sample_volume(vol, q, nodal=True)      # noqa: E731
    if mode in (5, 8, 11):
        want, _, ost = oracle.render_streaming(sc, sample)
        if verbose:
            print("streaming: library", st, "oracle", ost, "max |diff|", float(np.abs(img - want).max()), "alpha max", float(want[..., 3].max()))
        assert st["n_rays_hit"] == ost["n_rays_hit"], ("rays hit", st["n_rays_hit"], ost["n_rays_hit"])
        # the library counts the iterations that evaluated a sample; the reference's loop (method_raymarching.cu:931-958) also makes a last
        # trip for rays that survived a batch and then find nothing more to sample (2 of ~600 draws of the sweeps; the frames are equal)
        assert ost["n_iterations"] - st["n_iterations"] in (0, 1), ("iterations", st["n_iterations"], ost["n_iterations"])
    elif mode == 14:
        want, _, ost = oracle.render_pathtracing(sc, sample)
        assert st["n_rays_hit"] == ost["n_rays_hit"], ("rays hit", st["n_rays_hit"], ost["n_rays_hit"])
    elif mode == 13:
        want, _ = oracle.render_pathtracing_monolithic(sc, vol)
    else:
        want, _ = oracle.render_monolithic(sc, vol)
    assert np.isfinite(img).all()
    if mode in (13, 14):
        # path tracing: the same random walk on the same numbers; a path whose tracking decision sits on a rounding takes the
        # other branch, so all but a few pixels are equal and the image's mean is
        same = np.abs(img - want).max(axis=2) < 2e-4        # (the bar of the marched frames; a long path sums a few hundred terms)
        if verbose:
            dd = np.abs(img - want).max(axis=2)
            print("path tracing: pixels", same.size, "differing", int((~same).sum()), "mean |diff| of those", float(dd[~same].mean()) if (~same).any() else 0.0,
                  "image means", float(img[..., :3].mean()), float(want[..., :3].mean()), "lit pixels", float((want[..., :3].sum(axis=2) > 0).mean()),
                  "stats", st)
        assert np.array_equal(img[..., 3], want[..., 3]), "path tracing alpha"
        assert same.mean() > 0.99, ("path tracing pixels equal", float(same.mean()))
        assert abs(float(img[..., :3].mean()) - float(want[..., :3].mean())) < 1e-3, "path tracing mean"
    else:
        err = float(np.abs(img - want).max())
        assert err < 2e-4, ("frame", err)
    return d


def test_randomly_drawn_scenes_on_a_dense_volume_match_the_oracle(oracle):
    """the march itself, with the network out of the way: volumes of random ragged shapes (5..70 voxels an axis), transfer functions of random
    lengths and contents, cameras anywhere around (one in five INSIDE the volume), any field of view, frame shape, sampling rate and density
    scale, the volume scaled per axis and clipped to a box (in either order), rendering modes 4 / 5 (ray marching), 7 / 8 (gradient
    shading), 10 / 11 (single-shade heuristic) and 13 / 14 (path tracing).  Sampling and macrocells bit-exact; frames within 2e-4 of the
    oracle's (device powf against glibc's), hit rays and iterations equal for the streaming modes."""
    n = int(os.environ.get("VNR_FUZZ_SCENES", "60"))
    seed = int(os.environ.get("VNR_FUZZ_SEED", "20260410")) + 47
    only = [int(x) for x in os.environ.get("VNR_FUZZ_ONLY", "").split(",") if x]
    failures = []
    for i in (only or range(n)):
        try:
            d = scene_draw(oracle, seed, i, verbose=bool(only))
            msg = "ok"
        except Exception as e:
            d, msg = getattr(scene_draw, "last", i), "FAIL " + repr(e)[:300]
            failures.append((d, msg))
        if os.environ.get("VNR_FUZZ_LOG"):
            with open(os.environ["VNR_FUZZ_LOG"], "a") as f:
                f.write(f"scene {d} {msg}\n")
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ pixel shares
def test_randomly_drawn_pixel_shares_assemble_to_the_unsharded_frame(oracle):
    """the multi-GPU render path on one device (vnrRendererSetPixelInterleave / SetPixelRange): for random frame shapes (ragged against the
    8-scanline blocks the shares are cut in), world sizes 2..8, rendering modes 5 / 6 / 8 / 14 and
    both kinds of volume, every pixel of every rank's share is the unsharded frame's pixel bit for bit (a pixel's ray does not depend on
    which rays share its wave, its tile or its launch)."""
    from instantvnr_amd import dist as vdist
    n = int(os.environ.get("VNR_FUZZ_SHARES", "24"))
    rng = np.random.default_rng(int(os.environ.get("VNR_FUZZ_SEED", "20260410")) + 59)
    colors, alphas = syn.tfn_ramp_with_bumps()
    sv = api.vnrCreateSimpleVolume(syn.analytic_volume(32))
    tfn = api.vnrCreateTransferFunction()
    api.vnrTransferFunctionSetColor(tfn, colors); api.vnrTransferFunctionSetAlpha(tfn, alphas); api.vnrTransferFunctionSetValueRange(tfn, (0, 1))
    failures = []
    for i in range(n):
        size = (int(rng.integers(16, 180)), int(rng.integers(16, 120)))
        n_pixels = size[0] * size[1]
        world = int(rng.integers(2, 9))
        block = 8 * size[0]                      # the library's unit: 8 scanlines, one row of ray tiles (anything else is refused by name)
        mode = int(rng.choice([5, 6, 8, 14]))
        neural = bool(rng.uniform() < 0.6)
        d = dict(i=i, size=size, world=world, block=block, mode=mode, neural=neural)
        try:
            if neural:
                F = int(rng.choice([1, 2, 4, 8]))
                W = int(rng.choice([16, 32, 64, 64, 128]))
                cfg = syn.model_config(n_levels=int(rng.integers(2, 9)), n_features=F, log2_hashmap_size=12, base_resolution=4, n_hidden_layers=int(rng.integers(1, 4)))
                cfg["network"]["n_neurons"] = W
                volume = api.vnrCreateNeuralVolume(cfg, sv, online_macrocell_construction=False)
                info = api.neural_info(volume)
                api.neural_set_params_fp16(volume, syn.random_params(info["n_params"], oracle.mlp_n_params(info["padded_width"], W, cfg["network"]["n_hidden_layers"] - 1), seed=300 + i))
                d.update(F=F, W=W)
            else:
                volume = sv
            v = rng.normal(size=3); v /= np.linalg.norm(v)
            if abs(v[1]) > 0.95:
                v = np.array([0.6, 0.5, -0.62]); v /= np.linalg.norm(v)
            camera = api.vnrCreateCamera()
            api.vnrCameraSet(camera, tuple(float(x) for x in v * 32 * rng.uniform(0.9, 2.0)), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), float(rng.uniform(30, 70)))

            def renderer():
                r = api.vnrCreateRenderer(volume)
                api.vnrRendererSetTransferFunction(r, tfn); api.vnrRendererSetCamera(r, camera); api.vnrRendererSetFramebufferSize(r, size)
                api.vnrRendererSetMode(r, mode)
                return r

            r = renderer()
            api.vnrRender(r)
            want = api.vnrRendererMapFrame(r).reshape(-1, 4).copy()
            shares = []
            for part in range(world):
                rp = renderer()
                api.vnrRendererSetPixelInterleave(rp, block, world, part)
                api.vnrRender(rp)
                shares.append(vdist.pack_share(api.vnrRendererMapFrame(rp).reshape(-1, 4).copy(), block, world, part, n_pixels))
            n_local = max(s.shape[0] for s in shares)
            full = vdist.assemble_shares(np.stack([np.pad(s, ((0, n_local - s.shape[0]), (0, 0))) for s in shares]), block, world, n_pixels)
            assert np.array_equal(full, want), ("interleave", int((full != want).any(axis=1).sum()))
            lo = int(rng.integers(0, n_pixels - 1)); hi = int(rng.integers(lo + 1, n_pixels + 1))
            rr = renderer()
            api.vnrRendererSetPixelRange(rr, lo, hi)
            api.vnrRender(rr)
            assert np.array_equal(api.vnrRendererMapFrame(rr).reshape(-1, 4)[lo:hi], want[lo:hi]), ("range", lo, hi)
        except Exception as e:
            failures.append((d, repr(e)[:300]))
        if os.environ.get("VNR_FUZZ_LOG"):
            with open(os.environ["VNR_FUZZ_LOG"], "a") as f:
                f.write(f"shares {d} {'FAIL ' + failures[-1][1] if failures and failures[-1][0] is d else 'ok'}\n")
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ the optimizer
def optimizer_draw(oracle, seed, i, verbose=False):
    """one draw of the optimizer sweep (its own generator: a failing draw can be replayed alone, VNR_FUZZ_ONLY=<i>,<i>..)"""
    import ctypes as C
    from oracle import train_oracle as T
    from instantvnr_amd._lib import check, lib
    rng = np.random.default_rng([seed, i])
    F = int(rng.choice([1, 2, 4, 8])); L = int(rng.integers(1, 7)); W = int(rng.choice([16, 32, 64, 128])); H = int(rng.integers(1, 4))
    opt = dict(lr=float(10 ** rng.uniform(-4, -1.5)), beta1=float(rng.choice([0.0, 0.5, 0.9])), beta2=float(rng.choice([0.9, 0.99, 0.999])),
               eps=float(rng.choice([1e-15, 1e-8, 1e-3])), l2=float(rng.choice([0.0, 1e-8, 1e-6, 1e-3])))
    decay = None if rng.uniform() < 0.4 else dict(start=int(rng.integers(1, 5)), interval=int(rng.integers(1, 4)), base=float(rng.uniform(0.3, 0.9)))
    grad_scale = float(rng.choice([1.0, 0.5, 4.0]))
    d = dict(i=i, L=L, F=F, W=W, H=H, opt=opt, decay=decay, grad_scale=grad_scale)
    cfg = syn.model_config(n_levels=L, n_features=F, log2_hashmap_size=int(rng.integers(8, 13)), base_resolution=int(rng.integers(2, 6)), n_hidden_layers=H)
    cfg["network"]["n_neurons"] = W
    adam = {"otype": "Adam", "learning_rate": opt["lr"], "beta1": opt["beta1"], "beta2": opt["beta2"], "epsilon": opt["eps"], "l2_reg": opt["l2"]}
    cfg["optimizer"] = adam if decay is None else {"otype": "ExponentialDecay", "decay_start": decay["start"], "decay_interval": decay["interval"],
                                                   "decay_base": decay["base"], "nested": adam}
    vol = api.vnrCreateNeuralVolume(cfg, (16, 16, 16))
    info = api.neural_info(vol)
    N = info["n_params"]
    n_mlp = oracle.mlp_n_params(info["padded_width"], W, H - 1)
    params = syn.random_params(N, n_mlp, seed=500 + i)
    api.neural_set_params_fp16(vol, params)
    master = params.astype(np.float64); m = np.zeros(N); v = np.zeros(N); steps = np.zeros(N)
    lr, step_no = np.float32(opt["lr"]), 0
    history, slack, tied = [], np.zeros(N), np.zeros(N, bool)
    for step in range(6):
        g = np.zeros(N, np.float32)
        pick = rng.random(N) < (0.9 if step == 3 else 0.15)
        g[pick] = rng.normal(0, 10 ** rng.uniform(-4, 0), int(pick.sum())).astype(np.float16).astype(np.float32)
        g[rng.integers(0, N, 50)] = -0.0
        g[rng.integers(0, N, 50)] = 6e-8                       # the smallest subnormal half
        g = g.astype(np.float16).astype(np.float32)             # what the gradient blob can hold
        before = api.neural_get_params_fp16(vol).view(np.uint16).copy()
        check(lib().vnrAmdNeuralVolumeSetGradients(vol.h, g.ctypes.data_as(C.POINTER(C.c_float)), g.size))
        api.neural_train_end(vol, grad_scale)
        after = api.neural_get_params_fp16(vol)
        prev = (master, m, v, steps)
        master, m, v, steps = T.adam_step(master, g.astype(np.float64), m, v, steps, n_mlp, lr=float(lr), beta1=float(np.float32(opt["beta1"])),
                                          beta2=float(np.float32(opt["beta2"])), eps=float(np.float32(opt["eps"])),
                                          l2_reg=float(np.float32(opt["l2"])), grad_scale=grad_scale)
        history.append((g, prev, float(lr)))
        step_no += 1
        if decay is not None and step_no >= decay["start"] and step_no % decay["interval"] == 0:
            lr = np.float32(lr * np.float32(decay["base"]))
        want = master.astype(np.float32).astype(np.float16)
        untouched = np.ones(N, bool); untouched[:n_mlp] = False; untouched &= (g == 0)
        assert np.array_equal(after.view(np.uint16)[untouched], before[untouched]), (d, "an untouched grid entry moved", step)
        a, b = after.astype(np.float64), want.astype(np.float64)
        assert np.isfinite(a).all(), (d, "finite", step)
        # one half-precision ulp, or -- for a parameter the step carried next to zero, where halves are dense -- 1e-4 of the step it took:
        # the bias correction sqrt(1 - beta2^step) is evaluated in fp32 (a difference of nearly equal numbers: 3e-5 relative at
        # beta2 = 0.999, step 1), here and in the reference
        ulp = np.spacing(np.maximum(np.abs(after), np.abs(want)).astype(np.float16)).astype(np.float64)
        slack = slack + 1e-4 * np.abs(b - before.view(np.float16).astype(np.float64))      # (it stays with the parameter over the following steps)
        ulp = np.maximum(ulp, slack)
        off = a != b
        # a parameter whose fp64 master lies within fp32 rounding of the midpoint of two halves rounds either way.  That is not rare here: one
        # gradient followed by none makes Adam's step a constant (m / sqrt(v) = (1 - b1) / sqrt(1 - b2) whatever the gradient), and when
        # that constant is k + 1/2 ulps of a binade every parameter of the binade sits on a tie (draw 151 of seed 505: 64 of 512)
        tied = tied | (off & (np.abs(master - (a + b) / 2) <= 1e-5 * np.abs(master)))    # (and stays an ulp apart in the steps that follow)
        off = off & ~tied
        if verbose:
            print("draw", i, "step", step, "lr", float(lr), "an ulp off: all %.4f  mlp %.4f  grid %.4f  (touched grid entries %.3f)" %
                  (off.mean(), off[:n_mlp].mean(), off[n_mlp:].mean() if N > n_mlp else 0.0, (g[n_mlp:] != 0).mean() if N > n_mlp else 0.0), "N", N, "n_mlp", n_mlp)
        if verbose and off.mean() > 0.01:
            for k in np.flatnonzero(off)[:4]:
                print("   off by an ulp: element", int(k), "hip", a[k], "restatement", b[k], "fp64 master", master[k], "before", float(before[k:k + 1].view(np.float16)[0]))
                for s_, (g_, (ma, m_, v_, st_), lr_) in enumerate(history):
                    print("      step", s_, "g", g_[k], "master", ma[k], "m", m_[k], "v", v_[k], "steps", st_[k], "lr", lr_)
        if verbose and (np.abs(a - b) > ulp).any():
            k = int(np.argmax(np.abs(a - b) / ulp))
            print("draw", d, "step", step, "element", k, "of", N, "(n_mlp", n_mlp, ") hip", a[k], "restatement", b[k], "fp64 master", master[k],
                  "before", float(before[k:k + 1].view(np.float16)[0]))
            for s_, (g_, (ma, m_, v_, st_), lr_) in enumerate(history):
                print("   step", s_, "g", g_[k], "master", ma[k], "m", m_[k], "v", v_[k], "steps", st_[k], "lr", lr_)
        assert (np.abs(a - b) <= ulp).all(), (d, "more than an ulp", step, float(np.abs(a - b).max()), int((np.abs(a - b) > ulp).sum()))
        assert off.sum() <= max(3, (2e-3 + 0.5 * opt["lr"]) * N), (d, "fraction of parameters an ulp off", step, float(off.mean()), int(off.sum()))   # (the same 3e-5 of a step of ~lr against a half's ulp)
    assert api.vnrNeuralVolumeGetTrainingStep(vol) == 6
    assert np.all(api.neural_gradients(vol) == 0), "gradients cleared"
    return d


def test_randomly_drawn_optimizers_follow_the_restatement_step_by_step(oracle):
    """EXTERNAL tcnn Adam / ExponentialDecay{Adam} (restated in oracle/train_oracle.py::adam_step) under random hyper-parameters: learning
    rate 1e-4..3e-2, beta1 0 / 0.5 / 0.9, beta2 0.9 / 0.99 / 0.999, epsilon 1e-15 / 1e-8 / 1e-3, l2_reg 0..1e-3, a decay schedule that
    starts within the run, grad_scale 1 / 0.5 / 4; six steps on injected gradients (sparse on the grid: untouched entries must not move,
    their step counters must not advance; zeros, negative zeros and the smallest halves among them).  After every step the fp16 parameters
    equal the fp64 restatement's, rounded: at most one half-precision ulp apart (1e-4 of the step for a parameter that lands next to zero),
    and that on fewer than 0.2 % + lr / 2 of them (fp32 state and the bias correction 1 - beta2^step evaluated in fp32, as in the reference,
    against fp64)."""
    n = int(os.environ.get("VNR_FUZZ_OPTIMIZERS", "30"))
    seed = int(os.environ.get("VNR_FUZZ_SEED", "20260410")) + 71
    only = [int(x) for x in os.environ.get("VNR_FUZZ_ONLY", "").split(",") if x]
    failures = []
    for i in (only or range(n)):
        try:
            d = optimizer_draw(oracle, seed, i, verbose=bool(only))
            msg = "ok"
        except Exception as e:
            d, msg = i, "FAIL " + repr(e)[:600]
            failures.append((i, msg))
        if os.environ.get("VNR_FUZZ_LOG"):
            with open(os.environ["VNR_FUZZ_LOG"], "a") as f:
                f.write(f"optimizer {d} {msg}\n")
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ damaged descriptions
POOL = [0, -1, 1, 2, 3, 7, 16, 17, 33, 64, 100, 1000, 2 ** 31, 2 ** 32 + 5, 0.5, -2.5, 1e30, 1e-30, "x", "", "ReLU", "Hash", "Adam", None, True, False, [], {},
        [1, 2], {"otype": "Adam"}]


def _paths(doc, prefix=()):
    out = []
    for k, v in doc.items():
        out.append(prefix + (k,))
        if isinstance(v, dict):
            out += _paths(v, prefix + (k,))
    return out


def test_damaged_model_descriptions_are_refused_by_name_or_run(oracle):
    """a model description with keys missing, values of the wrong type, negative, fractional, absurdly large or small: the library either
    refuses it with a message (the reference: a tcnn / nlohmann exception) or builds a network that evaluates and trains without a
    fault -- never a crash, a hang, or a silent fallback.  (Sizes are kept where a mistaken success cannot exhaust the host.)"""
    import copy
    n = int(os.environ.get("VNR_FUZZ_DAMAGED", "150"))
    seed = int(os.environ.get("VNR_FUZZ_SEED", "20260410")) + 83
    sv = api.vnrCreateSimpleVolume(syn.analytic_volume(16))
    coords = np.random.default_rng(1).uniform(0, 1, (65, 3)).astype(np.float32)
    refused, ran, messages = 0, 0, set()
    for i in range(n):
        rng = np.random.default_rng([seed, i])
        cfg = copy.deepcopy(syn.model_config(n_levels=4, n_features=2, log2_hashmap_size=10, base_resolution=4, n_hidden_layers=2))
        for _ in range(int(rng.integers(1, 4))):
            paths = _paths(cfg)
            if not paths:
                break
            path = paths[int(rng.integers(0, len(paths)))]
            node = cfg
            for k in path[:-1]:
                node = node[k]
            if rng.uniform() < 0.3:
                del node[path[-1]]
            else:
                node[path[-1]] = copy.deepcopy(POOL[int(rng.integers(0, len(POOL)))])
        enc = cfg.get("encoding", {}) if isinstance(cfg.get("encoding"), dict) else {}
        if isinstance(enc.get("log2_hashmap_size"), (int, float)) and 22 < enc["log2_hashmap_size"] <= 28:
            enc["log2_hashmap_size"] = 22
        try:
            vol = api.vnrCreateNeuralVolume(cfg, sv)
        except api.VnrAmdError as e:
            refused += 1
            assert str(e), cfg
            messages.add(str(e)[:60])
            continue
        try:
            out = api.neural_inference(vol, coords)
            assert out.shape == (65,)
            api.vnrNeuralVolumeTrain(vol, 2, True)
            api.neural_inference(vol, coords)
            ran += 1
        except api.VnrAmdError as e:           # a description that builds but cannot run must say so as well
            refused += 1
            assert str(e), cfg
            messages.add(str(e)[:60])
        if os.environ.get("VNR_FUZZ_LOG"):
            with open(os.environ["VNR_FUZZ_LOG"], "a") as f:
                f.write(f"damaged {i} ok\n")
    assert refused > n // 10 and ran > n // 10, (refused, ran)
    assert len(messages) >= 8, messages          # many different refusals, by name


def test_damaged_scene_descriptions_are_refused_by_name_or_load(oracle, tmp_path):
    """a scene document (serializer.cpp:137-477) whose description does not match its file -- dimensions larger than the file, negative,
    zero, 2^31, an offset behind the end, a missing file, a wrong type name, keys missing or of the wrong type -- in both of the reference's
    formats and both loading modes: refused with a message before anything of the claimed size is allocated, or loaded and sampled."""
    import copy
    n = int(os.environ.get("VNR_FUZZ_DAMAGED", "150"))
    seed = int(os.environ.get("VNR_FUZZ_SEED", "20260410")) + 97
    dims = (20, 12, 9)
    rng0 = np.random.default_rng(0)
    raw = tmp_path / "v.raw"
    with open(raw, "wb") as f:
        f.write(b"\0" * 16)
        f.write(rng0.integers(0, 255, dims[::-1], dtype=np.uint8).tobytes())
    vidi = {"dataSource": [{"format": "REGULAR_GRID_RAW_BINARY", "fileName": str(raw), "dimensions": {"x": dims[0], "y": dims[1], "z": dims[2]},
                            "type": "UNSIGNED_BYTE", "offset": 16, "endian": "LITTLE_ENDIAN"}],
            "view": {"volume": {"transferFunction": {}, "scalarMappingRangeUnnormalized": {"minimum": 3.0, "maximum": 200.0}}}}
    diva = {"version": "DIVA", "volume": {"dims": {"x": dims[0], "y": dims[1], "z": dims[2]}, "type": "UNSIGNED_BYTE", "offset": 16,
                                          "range": {"x": 3.0, "y": 200.0}, "filename": str(raw)}}
    pool = POOL + [dims[0] + 1, 4096, 100000, -5, 15, 17, 2160, 2161, "FLOAT", "DOUBLE", "UNSIGNED_SHORT", "BYTE", "BIG_ENDIAN", str(tmp_path), str(tmp_path / "nope.raw"),
                   {"x": 4096, "y": 4096, "z": 4096}, {"x": -1, "y": 12, "z": 9}, {"x": 20, "y": 12}, [str(tmp_path / "nope.raw"), str(raw)]]
    coords = np.random.default_rng(1).uniform(0, 1, (33, 3)).astype(np.float32)
    refused, loaded, messages = 0, 0, set()
    os.environ.setdefault("VNR_NUM_CONCURRENT_BLOCKS", "2"); os.environ.setdefault("VNR_NUM_BLOCKS", "4")
    for i in range(n):
        rng = np.random.default_rng([seed, i])
        sc = copy.deepcopy(vidi if rng.uniform() < 0.6 else diva)
        for _ in range(int(rng.integers(1, 3))):
            root = sc["dataSource"][0] if "dataSource" in sc and isinstance(sc.get("dataSource"), list) and sc["dataSource"] and rng.uniform() < 0.7 else sc
            if not isinstance(root, dict):
                break
            paths = _paths(root)
            if not paths:
                break
            path = paths[int(rng.integers(0, len(paths)))]
            node = root
            for k in path[:-1]:
                node = node[k]
            if rng.uniform() < 0.25:
                del node[path[-1]]
            else:
                node[path[-1]] = copy.deepcopy(pool[int(rng.integers(0, len(pool)))])
        mode = "GPU" if rng.uniform() < 0.7 else "OUT_OF_CORE"
        try:
            sv = api.vnrCreateSimpleVolume(sc, mode)
            d = api.vnrVolumeGetDims(sv)
            assert all(0 < q <= 4096 for q in d), d
            if mode == "GPU":
                out = api.simple_volume_sample(sv, coords, nodal=False)
                assert out.shape == (33,)        # (random bytes read as FLOAT / DOUBLE hold NaNs: the values are the file's business)
            loaded += 1
        except api.VnrAmdError as e:
            refused += 1
            assert str(e), sc
            messages.add(str(e)[:50])
        if os.environ.get("VNR_FUZZ_LOG"):
            with open(os.environ["VNR_FUZZ_LOG"], "a") as f:
                f.write(f"scene-description {i} ok\n")
    assert refused > n // 10 and loaded > n // 10, (refused, loaded)
    assert len(messages) >= 8, messages


def test_damaged_params_files_are_refused_by_name_or_load(oracle):
    """a params.json (BSON: volume.dims + model + parameters + macrocell, network.cu:827-877) with bytes flipped, lengths overwritten or
    its tail cut off, outside the parameter blob: refused with a message or loaded into a network that evaluates"""
    import struct
    n = int(os.environ.get("VNR_FUZZ_DAMAGED", "150"))
    seed = int(os.environ.get("VNR_FUZZ_SEED", "20260410")) + 101
    cfg = syn.model_config(n_levels=4, n_features=2, log2_hashmap_size=9, base_resolution=4, n_hidden_layers=2)
    sv = api.vnrCreateSimpleVolume(syn.analytic_volume(16))
    vol = api.vnrCreateNeuralVolume(cfg, sv)
    info = api.neural_info(vol)
    params = syn.random_params(info["n_params"], oracle.mlp_n_params(info["padded_width"], 64, 1), seed=5)
    api.neural_set_params_fp16(vol, params)
    good = api.vnrNeuralVolumeSerializeParams(vol)
    blob_at = good.find(params.tobytes())
    assert blob_at > 0
    outside = np.concatenate([np.arange(0, blob_at), np.arange(blob_at + params.nbytes, len(good))])
    coords = np.random.default_rng(1).uniform(0, 1, (65, 3)).astype(np.float32)
    want = api.neural_inference(api.vnrCreateNeuralVolume(good), coords)
    refused, loaded, same, messages = 0, 0, 0, set()
    for i in range(n):
        rng = np.random.default_rng([seed, i])
        b = bytearray(good)
        for _ in range(int(rng.integers(1, 4))):
            k = rng.integers(0, 4)
            p = min(int(outside[int(rng.integers(0, outside.size))]), len(b) - 1)      # (an earlier cut may have shortened it)
            if k == 0: b[p] = int(rng.integers(0, 256))
            elif k == 1: b[p] ^= 1 << int(rng.integers(0, 8))
            elif k == 2 and p + 4 <= len(b): struct.pack_into("<i", b, p, int(rng.choice([-1, 0, 1, 5, 28, 2 ** 31 - 1, len(b), params.nbytes + 1, params.nbytes - 1, int(rng.integers(-100, 70000))])))
            else: b = b[:max(5, p)]
        try:
            v2 = api.vnrCreateNeuralVolume(bytes(b))
            out = api.neural_inference(v2, coords)
            assert out.shape == (65,)
            loaded += 1
            same += int(np.array_equal(out.view(np.uint32), want.view(np.uint32)))
        except api.VnrAmdError as e:
            refused += 1
            assert str(e)
            messages.add(str(e)[:50])
        if os.environ.get("VNR_FUZZ_LOG"):
            with open(os.environ["VNR_FUZZ_LOG"], "a") as f:
                f.write(f"params-file {i} ok\n")
    assert refused > n // 4 and loaded > n // 50, (refused, loaded, same)
    assert len(messages) >= 5, messages


# ------------------------------------------------------------------------------------------------ odd renderer parameters
def test_odd_renderer_parameters_are_refused_or_rendered_never_fatal(oracle):
    """what an interactive application sends while its user drags sliders: a camera at its own focus, an up vector along the view, a field
    of view of 0 / 180 / NaN, a clipping box inside out, a value range of zero width, one-entry transfer functions, frames of one pixel,
    empty pixel ranges, density 0 / huge / NaN, NaN anywhere -- in every rendering mode, on a dense and on a neural volume.  Every call
    either fails with a message or returns; frames may hold anything; nothing faults or hangs."""
    n = int(os.environ.get("VNR_FUZZ_ODD", "120"))
    seed = int(os.environ.get("VNR_FUZZ_SEED", "20260410")) + 113
    sv = api.vnrCreateSimpleVolume(syn.analytic_volume(32))
    cfg = syn.model_config(n_levels=4, n_features=2, log2_hashmap_size=12, base_resolution=4, n_hidden_layers=2)
    nv = api.vnrCreateNeuralVolume(cfg, sv, online_macrocell_construction=False)
    info = api.neural_info(nv)
    api.neural_set_params_fp16(nv, syn.random_params(info["n_params"], oracle.mlp_n_params(info["padded_width"], 64, 1), seed=3))
    nan, inf = float("nan"), float("inf")
    F = [0.0, 1.0, -1.0, 1e-30, 1e30, -1e30, nan, inf, -inf, 0.5, 45.0, 16.0, 33.0]
    refused = rendered = 0
    messages = set()
    for i in range(n):
        rng = np.random.default_rng([seed, i])
        pick = lambda pool=F: float(pool[int(rng.integers(0, len(pool)))])      # noqa: E731
        vec = lambda: tuple(pick() if rng.uniform() < 0.08 else float(rng.normal() * 40) for _ in range(3))   # noqa: E731
        volume = nv if rng.uniform() < 0.5 else sv
        calls = []
        try:
            tfn = api.vnrCreateTransferFunction()
            nc, na = int(rng.choice([1, 2, 3, 256])), int(rng.choice([1, 2, 3, 256]))
            colors = rng.uniform(0, 1, (nc, 3)).astype(np.float32); alphas = rng.uniform(0, 1, na).astype(np.float32)
            if rng.uniform() < 0.2: colors[int(rng.integers(0, nc))] = pick()
            if rng.uniform() < 0.2: alphas[int(rng.integers(0, na))] = pick()
            api.vnrTransferFunctionSetColor(tfn, colors); api.vnrTransferFunctionSetAlpha(tfn, alphas)
            api.vnrTransferFunctionSetValueRange(tfn, (pick([0.0, 0.0, 0.5, 1.0, nan, -1.0]), pick([1.0, 1.0, 0.5, 0.0, nan, inf])))
            camera = api.vnrCreateCamera()
            frm = vec()
            at = frm if rng.uniform() < 0.05 else (vec() if rng.uniform() < 0.3 else (0.0, 0.0, 0.0))
            up = (0.0, 1.0, 0.0) if rng.uniform() < 0.7 else (tuple(a - b for a, b in zip(at, frm)) if rng.uniform() < 0.25 else vec())
            api.vnrCameraSet(camera, frm, at, up, pick([45.0, 45.0, 60.0, 30.0, 0.0, 1e-3, 179.99, 180.0, 360.0, -30.0, nan]))
            r = api.vnrCreateRenderer(volume)
            api.vnrRendererSetTransferFunction(r, tfn); api.vnrRendererSetCamera(r, camera)
            size = (int(rng.choice([1, 2, 7, 64])), int(rng.choice([1, 3, 8, 48])))
            calls.append(("size", size)); api.vnrRendererSetFramebufferSize(r, size)
            mode = int(rng.choice([5, 6, 8, 9, 11, 12, 14, 15])) if rng.uniform() < 0.8 else int(rng.integers(4, 16))      # (4 / 7 / 10 / 13 need a decoded volume)
            calls.append(("mode", mode)); api.vnrRendererSetMode(r, mode)
            if rng.uniform() < 0.5:
                rate = pick([1.0, 0.25, 8.0, 2.0, 0.5, 1e-3, 0.0, -1.0, nan, inf])
                calls.append(("rate", rate)); api.vnrRendererSetVolumeSamplingRate(r, rate)
            if rng.uniform() < 0.5:
                dens = pick([1.0, 0.0, 1e-3, 100.0, 1e30, -1.0, nan, inf])
                calls.append(("density", dens)); api.vnrRendererSetVolumeDensityScale(r, dens)
            if rng.uniform() < 0.3:
                lo, hi = vec(), vec()
                calls.append(("clip", lo, hi)); api.vnrVolumeSetClippingBox(volume, tuple(x / 40 for x in lo), tuple(x / 40 for x in hi))
            if rng.uniform() < 0.3:
                n_px = size[0] * size[1]
                lo = int(rng.integers(0, n_px + 1)); hi = int(rng.integers(0, n_px + 3))
                calls.append(("range", lo, hi)); api.vnrRendererSetPixelRange(r, lo, hi)
            for _ in range(2):
                api.vnrRender(r)
                img = api.vnrRendererMapFrame(r)
                assert img.shape == (size[1], size[0], 4)
            rendered += 1
        except api.VnrAmdError as e:
            refused += 1
            assert str(e), calls
            messages.add(str(e)[:50])
        finally:
            api.vnrVolumeSetClippingBox(volume, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        if os.environ.get("VNR_FUZZ_LOG"):
            with open(os.environ["VNR_FUZZ_LOG"], "a") as f:
                f.write(f"odd-renderer {i} {calls} ok\n")
    assert rendered > n // 4 and refused > n // 10, (rendered, refused, messages)


# ------------------------------------------------------------------------------------------------ marching cubes
def test_randomly_drawn_volumes_give_the_restatement_s_triangles(oracle):
    """vnrMarchingCube (core/marching_cube.cu) on ragged volumes (2..40 voxels an axis, incl. a single layer of cells), smooth fields,
    noise (every ambiguous case) and data quantised to a few levels with the isovalue ON a level (ties in every comparison): the same
    cells in the same order with the same bits as oracle/mc_oracle.py"""
    from oracle import mc_oracle
    n = int(os.environ.get("VNR_FUZZ_MC", "30"))
    seed = int(os.environ.get("VNR_FUZZ_SEED", "20260410")) + 131
    total = 0
    for i in range(n):
        rng = np.random.default_rng([seed, i])
        dims = tuple(int(v) for v in rng.integers(2, 41, 3))             # (nz, ny, nx)
        kind = int(rng.integers(0, 3))
        z, y, x = np.meshgrid(*[np.linspace(0, 1, q) for q in dims], indexing="ij")
        k = rng.uniform(1, 9, 3); ph = rng.uniform(0, 6.28, 3)
        f = 0.5 + 0.5 * np.sin(k[0] * x + ph[0]) * np.sin(k[1] * y + ph[1]) * np.sin(k[2] * z + ph[2])
        if kind == 1:
            f = rng.uniform(0, 1, dims)
        f = ((f - f.min()) / max(f.max() - f.min(), 1e-9)).astype(np.float32)
        iso = float(rng.uniform(0.05, 0.95))
        if kind == 2:                                                      # a few levels, the isovalue on one of them
            levels = int(rng.integers(3, 9))
            f = (np.round(f * (levels - 1)) / np.float32(levels - 1)).astype(np.float32)
            iso = float(np.float32(int(rng.integers(1, levels - 1)) / np.float32(levels - 1))) if levels > 2 else 0.5
        f[tuple(rng.integers(0, q) for q in dims)] = 1.0; f[tuple(rng.integers(0, q) for q in dims)] = 0.0   # min / max stay 0 / 1: the library's normalisation is the identity
        if f.min() != 0.0 or f.max() != 1.0:
            continue
        sv = api.vnrCreateSimpleVolume(f)
        got = api.vnrMarchingCube(sv, iso)
        want = mc_oracle.marching_cubes(f, iso)
        assert got.shape == want.shape, (i, dims, kind, iso, got.shape, want.shape)
        assert np.array_equal(got, want), (i, dims, kind, iso)
        total += got.shape[0]
    assert total > 1000 * max(1, n // 10), total


# ------------------------------------------------------------------------------------------------ out-of-core sampler
def test_randomly_drawn_files_sample_like_the_oracle_out_of_core(oracle, tmp_path):
    """the out-of-core training sampler (neural_sampler.cpp:377-668, 1043-1127) on files of random shapes (1..9 x 5..90 x 8..300 voxels:
    slab geometry, ghost layers and the ragged last slab all move), every voxel type, header offsets, resident / replaced slab counts,
    ragged batch sizes and sub-boxes: slab geometry equal to the oracle's, and with the library's slot table handed to the oracle the
    coordinates and values of every batch bit for bit"""
    from test_gpu_ooc import SEED, STREAM
    n = int(os.environ.get("VNR_FUZZ_OOC", "20"))
    seed = int(os.environ.get("VNR_FUZZ_SEED", "20260410")) + 149
    for i in range(n):
        rng = np.random.default_rng([seed, i])
        dtype = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64][int(rng.integers(0, 8))]
        shape = (int(rng.integers(1, 10)), int(rng.integers(5, 91)), int(rng.integers(8, 301)))      # (nz, ny, nx)
        header = int(rng.choice([0, 0, 16, 24, 513]))
        if np.issubdtype(dtype, np.integer):
            ii = np.iinfo(dtype)
            vol = rng.integers(ii.min, ii.max, shape, dtype=dtype)
            vr = (float(ii.min) + 2.0, float(ii.max) - 7.0)
        else:
            vol = rng.normal(0, 1, shape).astype(dtype)
            vr = (-1.25, 1.75)
        path = tmp_path / f"v{i}.raw"
        with open(path, "wb") as f:
            f.write(b"\xab" * header); f.write(vol.tobytes())
        dims = shape[::-1]
        g = oracle.ooc_geometry(dims, dtype)
        n_blocks = int(rng.integers(2, 41))
        n_conc = int(rng.integers(1, n_blocks + 1))
        d = dict(i=i, dtype=np.dtype(dtype).name, dims=dims, header=header, n_blocks=n_blocks, n_concurrent=n_conc)
        sv = api.vnrCreateSimpleVolumeOutOfCore(path, dims, dtype, vr, offset=header, n_concurrent_blocks=n_conc, n_blocks=n_blocks)
        info = api.out_of_core_info(sv)
        assert info["block_dims"] == tuple(g.block_dims) and info["block_index_space"] == tuple(g.index_space), d
        assert info["block_size_aligned"] == g.block_size_aligned, d
        offset = 0
        for step in range(3):
            nb = int(rng.choice([1, 63, 1000, 4097]))
            blocks = api.out_of_core_blocks(sv)
            if rng.uniform() < 0.5:
                lower, upper = (0, 0, 0), (1, 1, 1)
            else:
                a_, b_ = np.sort(rng.uniform(0, 1, (2, 3)), axis=0)
                lower, upper = tuple(float(np.float32(q)) for q in a_), tuple(float(np.float32(q)) for q in b_)
            c, v = api.simple_volume_take_samples(sv, nb, lower, upper)
            r = oracle.pcg32_floats(5 * nb, offset, SEED, STREAM)
            wc, wv, bad = oracle.OocSlabSet(vol, blocks).sample(vr, r[:3 * nb].reshape(nb, 3), r[3 * nb:4 * nb], r[4 * nb:], lower, upper)
            assert bad == 0, d
            assert np.array_equal(c, wc), (d, step, "coordinates")
            assert np.array_equal(v, wv), (d, step, "values")
            offset += 5 * nb
        os.remove(path)
        if os.environ.get("VNR_FUZZ_LOG"):
            with open(os.environ["VNR_FUZZ_LOG"], "a") as f:
                f.write(f"ooc {d} ok\n")


# ------------------------------------------------------------------------------------------------ decoding
def test_randomly_shaped_volumes_decode_to_the_network_s_values(oracle):
    """vnrNeuralVolumeDecodeProgressive (network.cu:290-405) on ragged shapes (the last blob of 16 z-slices is short, rows and slices of odd
    length), blob by blob: what has been decoded equals the library's own inference at the voxel centres bit for bit (generate_coords,
    network.cu:51-68: x fastest, (i + 0.5) / dims), the rest is still zero, and the whole volume is within 2^-8 of the oracle's network"""
    n = int(os.environ.get("VNR_FUZZ_DECODE", "12"))
    seed = int(os.environ.get("VNR_FUZZ_SEED", "20260410")) + 163
    for i in range(n):
        rng = np.random.default_rng([seed, i])
        dims = (int(rng.integers(1, 60)), int(rng.integers(1, 60)), int(rng.integers(1, 70)))      # (nx, ny, nz)
        d = draw(rng)
        d["L"] = min(d["L"], 6); d["log2T"] = min(d["log2T"], 12); d["H"] = min(d["H"], 3); d["max_level"] = None
        if d["gtype"] == "Dense": d["L"] = min(d["L"], 3)
        if d["act"] in ("Exponential", "Softplus"): d["act"] = "ReLU"
        if d["out_act"] == "Exponential": d["out_act"] = "None"
        cfg = syn.model_config(n_levels=d["L"], n_features=d["F"], log2_hashmap_size=d["log2T"], base_resolution=d["base"], n_hidden_layers=d["H"],
                               per_level_scale=d["pls"])
        cfg["encoding"]["interpolation"] = d["interp"]; cfg["network"]["n_neurons"] = d["W"]
        cfg["network"]["activation"] = d["act"]; cfg["network"]["output_activation"] = d["out_act"]
        if d["gtype"] != "Hash": cfg["encoding"]["type"] = d["gtype"]
        nv = api.vnrCreateNeuralVolume(cfg, dims)
        info = api.neural_info(nv)
        n_mlp = oracle.mlp_n_params(info["padded_width"], d["W"], d["H"] - 1)
        params = syn.random_params(info["n_params"], n_mlp, seed=700 + i)
        api.neural_set_params_fp16(nv, params)
        nx, ny, nz = dims
        coords = oracle.grid_coords((0, 0, 0), dims, (1.0 / nx, 1.0 / ny, 1.0 / nz))
        mine = api.neural_inference(nv, coords).reshape(nz, ny, nx)
        blobs = api.vnrNeuralVolumeGetNumberOfBlobs(nv)
        assert blobs == (nz + 15) // 16, (dims, blobs)
        for b in range(blobs):
            api.vnrNeuralVolumeDecodeProgressive(nv)
            dec = api.neural_decoded_volume(nv, dims)
            done = min(nz, 16 * (b + 1))
            assert np.array_equal(dec[:done].view(np.uint32), mine[:done].view(np.uint32)), (i, dims, d, b)
            assert not dec[done:].any(), (i, dims, b)
        ocfg = oracle.grid_config(d["L"], d["F"], d["log2T"], d["base"], d["pls"], INTERP[d["interp"]], 0.0, 1000.0, d["gtype"])
        want = oracle.network_inference(ocfg, d["W"], d["H"], params.view(np.uint16), coords, activation=oracle.act_code(d["act"], d["out_act"])).reshape(nz, ny, nx)
        if np.isfinite(want).all():
            assert np.abs(dec - want).max() <= TOL_ABS * max(1.0, np.abs(want).max()), (i, dims, d)
