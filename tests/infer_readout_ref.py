"""The inference kernel's own hidden activations, read out through its output, and every layer held to the stage bounds of
tests/mlp_stage_ref.py (DESIGN.md 4.3 "the chain", the inference side).  fused_infer_kernel<F, K_IN, W, 0, GENERAL> stores nothing but its
output, so the output is made to BE a hidden unit:

  * row 0 of the last layer = e_j (exactly 1.0 at j, 0 elsewhere), output activation None: the v_dot2 chain of mlp_column_tile sums one product
    of a half with 1.0 and exact zeros, in whatever order, and finish_output rounds a half to half: the output is unit j of the last hidden
    layer, bit for bit;
  * every hidden matrix behind layer k = the identity: unit j of layer k passes each of them as one product with 1.0 among exact zeros and is
    rounded to the half it already is; activation None leaves it, ReLU leaves it because it is a ReLU's output (>= 0).  Any other activation
    changes it: then only the last hidden layer can be read.

W launches per layer give that layer's [n][W] activations as THIS kernel computed them; each stage is then checked from its own inputs with
R.forward_hidden / R.output, as the training step's stages are from its stored buffers.  No bound is introduced here.  A fault of the kernel
behind layer k also garbles the readout of the layers in front of it (their values pass through it): the stage where it was made misses, and
possibly earlier ones too.  A fault in the last row's v_dot2 chain garbles the channel itself and shows at the hidden stages.
A helper module of tests/test_infer_readout_host.py (which proves all this on a simulated kernel) and tests/test_gpu_inference_stages.py, not
a test file."""
import numpy as np

import mlp_stage_ref as R
from oracle import train_oracle as T

INVERTIBLE = (0, 1)          # hidden activations a hidden unit passes an identity row through unchanged: None, ReLU


def _dims(shape):
    return shape["W"], shape["in_w"], shape["H"] - 1


def readable_layers(shape):
    """the hidden layers (0 .. nh) whose activations the output can be made to be"""
    nh = shape["H"] - 1
    return list(range(nh + 1)) if R.code(shape["act"]) in INVERTIBLE else [nh]


def probe_params(mlp, shape, layer, unit):
    """the MLP part of the blob (layout: oracle.train_oracle.split_mlp) that makes the output unit `unit` of hidden layer `layer`: the hidden
    matrices layer + 1 .. nh (matrix k produces layer k) are the identity, the 16 rows of the last layer are zero except wl[0][unit] = 1; the
    first layer and the matrices up to `layer` are the model's"""
    W, in_w, nh = _dims(shape)
    assert 0 <= layer <= nh and 0 <= unit < W
    assert layer == nh or R.code(shape["act"]) in INVERTIBLE, "only None and ReLU pass a hidden unit through an identity matrix unchanged"
    p = np.array(np.asarray(mlp).view(np.float16) if np.asarray(mlp).dtype == np.uint16 else mlp, np.float16)
    off = W * in_w
    assert p.size == off + nh * W * W + 16 * W
    for m in range(layer, nh):
        p[off + m * W * W:off + (m + 1) * W * W] = np.eye(W, dtype=np.float16).ravel()
    p[off + nh * W * W:] = 0
    p[off + nh * W * W + unit] = 1
    return p


def is_half(y):
    """which of the float32 values are exactly halves (NaN is none)"""
    y = np.asarray(y, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return y.astype(np.float16).astype(np.float32).view(np.uint32) == y.view(np.uint32)


def readout(evaluate, mlp, shape, layers):
    """[len(layers)][n][W] halves: the activations of the hidden layers `layers`, one evaluation per unit.  evaluate(mlp_params) -> [n] float32
    is the network with that MLP part, the model's grid and OUTPUT ACTIVATION NONE: the only thing here that touches a device"""
    W = shape["W"]
    out = None
    for i, layer in enumerate(layers):
        for j in range(W):
            y = np.asarray(evaluate(probe_params(mlp, shape, layer, j)), np.float32)
            assert y.ndim == 1
            ok = is_half(y)
            assert ok.all(), ("layer %d unit %d: the probe's output is no half, so it is not a hidden unit" % (layer, j), int((~ok).sum()), y[~ok][:4])
            if out is None:
                out = np.zeros((len(layers), y.size, W), np.float16)
            out[i, :, j] = y.astype(np.float16)
    return out


def cut_model(mlp, shape, layer):
    """(mlp part, shape) of the model cut off behind hidden layer `layer`: its LAST hidden layer is that layer, so it can be read whatever the
    activation.  It stands in for the layer in front of the last when a transcendental activation hides it (check_inference, stand_in)"""
    W, in_w, nh = _dims(shape)
    assert 0 <= layer < nh
    p = np.asarray(mlp, np.float16)
    head = W * in_w + layer * W * W
    return np.concatenate([p[:head], p[W * in_w + nh * W * W:]]), dict(shape, H=layer + 1)


def check_inference(features, readouts, y, mlp, shape, stand_in=None):
    """every stage of one inference from its own inputs.  features [n][in_w] halves (vnrAmdNeuralVolumeEncode), readouts {layer: [n][W]} (or a
    sequence: layers 0 .. nh), y [n] float32 the model's real output, mlp the model's real MLP part.  A stage is checked when its input was read:
    "layer 0" from the features, "layer k" from layer k - 1, "output" from layer nh; every other stage is listed in stats["not observable"].
    stand_in: the activations of layer nh - 1 read from cut_model(mlp, shape, nh - 1), the input of layer nh where that layer itself cannot be
    read (the stages in front stay "not observable": what the cut model computes is not what this one does).
    -> R.Report(failures, ratios: largest error / bound per stage, stats: zero / sharp shares per stage, "not observable")"""
    W, in_w, nh = _dims(shape)
    act, out_act = R.code(shape["act"]), R.code(shape["out_act"])
    w1, wh, wl, _ = T.split_mlp(mlp, in_w, W, nh)
    if not isinstance(readouts, dict):
        readouts = dict(enumerate(readouts))
    assert all(0 <= l <= nh for l in readouts) and nh in readouts
    reads = {l: R.f64(a) for l, a in readouts.items()}
    inputs = {0: R.f64(features)}
    inputs.update({l + 1: a for l, a in reads.items() if l < nh})
    failures, ratios, stats = [], {}, {"zero": {}, "sharp": {}, "not observable": [], "stand-in": []}
    if stand_in is not None and nh >= 1 and nh not in inputs:
        inputs[nh] = R.f64(stand_in)
        stats["stand-in"].append("layer %d" % (nh - 1))
    for l in range(nh + 1):
        name = "layer %d" % l
        if l not in reads or l not in inputs:
            stats["not observable"].append(name)
            continue
        st = R.forward_hidden(inputs[l], w1 if l == 0 else wh[l - 1], act)
        R._miss(failures, ratios, name, reads[l], st)
        stats["zero"][name], stats["sharp"][name] = R._shares(st)
    y = np.asarray(y, np.float32)
    st = R.output(reads[nh], wl[0], out_act)
    R._miss(failures, ratios, "output", y, st)
    stats["zero"]["output"], stats["sharp"]["output"] = R._shares(st)
    if not is_half(y).all():          # finish_output rounds to half: an output that is none was taken before that
        bad = np.argwhere(~is_half(y))
        failures.append(("output", len(bad), [tuple(int(q) for q in b) for b in bad[:4]], float(y[tuple(bad[0])]), "not a half", 0.0, 0.0))
    return R.Report(failures, ratios, stats)


def vacuous(report):
    """the forward stages' rule of R.vacuous: in every stage checked, the bound holds at least 9/10 of the (non-zero) elements to 2^-6 of their
    value; and at least the output stage and one hidden stage were checked.  -> list of the conditions missed"""
    out = [("sharp share", name, s) for name, s in report.stats["sharp"].items() if not s >= 0.9]
    if len(report.stats["sharp"]) < 2:
        out.append(("stages checked", sorted(report.stats["sharp"]), len(report.stats["sharp"])))
    return out


def ratios_line(name, n, report):
    line = "%s n=%d: " % (name, n) + ", ".join("%s %.3f" % kv for kv in sorted(report.ratios.items()))
    if report.stats["not observable"]:
        line += "; not observable: " + ", ".join(report.stats["not observable"])
    return line
