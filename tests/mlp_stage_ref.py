"""numpy restatement of every stage of the MLP training step, each from the INPUTS THE LIBRARY ITSELF KEPT (vnrAmdNeuralVolumeTrainingBuffer
0 - 3 and 5 - 7), with a derived worst-case distance per element (DESIGN.md 4.3 "the chain").  Because a stage's inputs are the stored
buffers, the discontinuities of the function are gone: the ReLU mask is read from the stored activation, the L1 sign from the stored output.
What remains is exact products of halves summed in fp32 in an order nobody states and rounded to half once:

    |stored - S|  <=  ulp16(S) + terms * u * A          S = the float64 sum, A = the sum of |terms|, u = 2^-23

u is TWICE the round-to-nearest unit of fp32: the fp32 MFMA is documented as a round-to-nearest fma chain, the f16-input one's internal
rounding is not, so the bound also holds for truncation.  ulp16 is a whole ulp (not a half): the fp32 sum may sit on the other side of a
rounding boundary.  Every number below is derived, none is measured.  A helper module of tests/test_mlp_stage_ref_host.py (which proves that
the checker accepts every legal order of the sums and rejects single lost terms) and tests/test_gpu_mlp_stages.py, not a test file."""
import collections
import math

import numpy as np

from oracle import train_oracle as T

U = 2.0 ** -23
ACT = {"None": 0, "ReLU": 1, "Exponential": 2, "Sigmoid": 3, "Squareplus": 4, "Softplus": 5}
TRANSCENDENTAL = (2, 3, 4, 5)          # evaluated in fp32 on the half (__expf, a division) and rounded back: one more ulp16 of the result
INEXACT_FACTOR = (4, 5)                # activation-backward factors whose own fp32 evaluation is not exact (a division, __expf)
WG_BLOCK = 256                         # samples per block partial of the weight gradients (network_train.hip kWgStage * kWgStages)

Stage = collections.namedtuple("Stage", "want S A bound")


def code(a):
    return ACT.get(a, a)


def f64(x):
    return np.asarray(x, dtype=np.float64)


def f32(x):
    return np.asarray(x).astype(np.float32)


def ulp16_by_definition(x):
    """the distance from fp16(|x|) to the next half above it (tests/test_gpu_deterministic_training.py): 2^-24 at zero, nan beyond the halves"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float16)).astype(np.float64)


def ulp16(x):
    """ulp16_by_definition without the (slow) conversions to half: 2^(e - 11) for 2^(e-1) <= |x| < 2^e, one binade up where |x| rounds to 2^e,
    never below 2^-24 (tests/test_mlp_stage_ref_host.py holds the two equal)"""
    a = np.abs(np.asarray(x, np.float64))
    m, e = np.frexp(a)
    e = e + (m >= 1.0 - 2.0 ** -12)          # |x| at or above the midpoint below 2^e rounds up to it (ties to even: 2^e is the even one)
    out = np.where(a == 0, 2.0 ** -24, np.ldexp(1.0, np.maximum(e - 11, -24)))
    return np.where(a >= 65520.0, np.nan, np.where(a > 65488.0, np.inf, out))          # (the largest half has no neighbour above; beyond it: no half)


def act64(x, a):
    a = code(a)
    with np.errstate(over="ignore", invalid="ignore"):
        if a == 0: return x
        if a == 1: return np.maximum(x, 0.0)
        if a == 2: return np.exp(x)
        if a == 3: return 1.0 / (1.0 + np.exp(-x))
        if a == 4: t = 10.0 * x; return 0.5 * (t + np.sqrt(t * t + 4.0)) / 10.0
        if a == 5: return np.logaddexp(0.0, 10.0 * x) / 10.0
    raise ValueError(a)


def lipschitz(S, a):
    """what a distance in front of the activation becomes behind it: 1 for None, ReLU, Squareplus, Softplus (slopes within [0, 1]), 1/4 for
    Sigmoid, the value itself for Exponential"""
    a = code(a)
    if a == 3: return 0.25
    if a == 2: return np.abs(act64(S, a))
    return 1.0


def through_activation(S, A, terms, a):
    """stored = act(fp16(fp32 sum of `terms` exact products)): Lip (ulp16(S) + terms u A) + ulp16(act(S)) (+ one more for the transcendental ones)"""
    a = code(a)
    y = act64(S, a)
    b = lipschitz(S, a) * (ulp16(S) + terms * U * A) + ulp16(y)
    if a in TRANSCENDENTAL:
        b = b + ulp16(y)
    return Stage(y, S, A, b)


# ------------------------------------------------------------------------------------------------ forward
def forward_hidden(x, w, act):
    """buffer 3, one layer: x [n][K] halves (buffer 2, or the previous layer's slice of buffer 3), w [W][K] -> [n][W]"""
    x, w = f64(x), f64(w)
    return through_activation(x @ w.T, np.abs(x) @ np.abs(w).T, x.shape[1], act)


def output(a_last, wl0, out_act):
    """buffer 7: the last slice of buffer 3 [n][W] against row 0 of the last layer [W]: a v_dot2 chain per lane half and one add"""
    a, w = f64(a_last), f64(wl0)
    return through_activation(a @ w, np.abs(a) @ np.abs(w), a.shape[1] + 1, out_act)


# ------------------------------------------------------------------------------------------------ loss
def loss_and_dy(y, targets, loss, out_act):
    """buffer 6 and the loss value from buffer 7 and the targets: every operation is a single fp32 or fp16 rounding of exact operands, restated
    as such.  -> dict(dy (halves), ulps (0: bit-exact; 1: Squareplus / Softplus), loss (float64), loss_rel)"""
    y, t = f32(y), f32(targets)
    n = y.shape[0]
    inv_n = np.float32(1.0) / np.float32(n)
    d = y - t
    if loss == "L1":
        g = np.copysign(np.float32(1.0), d)          # + at y == t, as copysignf(1, +0) gives
    else:
        g = np.float32(2.0) * d
    raw = T.f16((np.float32(T.LOSS_SCALE) * g) * inv_n)
    dy = T.f16(T.act_backward(raw.astype(np.float32), T.f16(y).astype(np.float32), code(out_act)))
    d64 = f64(y) - f64(t)
    value = float(np.abs(d64).mean() if loss == "L1" else (d64 * d64).mean())
    blocks = min(-(-n // 256), 1024)
    rel = (math.ceil(n / (256 * blocks)) + 8 + blocks) * 2.0 ** -24          # the strided loop, the tree, the sum of the partials
    return {"dy": dy, "ulps": 1 if code(out_act) in INEXACT_FACTOR else 0, "loss": value, "loss_rel": rel}


# ------------------------------------------------------------------------------------------------ backward
def backward_last(dy, wl0, a_nh, act):
    """slice nh of buffer 5: fp16(w dy) (the product of two halves is exact in fp32: one rounding), through the activation's backward from the
    stored activation.  -> (halves, ulps: 0 bit-exact, 2 for Squareplus / Softplus)"""
    d = T.f16(f32(wl0)[None, :] * f32(dy)[:, None]).astype(np.float32)
    return T.f16(T.act_backward(d, f32(a_nh), code(act))), (2 if code(act) in INEXACT_FACTOR else 0)


def activation_factor(a, act):
    """the factor act_backward_f16 multiplies the gradient by, from the stored activation, as a half (None: 1, ReLU: the mask)"""
    if code(act) <= 1:
        return np.ones(np.shape(a)) if code(act) == 0 else (f64(a) > 0).astype(np.float64)
    return f64(T.f16(T.act_backward(np.ones(np.shape(a), np.float32), f32(a), code(act))))


def backward_hidden(d_above, wmat, a_below, act):
    """slices nh-1 .. 0 of buffer 5 (a_below = the layer's stored activation) and buffer 1 (a_below = None: no activation in front of the
    features): S[b][j] = sum_k W[k][j] d[b][k], stored = fp16(fp16(S) factor)"""
    d, w = f64(d_above), f64(wmat)
    S, A = d @ w, np.abs(d) @ np.abs(w)
    f = 1.0 if a_below is None else activation_factor(a_below, act)
    want = S * f
    b = np.abs(f) * (ulp16(S) + w.shape[0] * U * A) + ulp16(want)
    if a_below is not None and code(act) in INEXACT_FACTOR:
        b = b + ulp16(want)
    return Stage(want, S, A, b)


def wg_terms(n):
    """roundings of one weight-gradient element: 256 samples into a block's accumulator, ceil(nblk / 4) partials per chain of the reduce, 3 adds"""
    nblk = -(-n // WG_BLOCK)
    return WG_BLOCK + -(-nblk // 4) + 3


def weight_gradient(d, x, first=None):
    """one matrix of the MLP part of buffer 0: S[out][in] = sum_b d[b][out] x[b][in]; first: what the blob held before this call (a second
    ForwardBackward before TrainEnd adds: fp16(float(first) + S))"""
    d, x = f64(d), f64(x)
    S, A = d.T @ x, np.abs(d).T @ np.abs(x)
    want = S if first is None else f64(first) + S
    return Stage(want, S, A, ulp16(want) + wg_terms(d.shape[0]) * U * A)


# ------------------------------------------------------------------------------------------------ the chain
Report = collections.namedtuple("Report", "failures ratios stats")


def _miss(failures, ratios, name, got, st):
    err = np.abs(f64(got) - st.want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratios[name] = max(ratios.get(name, 0.0), float(np.max(err / st.bound)) if err.size else 0.0)
    bad = np.argwhere(~(err <= st.bound))
    if bad.size:
        i = tuple(bad[0])
        failures.append((name, len(bad), [tuple(int(q) for q in b) for b in bad[:4]], float(f64(got)[i]), float(st.want[i]), float(st.bound[i]),
                         float(st.A[i])))


def _miss_ulps(failures, ratios, name, got, want, ulps):
    got, want = f64(got), f64(want)
    err = np.abs(got - want)
    bad = np.argwhere(~(err <= ulps * np.maximum(ulp16(want), ulp16(got))))
    ratios[name] = max(ratios.get(name, 0.0), float(np.max(err / ulp16(want))) if err.size else 0.0)    # (in ulps: 0 is bit-exact)
    if bad.size:
        i = tuple(bad[0])
        failures.append((name, len(bad), [tuple(int(q) for q in b) for b in bad[:4]], float(got[i]), float(want[i]), ulps))


def _shares(st):
    """(share of elements whose exact value is zero, share of the non-zero ones the bound holds to 2^-6 of their value)"""
    nz = st.want != 0
    zero = 1.0 - float(nz.mean())
    sharp = float((st.bound[nz] <= 2.0 ** -6 * np.abs(st.want[nz])).mean()) if nz.any() else 0.0
    return zero, sharp


def run_chain(bufs, mlp_params, shape, targets, first_blob=None):
    """every link of the chain on one ForwardBackward.  bufs: features [n][in_w], acts [nh+1][n][W], y [n] fp32, dy [n], d_all [nh+1][n][W],
    dfeat [n][in_w], grads [n_mlp] (halves unless said), loss (float).  shape: dict(W, in_w, H, LF (the real feature columns), act, out_act,
    loss).  -> Report(failures, ratios: largest error / bound per stage (in ulps for the bit-exact stages), stats: non-vacuity shares)"""
    W, in_w, nh, LF = shape["W"], shape["in_w"], shape["H"] - 1, shape["LF"]
    act, out_act = code(shape["act"]), code(shape["out_act"])
    w1, wh, wl, n_mlp = T.split_mlp(mlp_params, in_w, W, nh)
    feat, acts, d_all = f64(bufs["features"]), f64(bufs["acts"]), f64(bufs["d_all"])          # (halves convert slowly: once)
    n = feat.shape[0]
    failures, ratios, stats = [], {}, {"zero": {}, "sharp": {}, "backward_sharp": {}}
    # forward
    x = feat
    for l in range(nh + 1):
        _miss(failures, ratios, "forward", acts[l], forward_hidden(x, w1 if l == 0 else wh[l - 1], act))
        x = acts[l]
    _miss(failures, ratios, "output", bufs["y"], output(acts[nh], wl[0], out_act))
    # loss
    ld = loss_and_dy(bufs["y"], targets, shape["loss"], out_act)
    _miss_ulps(failures, ratios, "dy", bufs["dy"], ld["dy"], ld["ulps"])
    ratios["loss"] = abs(bufs["loss"] - ld["loss"]) / (ld["loss_rel"] * ld["loss"]) if ld["loss"] > 0 else float(bufs["loss"] != 0)
    if not ratios["loss"] <= 1.0:
        failures.append(("loss", 1, [], float(bufs["loss"]), ld["loss"], ld["loss_rel"] * ld["loss"]))
    # backward
    want, ulps = backward_last(bufs["dy"], wl[0], acts[nh], act)
    _miss_ulps(failures, ratios, "backward last", d_all[nh], want, ulps)
    for l in range(nh - 1, -1, -1):
        st = backward_hidden(d_all[l + 1], wh[l], acts[l], act)
        _miss(failures, ratios, "backward hidden", d_all[l], st)
        stats["backward_sharp"]["hidden %d" % l] = _shares(st)[1]
    st = backward_hidden(d_all[0], w1, None, act)
    _miss(failures, ratios, "dfeat", bufs["dfeat"], st)
    stats["backward_sharp"]["dfeat"] = _shares(Stage(st.want[:, :LF], st.S[:, :LF], st.A[:, :LF], st.bound[:, :LF]))[1]
    # weight gradients
    g = np.asarray(bufs["grads"])[:n_mlp]
    fb = None if first_blob is None else np.asarray(first_blob)[:n_mlp]
    off = 0
    mats = [("matrix 0", d_all[0], feat, W * in_w, (W, in_w))]
    mats += [("matrix %d" % (l + 1), d_all[l + 1], acts[l], W * W, (W, W)) for l in range(nh)]
    mats += [("last row", f64(bufs["dy"]).reshape(n, 1), acts[nh], W, (1, W))]
    for name, d, xin, size, shp in mats:
        st = weight_gradient(d, xin, None if fb is None else fb[off:off + size].reshape(shp))
        _miss(failures, ratios, "weight gradients", g[off:off + size].reshape(shp), st)
        real = Stage(st.S[:, :LF], st.S[:, :LF], st.A[:, :LF], (ulp16(st.S) + wg_terms(n) * U * st.A)[:, :LF]) if name == "matrix 0" else \
            Stage(st.S, st.S, st.A, ulp16(st.S) + wg_terms(n) * U * st.A)
        stats["zero"][name], stats["sharp"][name] = _shares(real)
        if name == "matrix 0" and LF < in_w and f64(g[off:off + size].reshape(shp)[:, LF:]).any():
            failures.append(("padded feature columns", int(np.count_nonzero(f64(g[off:off + size].reshape(shp)[:, LF:]))), [], 0, 0, 0))
        off += size
    assert off + 15 * W == n_mlp == g.size
    if f64(g[off:]).any():
        failures.append(("padded rows of the last layer", int(np.count_nonzero(f64(g[off:]))), [], 0, 0, 0))
    return Report(failures, ratios, stats)


def vacuous(report, n):
    """the conditions under which the chain says something: in every matrix at most 1/10 of the real elements are exactly zero, the bound
    holds at least 9/10 (n <= 1025) or 2/3 (larger batches: the fp32 term grows with the sum of |terms|) of the others to 2^-6 of their
    value, and 9/10 in every backward stage.  -> list of the conditions missed"""
    out = []
    for name, z in report.stats["zero"].items():
        if not z <= 0.1: out.append(("zero share", name, z))
    for name, s in report.stats["sharp"].items():
        if not s >= (0.9 if n <= 1025 else 2.0 / 3.0): out.append(("sharp share", name, s))
    for name, s in report.stats["backward_sharp"].items():
        if not s >= 0.9: out.append(("sharp share", name, s))
    return out


# ------------------------------------------------------------------------------------------------ the library's buffers
def download(vol, n, shape, n_mlp):
    """buffers 0 - 3 and 5 - 7 and the loss, shaped for run_chain"""
    from instantvnr_amd import api
    training_buffer = api.neural_training_buffer
    W, in_w, nh = shape["W"], shape["in_w"], shape["H"] - 1
    return {"grads": training_buffer(vol, 0, np.float16)[:n_mlp],
            "dfeat": training_buffer(vol, 1, np.float16).reshape(n, in_w),
            "features": training_buffer(vol, 2, np.float16).reshape(n, in_w),
            "acts": training_buffer(vol, 3, np.float16).reshape(nh + 1, n, W),
            "d_all": training_buffer(vol, 5, np.float16).reshape(nh + 1, n, W),
            "dy": training_buffer(vol, 6, np.float16).reshape(n),
            "y": training_buffer(vol, 7, np.float32).reshape(n),
            "loss": float(api.vnrNeuralVolumeGetTrainingLoss(vol))}


# ------------------------------------------------------------------------------------------------ the cases (shared by the host and the GPU test)
# in_width -> (levels, features per level): L F zero-padded to a multiple of 16; some padded, some not
ENCODINGS = {16: [(5, 2), (4, 4), (8, 2), (4, 2)], 32: [(3, 8), (16, 2), (8, 4)], 48: [(6, 8), (5, 8)], 64: [(7, 8), (16, 4)], 80: [(10, 8)], 96: [(12, 8)],
             112: [(13, 8)], 128: [(16, 8), (15, 8)]}
GROWING = ("Exponential", "Softplus")


def case(name, W, in_w, H, n, enc=0, act="ReLU", out_act="None", loss="L1", seed=1):
    L, F = ENCODINGS[in_w][enc]
    assert (L * F + 15) // 16 * 16 == in_w
    grows = act in GROWING or out_act == "Exponential"
    return dict(name=name, W=W, in_w=in_w, H=H, n=n, L=L, F=F, LF=L * F, act=act, out_act=out_act, loss=loss, seed=seed,
                log2T=8 + seed % 3, base=2 + seed % 3, pls=(1.2, 1.3, 1.5)[seed % 3], mlp_scale=(0.35 if grows else 1.0) * (0.7 if H > 3 else 1.0))


# width x input tiling: MTF 1 - 4 with and without a ragged last half-tile, weight-gradient NT 1 / 2 / 4 with xc below and at the tile,
# T in {1, 2, 4, 8, 16} (both WPT > 1 hand-overs, TW > 1), nh = 0 (the second launch holds only the last layer)
TILING = [(16, 16, 2, 0), (16, 48, 1, 0), (16, 128, 3, 0), (32, 16, 1, 1), (32, 32, 2, 0), (32, 48, 3, 1), (32, 96, 2, 0), (64, 16, 2, 2), (64, 32, 3, 1),
          (64, 64, 1, 0), (64, 80, 2, 0), (64, 128, 4, 1), (128, 32, 2, 2), (128, 64, 3, 1), (128, 112, 2, 0), (128, 128, 4, 0)]
BATCH_EDGES = [1, 31, 63, 64, 65, 255, 256, 257, 1025]
N_FROM_CUS = -1      # n = 64 * 4 * (the device's CU count) + 37: one tile more than one trip of the backward kernel's grid, and ragged


def cases():
    out = [case("W%d in%d H%d" % (W, i, H), W, i, H, 1000, enc, seed=3 + k) for k, (W, i, H, enc) in enumerate(TILING)]
    for W, i, enc in ((64, 32, 1), (16, 16, 0)):
        # (one sample through ReLU masks three quarters of every hidden matrix whatever the seed: the single-sample row runs without activation,
        # on the same kernel instances, so that its matrices say something)
        out += [case("W%d n%d" % (W, n), W, i, 2, n, enc, act="None" if n == 1 else "ReLU", seed=20 + k if W == 64 else 62) for k, n in enumerate(BATCH_EDGES)]
    out.append(case("reduce: 67 block partials", 64, 32, 2, 256 * 67 + 5, 1, seed=30))
    out.append(case("backward grid-stride trip", 128, 32, 4, N_FROM_CUS, 1, seed=31))
    out.append(case("weights from global memory", 128, 32, 7, 257, 1, seed=382))
    for k, a in enumerate(["Sigmoid", "Squareplus", "Softplus", "Exponential", "None"]):
        out += [case("%s W%d" % (a, W), W, 32, 2, 320, 0, act=a, seed=40 + 2 * k + (W == 64)) for W in (32, 64)]
    out += [case("output %s" % a, 64, 32, 2, 320, 1, out_act=a, seed=50 + k) for k, a in enumerate(["ReLU", "Sigmoid", "Exponential"])]
    out.append(case("L2 W32 in32", 32, 32, 2, 1000, 0, loss="L2", seed=62))
    out.append(case("L2 W64 in80", 64, 80, 2, 1000, 0, loss="L2", seed=61))
    return out


def extra_cases():
    """the models of the GPU test's sequences: two calls before one optimizer step; 64 x 1 and then 32 x 2 on the same volume (the same 2 048 MLP
    parameters in another layout); a batch of 1025 and then one of 63"""
    return {"accumulation": case("accumulation", 64, 32, 2, 1000, 1, seed=70),
            "reconfiguration a": case("reconfiguration: W64 x 1", 64, 16, 1, 1000, 3, seed=71),
            "reconfiguration b": case("reconfiguration: W32 x 2", 32, 16, 2, 1000, 3, seed=72),
            "shrink": case("batch shrinks", 64, 32, 2, 1025, 1, seed=73)}


def batch_size(c, n_cus):
    return 64 * 4 * n_cus + 37 if c["n"] == N_FROM_CUS else c["n"]


FACES = [(0, 0, 0), (1, 1, 1), (1, 0, 0.5), (0.999999, 0.999999, 0.999999), (0.5, 1, 1), (1, 1, 0), (0, 1, 0.25), (1e-7, 0.5, 1)]


def batch(c, n, seed_offset=0):
    """uniform coordinates with the faces and corners of the domain in front, and targets (uniform, as the model sweep draws them)"""
    rng = np.random.default_rng(1000 + c["seed"] + seed_offset)
    coords = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    k = min(n, len(FACES))
    coords[:k] = np.array(FACES, np.float32)[:k]
    return coords, rng.uniform(0, 1, n).astype(np.float32)
