"""The chain of per-element checks of the MLP training step (tests/mlp_stage_ref.py) is sharp and not vacuous, shown without
the library: a numpy emulation of every stage that rounds where the kernels round -- exact products of halves, summed in fp32 in a shuffled
order in chunks of 16 (one MFMA k-step), cast to half once; the weight gradients in blocks of 256 samples whose partials the reduce sums in
four interleaved chains -- is accepted in every order drawn at every case the GPU test runs, every mutation of it that models a kernel bug
(a lost sample, a lost k-step, a ragged tail, a block counted twice, a mask or a sign taken from the wrong place) is rejected, and the bounds
hold almost every element to 2^-6 of its value."""
import os
import sys

import numpy as np
import pytest

from instantvnr_amd import synthetic as syn
from oracle import train_oracle as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_stage_ref as R  # noqa: E402

CASES = R.cases()
ALL = CASES + list(R.extra_cases().values())
N_CUS = 32           # a stand-in for the device's count, which the GPU test reads: the case's shape at a batch the scalar oracle forwards quickly


# ------------------------------------------------------------------------------------------------ the emulation
def emu_mm(x, w, rng):
    """[n][K] halves x [M][K] halves -> fp32 [n][M]: k in a shuffled order, 16 at a time into an fp32 accumulator"""
    x, w = R.f32(x), R.f32(w)
    perm = rng.permutation(x.shape[1])
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for k0 in range(0, perm.size, 16):
        idx = perm[k0:k0 + 16]
        acc = acc + x[:, idx] @ w[:, idx].T
    return acc


def act32(h, a):
    """the activation on the half, evaluated in fp32 and rounded back (infer_tile.h act_forward_f16)"""
    a = R.code(a)
    v = h.astype(np.float32)
    with np.errstate(over="ignore"):
        if a == 0: return h
        if a == 1: return np.maximum(h, np.float16(0))
        if a == 2: return T.f16(np.exp(v))
        if a == 3: return T.f16(np.float32(1) / (np.float32(1) + np.exp(-v)))
        if a == 4: t = v * np.float32(10); return T.f16(np.float32(0.5) * (t + np.sqrt(t * t + np.float32(4))) / np.float32(10))
        if a == 5: return T.f16(np.log(np.exp(v * np.float32(10)) + np.float32(1)) / np.float32(10))
    raise ValueError(a)


def block_partials(d, x, rng):
    """[nblk][out][in] fp32: a block's 256 samples in a shuffled order, 16 at a time (absent samples of a ragged last block are zeros)"""
    d, x = R.f32(d), R.f32(x)
    n, B = d.shape[0], R.WG_BLOCK
    nblk = -(-n // B)
    dp, xp = np.zeros((nblk * B, d.shape[1]), np.float32), np.zeros((nblk * B, x.shape[1]), np.float32)
    dp[:n], xp[:n] = d, x
    perm = (np.arange(nblk)[:, None] * B + np.stack([rng.permutation(B) for _ in range(nblk)])).ravel()
    dp, xp = dp[perm].reshape(nblk, B // 16, 16, -1), xp[perm].reshape(nblk, B // 16, 16, -1)
    out = np.zeros((nblk, d.shape[1], x.shape[1]), np.float32)
    for b0 in range(0, nblk, 16):
        steps = np.matmul(dp[b0:b0 + 16].transpose(0, 1, 3, 2), xp[b0:b0 + 16])          # [blocks][k-steps][out][in]
        for k in range(B // 16):
            out[b0:b0 + 16] = out[b0:b0 + 16] + steps[:, k]
    return out


def reduce_partials(parts, first=None, twice=None):
    """weight_grad_reduce_kernel: chain g sums blocks g, g + 4, ...; (c0 + c1) + (c2 + c3); one rounding to half on top of what the blob held.
    twice: a block counted a second time (a mutation)"""
    chains = [np.zeros(parts.shape[1:], np.float32) for _ in range(4)]
    for b in range(parts.shape[0]):
        chains[b % 4] = chains[b % 4] + parts[b]
        if twice == b:
            chains[b % 4] = chains[b % 4] + parts[b]
    total = (chains[0] + chains[1]) + (chains[2] + chains[3])
    return T.f16((np.float32(0) if first is None else R.f32(first)) + total)


def matrices(bufs, nh):
    """(d, x) of every matrix in the blob's order: first layer, hidden layers, row 0 of the last"""
    n = bufs["features"].shape[0]
    return [(bufs["d_all"][0], bufs["features"])] + [(bufs["d_all"][l + 1], bufs["acts"][l]) for l in range(nh)] + \
        [(np.asarray(bufs["dy"]).reshape(n, 1), bufs["acts"][nh])]


def assemble(rows, W):
    """the MLP part of the blob from its matrices: rows 1 .. 15 of the padded last layer are zero"""
    return np.concatenate([np.asarray(m, np.float16).ravel() for m in rows] + [np.zeros(15 * W, np.float16)])


def emulate(c, mlp, feat, targets, rng, forward=None, first_blob=None):
    """every buffer of one ForwardBackward.  forward = (acts, y): the forward stages from elsewhere (the oracle's fp32 sums in k order)"""
    W, in_w, nh = c["W"], c["in_w"], c["H"] - 1
    w1, wh, wl, n_mlp = T.split_mlp(mlp, in_w, W, nh)
    n = feat.shape[0]
    if forward is None:
        acts, x = np.zeros((nh + 1, n, W), np.float16), feat
        for l in range(nh + 1):
            acts[l] = act32(T.f16(emu_mm(x, w1 if l == 0 else wh[l - 1], rng)), c["act"])
            x = acts[l]
        y = act32(T.f16(emu_mm(acts[nh], wl[:1], rng)[:, 0]), c["out_act"]).astype(np.float32)
    else:
        acts, y = forward
    ld = R.loss_and_dy(y, targets, c["loss"], c["out_act"])
    d = y - targets
    terms = (np.abs(d) if c["loss"] == "L1" else d * d) * (np.float32(1) / np.float32(n))
    d_all = np.zeros((nh + 1, n, W), np.float16)
    d_all[nh] = R.backward_last(ld["dy"], wl[0], acts[nh], c["act"])[0]
    for l in range(nh - 1, -1, -1):
        h = T.f16(emu_mm(d_all[l + 1], wh[l].T, rng)).astype(np.float32)
        d_all[l] = T.f16(T.act_backward(h, acts[l].astype(np.float32), R.code(c["act"])))
    bufs = {"features": feat, "acts": acts, "y": y, "dy": ld["dy"], "d_all": d_all, "dfeat": T.f16(emu_mm(d_all[0], w1.T, rng)),
            "loss": float(terms.astype(np.float32).sum(dtype=np.float32))}
    off, rows = 0, []
    for dm, xm in matrices(bufs, nh):
        size = dm.shape[1] * xm.shape[1]
        first = None if first_blob is None else first_blob[off:off + size].reshape(dm.shape[1], xm.shape[1])
        rows.append(reduce_partials(block_partials(dm, xm, rng), first))
        off += size
    bufs["grads"] = assemble(rows, W)
    assert bufs["grads"].size == n_mlp
    return bufs


_inputs = {}


def inputs(oracle, c):
    """parameters, batch, the oracle's encode and forward of a case: computed once, shared, never changed"""
    if c["name"] not in _inputs:
        n = R.batch_size(c, N_CUS)
        ocfg = oracle.grid_config(c["L"], c["F"], c["log2T"], c["base"], c["pls"])
        n_mlp = oracle.mlp_n_params(c["in_w"], c["W"], c["H"] - 1)
        params = syn.random_params(oracle.n_params(ocfg, c["W"], c["H"]), n_mlp, seed=c["seed"], mlp_scale=c["mlp_scale"])
        coords, targets = R.batch(c, n)
        feat = oracle.grid_encode(ocfg, params[n_mlp:].view(np.uint16), coords)
        y, acts = oracle.mlp_forward(params[:n_mlp].view(np.uint16), c["in_w"], c["W"], c["H"] - 1, feat,
                                     activation=oracle.act_code(c["act"], c["out_act"]), want_activations=True)
        for a in (feat, y, acts, params, targets):
            a.flags.writeable = False
        _inputs[c["name"]] = (params[:n_mlp], feat.view(np.float16), targets, (acts.view(np.float16), y), n)
    return _inputs[c["name"]]


# ------------------------------------------------------------------------------------------------ accepted, and not vacuous
@pytest.mark.parametrize("c", ALL, ids=[c["name"] for c in ALL])
def test_every_order_of_the_sums_is_accepted_and_the_bounds_say_something(oracle, c):
    mlp, feat, targets, forward, n = inputs(oracle, c)
    # the oracle's forward (fp32 sums in k order, tcnn's own roundings) with the emulated backward: its activations stand in for the library's
    rep = R.run_chain(emulate(c, mlp, feat, targets, np.random.default_rng(0), forward=forward), mlp, c, targets)
    assert not rep.failures, rep.failures
    assert not R.vacuous(rep, n), (R.vacuous(rep, n), rep.stats)
    for order in (1, 2, 3):
        rep = R.run_chain(emulate(c, mlp, feat, targets, np.random.default_rng(order)), mlp, c, targets)
        assert not rep.failures, (order, rep.failures)
        assert not R.vacuous(rep, n), (order, R.vacuous(rep, n))


def test_a_second_call_before_the_step_is_accepted_on_top_of_the_first(oracle):
    c = CASES[8]
    mlp, feat, targets, forward, n = inputs(oracle, c)
    first = emulate(c, mlp, feat, targets, np.random.default_rng(1))
    second = emulate(c, mlp, feat, targets, np.random.default_rng(2), first_blob=first["grads"])
    assert not R.run_chain(second, mlp, c, targets, first_blob=first["grads"]).failures
    assert any(f[0] == "weight gradients" for f in R.run_chain(second, mlp, c, targets).failures), "twice the gradient is not one call's"
    lost = dict(second, grads=first["grads"])                      # the second call's sums never arrived
    assert any(f[0] == "weight gradients" for f in R.run_chain(lost, mlp, c, targets, first_blob=first["grads"]).failures)


# ------------------------------------------------------------------------------------------------ mutations
MUTATED = [CASES[i] for i in (0, 4, 8, 10, 13)] + [c for c in CASES if c["name"] in ("W64 n257", "reduce: 67 block partials")]


def stages_missed(bufs, mlp, c, targets):
    return {f[0] for f in R.run_chain(bufs, mlp, c, targets).failures}


def replace_matrix(bufs, c, which, new):
    """the blob with matrix `which` (0: first layer, ..., nh + 1: the last row) replaced"""
    W, in_w, nh = c["W"], c["in_w"], c["H"] - 1
    sizes = [W * in_w] + [W * W] * nh + [W]
    off = sum(sizes[:which])
    g = np.array(bufs["grads"])
    g[off:off + sizes[which]] = np.asarray(new, np.float16).ravel()
    return dict(bufs, grads=g)


@pytest.mark.parametrize("c", MUTATED, ids=[c["name"] for c in MUTATED])
def test_every_mutation_of_the_weight_gradients_is_rejected(oracle, c):
    mlp, feat, targets, forward, n = inputs(oracle, c)
    rng = np.random.default_rng(7)
    bufs = emulate(c, mlp, feat, targets, rng)
    assert not stages_missed(bufs, mlp, c, targets)
    for which, (d, x) in enumerate(matrices(bufs, c["H"] - 1)):
        d32, x32 = R.f32(d), R.f32(x)
        parts = block_partials(d, x, rng)
        st = R.weight_gradient(d, x)
        rejected = lambda m: bool((np.abs(R.f64(m) - st.want) > st.bound).any())          # noqa: E731  (what run_chain asks of this matrix)
        assert not rejected(reduce_partials(parts))
        # one sample's term removed from one element: a sample and element with a large |term|
        b, o = np.unravel_index(int(np.argmax(np.abs(d32) * np.abs(x32).max(axis=1, keepdims=True))), d32.shape)
        i = int(np.argmax(np.abs(x32[b])))
        p = parts.copy()
        p[b // R.WG_BLOCK, o, i] -= d32[b, o] * x32[b, i]
        assert rejected(reduce_partials(p)), ("one term", which)
        # the last n mod 64 samples removed
        if n % 64:
            d_cut = d32.copy()
            d_cut[n - n % 64:] = 0
            assert rejected(reduce_partials(block_partials(d_cut, x, rng))), ("ragged tail", which)
        # one 16-sample k-step removed from one 32 x 32 tile
        if n >= 16:
            s0 = 16 * int(rng.integers(0, n // 16))
            p = parts.copy()
            p[s0 // R.WG_BLOCK, :32, :32] -= (d32[s0:s0 + 16].T @ x32[s0:s0 + 16])[:32, :32]
            assert rejected(reduce_partials(p)), ("k-step", which, s0)
        # one block partial counted twice
        assert rejected(reduce_partials(parts, twice=parts.shape[0] - 1)), ("twice", which)
        # the element the bound holds tightest, off by 3 fp16 ulps
        with np.errstate(divide="ignore", invalid="ignore"):
            o, i = np.unravel_index(int(np.argmax(np.where(st.S != 0, np.abs(st.S) / st.bound, 0))), st.S.shape)
        m = reduce_partials(parts)
        m[o, i] = m[o, i] + np.float16(3 * R.ulp16(m[o, i]))
        assert rejected(m), ("3 ulps", which)
        assert "weight gradients" in stages_missed(replace_matrix(bufs, c, which, m), mlp, c, targets), ("3 ulps in the chain", which)
    # a padded feature column, and a padded row of the last layer, with the smallest non-zero value
    if c["LF"] < c["in_w"]:
        g = np.array(bufs["grads"])
        g[c["in_w"] - 1] = np.float16(2.0 ** -24)
        assert "padded feature columns" in stages_missed(dict(bufs, grads=g), mlp, c, targets)
    g = np.array(bufs["grads"])
    g[-1] = np.float16(2.0 ** -24)
    assert "padded rows of the last layer" in stages_missed(dict(bufs, grads=g), mlp, c, targets)


def off_by_3_ulps(a, where):
    a = np.array(a)
    step = 3 * R.ulp16(a[where])
    a[where] = (a[where].astype(np.float64) + step).astype(a.dtype)
    return a


@pytest.mark.parametrize("c", MUTATED[:-1], ids=[c["name"] for c in MUTATED[:-1]])
def test_every_mutation_of_the_forward_and_backward_stages_is_rejected(oracle, c):
    mlp, feat, targets, forward, n = inputs(oracle, c)
    rng = np.random.default_rng(11)
    bufs = emulate(c, mlp, feat, targets, rng)
    W, in_w, nh = c["W"], c["in_w"], c["H"] - 1
    w1, wh, wl, _ = T.split_mlp(mlp, in_w, W, nh)
    b = int(rng.integers(0, n))
    # one element of every stage's output off by 3 fp16 ulps, at an element the stage's bound holds tight
    for l in range(nh + 1):
        st = R.forward_hidden(feat if l == 0 else bufs["acts"][l - 1], w1 if l == 0 else wh[l - 1], c["act"])
        j = int(np.argmax(np.abs(st.want[b]) / st.bound[b]))
        assert "forward" in stages_missed(dict(bufs, acts=off_by_3_ulps(bufs["acts"], (l, b, j))), mlp, c, targets), l
    assert "output" in stages_missed(dict(bufs, y=off_by_3_ulps(bufs["y"].astype(np.float16), b).astype(np.float32)), mlp, c, targets)
    assert "dy" in stages_missed(dict(bufs, dy=off_by_3_ulps(bufs["dy"], b)), mlp, c, targets)
    for l in range(nh + 1):
        live = np.nonzero(bufs["d_all"][l][b])[0]
        if live.size:
            want = {"backward last"} if l == nh else {"backward hidden"}
            assert want <= stages_missed(dict(bufs, d_all=off_by_3_ulps(bufs["d_all"], (l, b, int(live[0])))), mlp, c, targets), l
    st = R.backward_hidden(bufs["d_all"][0], w1, None, c["act"])
    j = int(np.argmax(np.abs(st.want[b]) / st.bound[b]))
    assert "dfeat" in stages_missed(dict(bufs, dfeat=off_by_3_ulps(bufs["dfeat"], (b, j))), mlp, c, targets)
    # one L1 sign flipped / one L2 residual negated
    dy = np.array(bufs["dy"])
    live = np.nonzero(dy)[0]
    dy[live[0]] = -dy[live[0]]
    assert "dy" in stages_missed(dict(bufs, dy=dy), mlp, c, targets)
    # one 16-term k-step removed from one 32 x 32 tile of a backward product (32 samples x 32 columns of dL/dfeatures)
    d0 = R.f32(bufs["d_all"][0])
    lost = emu_mm(bufs["d_all"][0], w1.T, rng)
    lost[:32, :32] -= (d0[:32, :16] @ R.f32(w1)[:16, :32])
    assert "dfeat" in stages_missed(dict(bufs, dfeat=T.f16(lost)), mlp, c, targets)
    # the loss summed without its last sample
    y, t = bufs["y"], targets
    terms = np.abs(y - t) if c["loss"] == "L1" else (y - t) ** 2
    if n > 1 and terms[-1] > 0:
        assert "loss" in stages_missed(dict(bufs, loss=float(terms[:-1].sum() / n)), mlp, c, targets)


def test_a_relu_mask_taken_from_the_sum_instead_of_the_stored_activation_is_rejected():
    """a pre-activation whose fp32 sum is positive and rounds to a half of zero: the stored activation is 0, the backward's mask follows IT
    (tcnn reads the mask from the stored output); a kernel that kept the mask of its fp32 accumulator would pass the gradient through"""
    W, n = 16, 4
    x = np.zeros((n, W), np.float16); x[:, 0] = np.float16(2.0 ** -13)
    w = np.zeros((W, W), np.float16); w[:, 0] = np.float16(2.0 ** -13)
    pre = R.f32(x) @ R.f32(w).T                                # 2^-26 everywhere: positive, and zero as a half
    stored = np.maximum(T.f16(pre), np.float16(0))
    assert (pre > 0).all() and not stored.any()
    assert not (np.abs(R.f64(stored) - R.forward_hidden(x, w, "ReLU").want) > R.forward_hidden(x, w, "ReLU").bound).any()
    rng = np.random.default_rng(3)
    d_above = rng.uniform(-1, 1, (n, W)).astype(np.float16)
    wh = rng.uniform(-0.35, 0.35, (W, W)).astype(np.float16)
    st = R.backward_hidden(d_above, wh, stored, "ReLU")
    s16 = T.f16(R.f32(d_above) @ R.f32(wh))
    from_stored = np.where(stored > 0, s16, np.float16(0))
    from_sum = np.where(pre > 0, s16, np.float16(0))
    assert (np.abs(R.f64(from_stored) - st.want) <= st.bound).all()
    assert (np.abs(R.f64(from_sum) - st.want) > st.bound).any()


def test_the_fast_ulp16_is_the_definition():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.normal(size=200000) * 10.0 ** rng.uniform(-9, 5, 200000), [0.0, 2.0 ** -25, 2.0 ** -24, 2.0 ** -14, 1.0, 65504.0, 65519.9, 65520.0, 1e6],
                        np.ldexp(1.0 - 2.0 ** -12, np.arange(-26, 17)), np.ldexp(1.0 - 2.0 ** -12 - 2.0 ** -30, np.arange(-26, 17)),
                        np.ldexp(1.0 - 2.0 ** -13, np.arange(-26, 17)), np.ldexp(1.0, np.arange(-26, 17))])
    assert np.array_equal(R.ulp16(x), R.ulp16_by_definition(x), equal_nan=True)
