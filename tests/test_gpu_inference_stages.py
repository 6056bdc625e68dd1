"""The inference kernel (vnrAmdNeuralVolumeInference: fused_infer_kernel<F, K_IN, W, 0, GENERAL>) held LAYER BY LAYER to the per-element stage
bounds of the training step (DESIGN.md 4.3 "the chain", the inference side).  The kernel stores nothing but its output, so its hidden
activations are read out THROUGH the output (tests/infer_readout_ref.py: a unit row in the last layer, identity matrices behind the layer read;
W launches a layer, every value the kernel's own, bit for bit) and every stage is then checked from its own inputs with tests/mlp_stage_ref.py,
at the shapes where the kernels branch (R.cases()).  tests/test_infer_readout_host.py shows on the CPU that the readout is exact in every order
of the sums and that a single lost product, which the 2^-8 end-to-end bar of test_gpu_network.py accepts, is rejected.  On top of that: the
output equals the training forward's (the same template with MODE == 2) bit for bit, and a sample's value does not depend on the batch's size
or on where in it the sample sits, with nothing written behind the batch."""
import os
import sys

import numpy as np
import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn
from instantvnr_amd._lib import check, lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infer_readout_ref as IR  # noqa: E402
import mlp_stage_ref as R  # noqa: E402
from test_gpu_mlp_stages import device_cus, model_config  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = R.cases()
EXTRA = R.extra_cases()
TILED = CASES[:len(R.TILING)]
GLOBAL = [c for c in CASES if c["name"] == "weights from global memory"]
ACTIVATIONS = [c for c in CASES if c["name"].split()[0] in R.ACT or c["name"].startswith("output ")]
assert len(TILED) == 16 and len(GLOBAL) == 1 and len(ACTIVATIONS) == 13
SENTINEL = 0x7fa5a5a5          # a NaN whose low 13 bits are set: no half-valued output


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    monkeypatch.delenv("VNR_AMD_DETERMINISTIC", raising=False)
    monkeypatch.delenv("VNR_AMD_TRAIN_OVERLAP", raising=False)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Model:
    """a volume of the case's model with the case's seeded parameters"""

    def __init__(self, oracle, c, out_act=None, hidden_layers=None):
        cfg = model_config(dict(c, out_act=c["out_act"] if out_act is None else out_act, H=hidden_layers or c["H"]))
        self.c, self.vol = c, api.vnrCreateNeuralVolume(cfg, (32, 32, 32))
        info = api.neural_info(self.vol)
        assert info["padded_width"] == c["in_w"] and info["n_neurons"] == c["W"] and info["mfma_kernels"] == 1, info
        # (the blob of the case's own depth: a volume cut off behind an earlier layer shares its grid)
        n_mlp = oracle.mlp_n_params(c["in_w"], c["W"], c["H"] - 1)
        n_grid = info["n_params"] - oracle.mlp_n_params(c["in_w"], c["W"], (hidden_layers or c["H"]) - 1)
        params = syn.random_params(n_mlp + n_grid, n_mlp, seed=c["seed"], mlp_scale=c["mlp_scale"])
        self.mlp, self.grid = params[:n_mlp], params[n_mlp:]
        if hidden_layers is None:
            self.set_mlp(self.mlp)

    def set_mlp(self, mlp):
        api.neural_set_params_fp16(self.vol, np.concatenate([np.asarray(mlp, np.float16), self.grid]))

    def hashed(self):
        return any(lv["kind"] == 1 for lv in api.neural_level_table(self.vol))


class Launcher:
    """vnrAmdNeuralVolumeInference of one batch that stays on the device: evaluate(mlp part) is what tests/infer_readout_ref.py asks for"""

    def __init__(self, model, coords):
        self.model, self.n = model, coords.shape[0]
        self.coords = api.DeviceArray.from_numpy(np.ascontiguousarray(coords, np.float32))
        self.out = api.DeviceArray((self.n,), np.float32)

    def launch(self):
        check(lib().vnrAmdNeuralVolumeInference(self.model.vol.h, self.n, self.coords.ptr, self.out.ptr, None))
        check(lib().vnrAmdSynchronize())
        return self.out.numpy()

    def evaluate(self, mlp):
        self.model.set_mlp(mlp)
        return self.launch()


def inspect(oracle, c, n, layers=None):
    """read the layers out, evaluate the real weights, check every stage; -> (report, the model, its launcher, the readouts {layer: [n][W]})"""
    coords = R.batch(c, n)[0]
    model = Model(oracle, c)
    real = Launcher(model, coords)
    # the probes run with output activation None: on the model's own volume where that is its own, else on a second one with the same blob
    probes = real if R.code(c["out_act"]) == 0 else Launcher(Model(oracle, c, out_act="None"), coords)
    layers = IR.readable_layers(c) if layers is None else layers
    reads = dict(zip(layers, IR.readout(probes.evaluate, model.mlp, c, layers)))
    stand_in = None
    if layers[0] > 0 and layers[0] - 1 not in reads and R.code(c["act"]) not in IR.INVERTIBLE:
        # a transcendental activation hides the layer in front of the last: read it from the model cut off behind it (the same kernel, the
        # same first matrices and grid), as the last stage's input; the stages in front stay "not observable"
        cut_mlp, cc = IR.cut_model(model.mlp, c, layers[0] - 1)
        cut = Launcher(Model(oracle, c, out_act="None", hidden_layers=cc["H"]), coords)
        stand_in = IR.readout(cut.evaluate, cut_mlp, cc, [layers[0] - 1])[0]
    y = real.evaluate(model.mlp)
    rep = IR.check_inference(api.neural_encode(model.vol, coords), reads, y, model.mlp, c, stand_in=stand_in)
    line = IR.ratios_line(c["name"], n, rep)
    print(line)
    if os.environ.get("VNR_STAGE_LOG"):
        with open(os.environ["VNR_STAGE_LOG"], "a") as f:
            f.write("inference " + line + "\n")
    assert not rep.failures, (c["name"], rep.failures)
    assert not IR.vacuous(rep), (c["name"], IR.vacuous(rep), rep.stats)
    assert max(rep.ratios.values()) <= 1.0
    return rep, model, real, reads


# ------------------------------------------------------------------------------------------------ a. layer by layer
@pytest.mark.parametrize("c", TILED, ids=[c["name"] for c in TILED])
def test_every_layer_of_the_inference_kernel_is_its_inputs_exact_result_within_rounding(oracle, c):
    """every width x input tiling, every layer read out; and one probe once more from the de-hashed brick image.  Every probe changes the
    parameters, which drops the image (network.h), so the image is waited for here, with one probe's parameters left alone"""
    rep, model, real, reads = inspect(oracle, c, 1000)
    assert not rep.stats["not observable"] and len(rep.ratios) == c["H"] + 1
    # what was read out is what the training forward (the same template with MODE == 2) stores, value for value (the sign of a zero aside,
    # which the identity rows do not hand on): says in which layer the two kernels part, should the test of their outputs below ever fail
    coords, targets = R.batch(c, 1000)
    api.neural_forward_backward(model.vol, coords, targets)
    stored = api.neural_training_buffer(model.vol, 3, np.float16).reshape(c["H"], 1000, c["W"])
    api.neural_train_end(model.vol, grad_scale=0.0)
    for l, a in reads.items():
        assert not np.isnan(a).any() and np.array_equal(a, stored[l]), (c["name"], l, int((a != stored[l]).sum()))
    if model.hashed():
        assert not api.neural_brick_image(model.vol)["in_use"]
        y0 = real.evaluate(IR.probe_params(model.mlp, c, 0, c["W"] - 1))
        for _ in range(60):
            if api.neural_brick_image(model.vol)["in_use"]:
                break
            real.launch()
        assert api.neural_brick_image(model.vol)["in_use"]
        assert np.array_equal(bits(real.launch()), bits(y0))          # the same hidden unit, bit for bit, from the image


@pytest.mark.parametrize("c", GLOBAL, ids=[c["name"] for c in GLOBAL])
def test_layers_of_a_model_whose_weights_stay_in_global_memory(oracle, c):
    """128 neurons x 7 hidden layers: layers 0, 3 and 6 are held (and 2 and 5 read as the inputs of 3 and 6)"""
    rep, *_ = inspect(oracle, c, c["n"], layers=[0, 2, 3, 5, 6])
    assert sorted(rep.ratios) == ["layer 0", "layer 3", "layer 6", "output"]


@pytest.mark.parametrize("c", ACTIVATIONS, ids=[c["name"] for c in ACTIVATIONS])
def test_the_last_hidden_layer_and_the_output_under_every_activation(oracle, c):
    """None / ReLU: both layers are read.  Sigmoid, Squareplus, Softplus, Exponential: the last hidden layer and the output stage are held,
    layer 0 is said to be not observable"""
    rep, *_ = inspect(oracle, c, c["n"])
    nh = c["H"] - 1
    assert {"layer %d" % nh, "output"} <= set(rep.ratios)
    assert rep.stats["not observable"] == ([] if R.code(c["act"]) in IR.INVERTIBLE else ["layer %d" % l for l in range(nh)])


# ------------------------------------------------------------------------------------------------ b. inference is the training forward
EVERY = CASES + list(EXTRA.values())


@pytest.mark.parametrize("c", EVERY, ids=[c["name"] for c in EVERY])
def test_inference_equals_the_training_forward_bit_for_bit(oracle, c):
    """mlp_tile<..., TRAIN, ...> differs from the inference instance by store_acts alone, nothing may be re-associated (-ffp-contract=off) and
    finish_output is shared: buffer 7 of a ForwardBackward and vnrAmdNeuralVolumeInference of the same batch are the same bits"""
    model = Model(oracle, c)
    n = R.batch_size(c, device_cus() if c["n"] == R.N_FROM_CUS else 0)
    coords, targets = R.batch(c, n)
    api.neural_forward_backward(model.vol, coords, targets)
    trained = api.neural_training_buffer(model.vol, 7, np.float32).reshape(n)
    y = api.neural_inference(model.vol, coords)
    api.neural_train_end(model.vol, grad_scale=0.0)          # consumes and clears the gradients
    differ = np.nonzero(bits(y) != bits(trained))[0]
    assert differ.size == 0, (c["name"], differ.size, differ[:4], y[differ[:4]], trained[differ[:4]])
    assert IR.is_half(y).all()


# ------------------------------------------------------------------------------------------------ c. position in the batch
POSITION = [c for c in TILED if c["name"] in ("W64 in32 H3", "W128 in64 H3")]
BATCHES = [1, 63, 64, 65, 449, 512, 513, 575, 1025, 64 * 15, 64 * 16 + 1, "second trip"]


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("c", POSITION, ids=[c["name"] for c in POSITION])
def test_a_samples_value_does_not_depend_on_its_place_in_the_batch(oracle, c, n):
    """1, 7, 8, 9, 15, 16, 17 tiles around the kernel's split into 8 ranges, ragged last tiles, and one tile more than one trip of the
    persistent tile loop holds: the 1000 coordinates of (a) repeated and permuted, every output the bits its coordinate has in the
    1000-sample call, every one of the n written and nothing behind them"""
    assert len(POSITION) == 2
    model = Model(oracle, c)
    coords = R.batch(c, 1000)[0]
    base = api.neural_inference(model.vol, coords)
    assert IR.is_half(base).all()
    if n == "second trip":
        n = 64 * (8 if c["W"] == 128 else 4) * 4 * device_cus() + 37
    idx = np.random.default_rng(4000 + n).permutation(np.arange(max(n, 1000)) % 1000)[:n]
    d_coords = api.DeviceArray.from_numpy(np.ascontiguousarray(coords[idx]))
    d_out = api.DeviceArray.from_numpy(np.full(n + 64, SENTINEL, np.uint32).view(np.float32))
    check(lib().vnrAmdNeuralVolumeInference(model.vol.h, n, d_coords.ptr, d_out.ptr, None))
    check(lib().vnrAmdSynchronize())
    out = bits(d_out.numpy())
    unwritten = np.nonzero(out[:n] == SENTINEL)[0]
    assert unwritten.size == 0, (n, unwritten.size, unwritten[:8])
    assert (out[n:] == SENTINEL).all(), (n, np.nonzero(out[n:] != SENTINEL)[0][:8])
    differ = np.nonzero(out[:n] != bits(base)[idx])[0]
    assert differ.size == 0, (n, differ.size, differ[:8], idx[differ[:8]])
