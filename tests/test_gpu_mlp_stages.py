"""Every stage of the MLP training step held to ITS OWN INPUTS at rounding level (DESIGN.md 4.3 "the chain"): the fused forward's training
store, loss_grad_kernel, mlp_backward_kernel, weight_grad_mfma_kernel and weight_grad_reduce_kernel against tests/mlp_stage_ref.py, each
from the buffers the library kept (vnrAmdNeuralVolumeTrainingBuffer 0 - 3 and 5 - 7), at the shapes where the kernels branch.  The ReLU mask
is read from the stored activation and the L1 sign from the stored output, so nothing is kept away from a kink, no element is skipped and
nothing is tried twice; the bounds are derived, per element (tests/test_mlp_stage_ref_host.py shows on the CPU that they accept every order
of the sums and reject a single lost term).  The 3 % tests of test_gpu_train.py / test_gpu_fuzz.py hold the independent restatement end to
end; this file holds the kernels."""
import ctypes as C
import os
import sys

import pytest

from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_stage_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = R.cases()
EXTRA = R.extra_cases()


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    monkeypatch.delenv("VNR_AMD_DETERMINISTIC", raising=False)
    monkeypatch.delenv("VNR_AMD_TRAIN_OVERLAP", raising=False)


def device_cus():
    """the CU count from the device properties, through the HIP runtime the library itself loaded (called with a volume alive: the device is chosen)"""
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = C.CDLL(path)
    dev, v = C.c_int(), C.c_int()
    assert hip.hipGetDevice(C.byref(dev)) == 0
    assert hip.hipDeviceGetAttribute(C.byref(v), 63, dev) == 0 and v.value > 0          # hipDeviceAttributeMultiprocessorCount
    return v.value


def model_config(c):
    cfg = syn.model_config(n_levels=c["L"], n_features=c["F"], log2_hashmap_size=c["log2T"], base_resolution=c["base"], n_neurons=c["W"],
                           n_hidden_layers=c["H"], per_level_scale=c["pls"])
    cfg["loss"]["otype"] = c["loss"]
    cfg["network"]["activation"] = c["act"]
    cfg["network"]["output_activation"] = c["out_act"]
    return cfg


def set_params(oracle, vol, c):
    info = api.neural_info(vol)
    assert info["padded_width"] == c["in_w"] and info["n_neurons"] == c["W"] and info["mfma_training_kernels"] == 1, info
    n_mlp = oracle.mlp_n_params(c["in_w"], c["W"], c["H"] - 1)
    params = syn.random_params(info["n_params"], n_mlp, seed=c["seed"], mlp_scale=c["mlp_scale"])
    api.neural_set_params_fp16(vol, params)
    return params[:n_mlp], n_mlp


def step_and_check(vol, c, mlp, n_mlp, n, seed_offset=0, first_blob=None):
    """one ForwardBackward, every link of the chain on what it left, the non-vacuity conditions on the library's own values"""
    coords, targets = R.batch(c, n, seed_offset)
    api.neural_forward_backward(vol, coords, targets)
    bufs = R.download(vol, n, c, n_mlp)
    rep = R.run_chain(bufs, mlp, c, targets, first_blob=first_blob)
    line = "%s n=%d: " % (c["name"], n) + ", ".join("%s %.3f" % kv for kv in sorted(rep.ratios.items()))
    print(line)
    if os.environ.get("VNR_STAGE_LOG"):
        with open(os.environ["VNR_STAGE_LOG"], "a") as f:
            f.write(line + "\n")
    assert not rep.failures, (c["name"], rep.failures)
    assert not R.vacuous(rep, n), (c["name"], R.vacuous(rep, n))
    return bufs


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_every_stage_of_the_training_step_is_its_inputs_exact_result_within_rounding(oracle, c):
    vol = api.vnrCreateNeuralVolume(model_config(c), (32, 32, 32))
    mlp, n_mlp = set_params(oracle, vol, c)
    n = R.batch_size(c, device_cus() if c["n"] == R.N_FROM_CUS else 0)
    step_and_check(vol, c, mlp, n_mlp, n)


def test_a_second_call_before_the_optimizer_step_adds_within_rounding(oracle):
    c = EXTRA["accumulation"]
    vol = api.vnrCreateNeuralVolume(model_config(c), (32, 32, 32))
    mlp, n_mlp = set_params(oracle, vol, c)
    first = step_and_check(vol, c, mlp, n_mlp, 1000)
    step_and_check(vol, c, mlp, n_mlp, 777, seed_offset=1, first_blob=first["grads"])


def test_a_reconfigured_model_of_the_same_mlp_size_keeps_its_padding_zero(oracle):
    """64 neurons x 1 hidden layer, then 32 x 2 on the SAME volume: both have 2 048 MLP parameters in other layouts, so whatever the first left
    in the slab or the blob would sit in the second's padded rows and columns"""
    a, b = EXTRA["reconfiguration a"], EXTRA["reconfiguration b"]
    sv = api.vnrCreateSimpleVolume(syn.analytic_volume(16))
    vol = api.vnrCreateNeuralVolume(model_config(a), sv)
    mlp, n_mlp = set_params(oracle, vol, a)
    step_and_check(vol, a, mlp, n_mlp, 1000)
    api.neural_train_end(vol)
    api.vnrNeuralVolumeSetModel(vol, model_config(b))
    mlp_b, n_mlp_b = set_params(oracle, vol, b)
    assert n_mlp_b == n_mlp
    step_and_check(vol, b, mlp_b, n_mlp_b, 1000)          # (rows 1 .. 15 of the last layer and the padded feature columns: exactly zero, in the chain)


def test_a_smaller_batch_after_a_larger_one_on_the_same_volume(oracle):
    c = EXTRA["shrink"]
    vol = api.vnrCreateNeuralVolume(model_config(c), (32, 32, 32))
    mlp, n_mlp = set_params(oracle, vol, c)
    step_and_check(vol, c, mlp, n_mlp, 1025)
    api.neural_train_end(vol, grad_scale=0.0)            # consumes and clears the gradients (l2 moves the weights: set them again)
    mlp, n_mlp = set_params(oracle, vol, c)
    step_and_check(vol, c, mlp, n_mlp, 63, seed_offset=1)
