"""The evaluation kernel at five waves per SIMD (csrc/infer_kernel.h).  (a) Resources, from the loaded code object
(vnrAmdDebugEvalKernelResources): the bench instance fits 96 vector registers without scratch, and no common-kind inference instance of widths
16 / 32 / 64 has scratch.  (b) Values: one small model whose levels take all three encode paths (dense, hashed four-entry groups, brick image)
gives the same bits with the brick image off, in its small tier and in its full tier, and those are the bits of the commit before
(tests/golden/eval_five_waves_parent.npy, recorded by tests/golden/make_eval_five_waves_parent.py).  Model and points:
tests/eval_five_waves_cases.py."""
import os

import numpy as np
import pytest

import eval_five_waves_cases as cases
from instantvnr_amd import api
from instantvnr_amd._lib import check, lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_five_waves_parent.npy")
SHAPES = ([(1, k) for k in (16, 32)] + [(2, k) for k in (16, 32, 48, 64)] + [(f, k) for f in (4, 8) for k in range(16, 129, 16)])


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def pts():
    return cases.points()


def bits(values):
    return np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)


def by_brick_mode(vol, pts):
    """outputs with the brick image off, in its small tier and in its full tier"""
    out = {}
    check(lib().vnrAmdNeuralVolumeSetBrickImageMode(vol.h, 0))
    out["off"] = api.neural_inference(vol, pts)
    assert not api.neural_brick_image(vol)["in_use"]
    # small tier: the automatic policy builds it at the first launch of a frame's size after the parameters changed
    check(lib().vnrAmdNeuralVolumeSetBrickImageMode(vol.h, -1))
    api.neural_inference(vol, cases.big_launch_points())
    st = api.neural_brick_image(vol)
    assert st["in_use"] and st["tier"] == 1 and st["levels"] == 0b11110000, st
    out["small"] = api.neural_inference(vol, pts)
    assert api.neural_brick_image(vol)["tier"] == 1
    check(lib().vnrAmdNeuralVolumeSetBrickImageMode(vol.h, 1))
    out["full"] = api.neural_inference(vol, pts)
    st = api.neural_brick_image(vol)
    assert st["in_use"] and st["tier"] == 2 and st["levels"] == 0b11110000, st
    return out


def test_the_bench_instance_fits_five_waves_without_scratch():
    check(lib().vnrAmdInit(-1))
    r = api.eval_kernel_resources(2, 32, 64)
    print("fused_infer_kernel<2, 32, 64, 0, false>:", r)
    assert 0 < r["regs"] <= 96 and r["scratch_bytes"] == 0, r


def test_no_common_inference_instance_has_scratch():
    check(lib().vnrAmdInit(-1))
    for width in (16, 32, 64):
        for f, k in SHAPES:
            r = api.eval_kernel_resources(f, k, width)
            print(f"fused_infer_kernel<{f}, {k}, {width}, 0, false>:", r)
            assert r["regs"] > 0 and r["scratch_bytes"] == 0, (f, k, width, r)


def test_values_are_the_parents_on_every_level_path(golden, pts, monkeypatch):
    monkeypatch.delenv("VNR_AMD_BRICK", raising=False)
    out = by_brick_mode(cases.make_volume(), pts)
    assert golden.shape == (pts.shape[0],) and np.isfinite(golden).all()
    for mode, values in out.items():
        differ = np.flatnonzero(bits(values) != bits(golden))
        print(mode, "values that differ from the parent's:", differ.size)
        assert np.array_equal(bits(values), bits(out["off"])), mode
        assert differ.size == 0, (mode, differ[:8], values[differ[:8]], golden[differ[:8]])

