#!/usr/bin/env python3
"""Records tests/golden/eval_five_waves_parent.npy: the evaluation kernel's outputs (float32) for the model and the points of
tests/eval_five_waves_cases.py, with the brick image switched off.

    python tests/golden/make_eval_five_waves_parent.py [out.npy]     # on a GPU box; VNR_AMD_LIB_PATH chooses the build of the library

The committed file was recorded ONCE, from a build of the commit before the evaluation kernel was brought down to 96 registers (5118795):
tests/test_gpu_eval_five_waves.py holds every later build to those values bit for bit, whichever path reads the levels.  Run it again only
from a build whose values are known to be right.  This script reads nothing but the library and the repository's own modules."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import eval_five_waves_cases as cases  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "eval_five_waves_parent.npy")
    from instantvnr_amd import api
    from instantvnr_amd._lib import check, lib
    vol = cases.make_volume()
    check(lib().vnrAmdNeuralVolumeSetBrickImageMode(vol.h, 0))
    off = api.neural_inference(vol, cases.points())
    check(lib().vnrAmdNeuralVolumeSetBrickImageMode(vol.h, 1))
    on = api.neural_inference(vol, cases.points())
    assert api.neural_brick_image(vol)["in_use"] and np.array_equal(off.view(np.uint32), on.view(np.uint32))
    assert np.isfinite(off).all() and float(np.abs(off).max()) > 0.0
    np.save(out_path, off)
    print(f"wrote {off.shape[0]} values to {out_path}; library build {api.lib().vnrAmdBuildId().decode()}")


if __name__ == "__main__":
    main()
