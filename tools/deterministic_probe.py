#!/usr/bin/env python3
"""Deterministic training against the production step (profiles/deterministic_training.txt).

  timing [--model c4|example] [--pairs 6] [--block 20]   step time, production and deterministic alternating in ONE process on ONE volume
  repro  [--runs 3] [--steps 1500]                        bench.py's training schedule (C4 model, 1024^3 Perlin volume, seed 20240611):
                                                          params checksum, train_loss and PSNR of N deterministic and N production runs

Both legs train through vnrNeuralVolumeTrain (GPU sampler); `timing` switches the mode with vnrAmdNeuralVolumeSetDeterministicTraining
between blocks of steps.  Run `timing` under `rocprofv3 --kernel-trace --stats` for the per-kernel split."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instantvnr_amd import api, dist, synthetic as syn  # noqa: E402
from instantvnr_amd._lib import check, lib  # noqa: E402


def c4_setup(size=1024):
    os.environ.setdefault("VNR_AMD_INIT_SEED", "20240611")
    pls = float(np.exp(np.log(size / 16.0) / 15))
    sv = api.vnrCreateSimpleVolumePerlin((size, size, size), seed=42, octaves=4, base_frequency=6.0)
    cfg = syn.model_config(n_levels=16, n_features=2, log2_hashmap_size=22, base_resolution=16, n_hidden_layers=3, per_level_scale=pls)
    return sv, cfg


def example_setup(size=256):
    os.environ.setdefault("VNR_AMD_INIT_SEED", "20240611")
    sv = api.vnrCreateSimpleVolumePerlin((size, size, size), seed=42, octaves=4, base_frequency=6.0)
    cfg = syn.model_config(n_levels=8, n_features=8, log2_hashmap_size=19, base_resolution=16, n_hidden_layers=4, per_level_scale=2.0)
    return sv, cfg


def timing(a):
    sv, cfg = c4_setup() if a.model == "c4" else example_setup()
    nv = api.vnrCreateNeuralVolume(cfg, sv, online_macrocell_construction=False)
    L = lib()
    plan = {m: None for m in (False, True)}
    for m in (False, True):
        api.neural_set_deterministic_training(nv, m)
        plan[m] = api.neural_grid_backward_plan(nv, 65536)
        api.vnrNeuralVolumeTrain(nv, a.block, True)   # warm-up of both forms (allocations, first launches)
    check(L.vnrAmdSynchronize())
    ms = {False: [], True: []}
    for _ in range(a.pairs):
        for m in (False, True):
            api.neural_set_deterministic_training(nv, m)
            check(L.vnrAmdSynchronize())
            t0 = time.perf_counter()
            api.vnrNeuralVolumeTrain(nv, a.block, True)
            check(L.vnrAmdSynchronize())
            ms[m].append((time.perf_counter() - t0) * 1e3 / a.block)
    for m in (False, True):
        name = "deterministic" if m else "production"
        v = np.array(ms[m])
        print(f"[timing] {a.model} {name:13s} step {v.mean():.3f} ms (min {v.min():.3f}, max {v.max():.3f}, {a.pairs} blocks of {a.block})  plan {plan[m]}")
    print(f"[timing] {a.model} ratio deterministic / production {np.mean(ms[True]) / np.mean(ms[False]):.3f}")


def repro(a):
    L = lib()
    for m in (True, False):
        for r in range(a.runs):
            svr, cfg = c4_setup()   # a fresh ground truth per run: its sampler starts at offset 0 (the bench builds one per process)
            nv = api.vnrCreateNeuralVolume(cfg, svr, online_macrocell_construction=False)
            api.neural_set_deterministic_training(nv, m)
            api.vnrNeuralVolumeTrain(nv, a.steps, True)
            check(L.vnrAmdSynchronize())
            loss = api.vnrNeuralVolumeGetTrainingLoss(nv)
            psnr = api.vnrNeuralVolumeGetPSNR(nv)
            print(f"[repro] {'deterministic' if m else 'production   '} run {r}: checksum {dist.params_checksum(nv):#014x} train_loss {loss:.9f} "
                  f"psnr {psnr:.4f} dB", flush=True)
            del nv, svr


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("what", choices=["timing", "repro"])
    p.add_argument("--model", choices=["c4", "example"], default="c4")
    p.add_argument("--pairs", type=int, default=6)
    p.add_argument("--block", type=int, default=20)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--steps", type=int, default=1500)
    a = p.parse_args()
    api.check(api.lib().vnrAmdInit(0))
    timing(a) if a.what == "timing" else repro(a)


if __name__ == "__main__":
    main()
