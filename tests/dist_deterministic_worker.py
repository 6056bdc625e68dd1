"""One rank of tests/test_gpu_deterministic_training.py's data-parallel check: deterministic training over the host-staged "shm" transport,
started twice by the parent with the same settings.  usage: dist_deterministic_worker.py <out.npz>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from instantvnr_amd import api, dist as vdist, synthetic as syn  # noqa: E402


def main():
    out_path = sys.argv[1]
    ctx = vdist.init_from_env()
    os.environ["VNR_AMD_INIT_SEED"] = str(100 + ctx.rank)   # different replicas: the first step synchronises them
    sv = api.vnrCreateSimpleVolume(syn.analytic_volume(32))
    nv = api.vnrCreateNeuralVolume(syn.model_config(n_levels=6, n_features=2, log2_hashmap_size=13, base_resolution=4, n_hidden_layers=2,
                                                    per_level_scale=1.5), sv, online_macrocell_construction=False)
    api.neural_set_deterministic_training(nv, True)
    vdist.train_data_parallel(ctx, nv, 20)
    out = {"rank": ctx.rank, "transport": ctx.transport or "none", "deterministic": api.neural_get_deterministic_training(nv),
           "step": api.vnrNeuralVolumeGetTrainingStep(nv), "loss": api.vnrNeuralVolumeGetTrainingLoss(nv),
           "params": api.neural_get_params_fp16(nv).view(np.uint16)}
    vdist.barrier()
    np.savez(out_path, **out)
    vdist.finalize()


if __name__ == "__main__":
    main()
