#!/usr/bin/env python3
"""Records tests/golden/ray_lists_parent.json: the sha-256 of the frames and the four frame statistics of every case of tests/ray_lists_cases.py
(synchronous frames, one ray part), as the library renders them.

    python tests/golden/make_ray_lists_parent.py [out.json]     # on a GPU box; VNR_AMD_LIB_PATH chooses the build of the library

The committed file was recorded ONCE, from a build of the commit before the streaming marcher's ray lists were indexed instead of packed
(52ab763), whose packing kernel copied every survivor into a dense list: tests/test_gpu_ray_lists.py holds every later build to those frames bit
for bit.  Run it again only from a build whose frames are known to be right, e.g. after a change that is MEANT to change them.  The file
holds digests and integers only; this script reads nothing but the library and the repository's own modules."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import ray_lists_cases as rl  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ray_lists_parent.json")
    os.environ.update(rl.ENV)
    os.environ["VNR_AMD_RENDER_HALVES"] = "1"
    from instantvnr_amd import api
    from instantvnr_amd import synthetic as syn
    sv = api.vnrCreateSimpleVolume(syn.analytic_volume(rl.DIM))
    out = {}
    for scene in rl.SCENES:
        volume = rl.make_volume(scene, sv)
        for mode in rl.MODES:
            for size in rl.SIZES:
                for tfn_kind in rl.TFNS:
                    frames, stats, schedule = rl.render(volume, rl.transfer_function(tfn_kind), size, mode, False)
                    cid = rl.case_id(scene, size, tfn_kind, mode)
                    out[cid] = {"sha256": rl.digest(frames), "stats": [stats[k] for k in rl.STAT_KEYS]}
                    print(cid, out[cid], schedule, flush=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(out)} cases to {out_path}; library build {api.lib().vnrAmdBuildId().decode()}")


if __name__ == "__main__":
    main()
