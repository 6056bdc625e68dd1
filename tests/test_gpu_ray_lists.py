"""The streaming marcher's two ray lists (csrc/pack_rays.h): a march leaves the survivors of every 64-ray group in the group's slots of the list it
writes, the evaluation kernel's prologue (or, without such a kernel, a kernel behind the evaluation) numbers them in group order, and the next
march reads its rays through that index from where they lie; the two lists swap roles every iteration.  Nothing of that may show in a frame:
(a) frames and statistics are the same bit for bit for 1, 2 and 3 ray parts, synchronous and pipelined; (b) they are the frames and statistics of
the commit before, which copied the survivors into a dense list (tests/golden/ray_lists_parent.json, recorded by tests/golden/make_ray_lists_parent.py).
Cases: tests/ray_lists_cases.py."""
import json
import os

import pytest

import ray_lists_cases as rl
from instantvnr_amd import api
from instantvnr_amd import synthetic as syn

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ray_lists_parent.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ground_truth():
    return api.vnrCreateSimpleVolume(syn.analytic_volume(rl.DIM))


@pytest.mark.parametrize("mode", rl.MODES)
@pytest.mark.parametrize("scene", rl.SCENES)
def test_frames_are_those_of_the_packed_lists_for_every_schedule(ground_truth, golden, monkeypatch, scene, mode):
    for k, v in rl.ENV.items():
        monkeypatch.setenv(k, v)
    volume = rl.make_volume(scene, ground_truth)
    for size in rl.SIZES:
        for tfn_kind in rl.TFNS:
            cid = rl.case_id(scene, size, tfn_kind, mode)
            tfn = rl.transfer_function(tfn_kind)
            want = None
            for parts in (1, 2, 3):
                monkeypatch.setenv("VNR_AMD_RENDER_HALVES", str(parts))
                for pipelined in (False, True):
                    frames, stats, schedule = rl.render(volume, tfn, size, mode, pipelined)
                    got = {"sha256": rl.digest(frames), "stats": [stats[k] for k in rl.STAT_KEYS]}
                    print(cid, parts, "pipelined" if pipelined else "synchronous", got, schedule)
                    # which path ran: the coupled loop with that many parts, the survivors numbered inside the evaluation kernel where there is one with 4-wave blocks
                    assert not schedule["decoupled"] and schedule["n_parts"] == parts and schedule["n_iters"] == 8, (cid, schedule)
                    assert schedule["fused_pack"] == (scene == "neural64"), (cid, schedule)
                    if want is None:
                        want = got
                        # the case is what it is meant to be: the volume in a corner of the image, and the rays' lifetimes
                        n_hit, n_pixels = stats["n_rays_hit"], size[0] * size[1]
                        assert 0.01 * n_pixels < n_hit < n_pixels / 8, (cid, n_hit)
                        if tfn_kind == "faint":
                            assert stats["n_iterations"] >= 6, (cid, stats)
                    assert got == want, (cid, parts, pipelined)                       # (a)
            assert want == golden[cid], (cid, want, golden[cid])                     # (b)
