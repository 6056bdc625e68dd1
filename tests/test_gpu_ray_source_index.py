"""The numbering of a march's surviving rays (csrc/pack_rays.h pack_rays_block, run on its own through vnrAmdDebugRaySourceIndex): group g of 64
rays leaves counts[g] & 0xff survivors in slots 64 g .. of the list the march wrote, and dense ray i of the next march is told its slot, in
group order.  Against a numpy restatement, exactly."""
import numpy as np
import pytest

from instantvnr_amd import api

pytestmark = pytest.mark.gpu

# one work item (4 groups, 256 slots) and less, items that end inside the last block's groups, many items; the last size is a part large
# enough for the items of 64 groups (pack_rays.h pack_item_groups), the last of which holds 4
N_IN = (1, 64, 255, 256, 257, 1024, 16640, 65536 + 192, 262144 + 197)
PATTERNS = ("none", "all", "random", "two_far_apart", "first_only", "last_only")


def survivors(pattern, n_in, rng):
    n_groups = (n_in + 63) // 64
    room = np.minimum(64, n_in - 64 * np.arange(n_groups)).astype(np.uint32)   # rays of each group
    c = np.zeros(n_groups, np.uint32)
    if pattern == "all":
        c = room.copy()
    elif pattern == "random":
        c = rng.integers(0, room + 1).astype(np.uint32)
    elif pattern == "two_far_apart":   # two groups with 300 empty ones between them (fewer where the array is shorter): more than one item of nothing
        a = min(3, n_groups - 1)
        b = min(a + 301, n_groups - 1)
        c[a] = rng.integers(1, room[a] + 1)
        c[b] = rng.integers(1, room[b] + 1)
    elif pattern == "first_only":
        c[0] = rng.integers(1, room[0] + 1)
    elif pattern == "last_only":
        c[-1] = rng.integers(1, room[-1] + 1)
    return c


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n_in", N_IN)
def test_dense_rays_are_numbered_in_group_order(n_in, pattern):
    rng = np.random.default_rng(1000 * N_IN.index(n_in) + PATTERNS.index(pattern))
    c = survivors(pattern, n_in, rng)
    # the bytes above the low one belong to the frame statistics (rays alive when the march began to emit): any pattern, so that a missing
    # `& 0xff` shows
    counts = c | (rng.integers(0, 1 << 24, c.shape).astype(np.uint32) << 8)
    src, alive = api.ray_source_index(counts, n_in)
    want = np.concatenate([64 * g + np.arange(k) for g, k in enumerate(c)]).astype(np.uint32)
    assert alive == int(c.sum())
    assert src.dtype == np.uint32 and np.array_equal(src, want)
