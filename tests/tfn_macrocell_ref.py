"""numpy restatement of what decides which matter a frame shows: the transfer-function window and lookup, the per-macrocell opacity
bound and the macrocell a neural volume builds from its training samples.  Written from the definitions (core/renderer/raytracing.h:71-81,
147-155; core/macrocell.cu:11-73, 153-193; object.cpp:321-348), vectorised.  Everything is integer work, comparisons and single fp32
roundings, so every result here is meant to equal the C oracle's and the library's bit for bit.

Also the input sets that tests/test_tfn_macrocell_ref_host.py (against the C oracle) and tests/test_gpu_tfn_macrocell.py (against the
library) share, and, behind `fault=`, five deliberately broken variants with which the host test shows that those inputs are sharp.
A helper module, not a test file."""
import numpy as np

F32 = np.float32
CELL = 16

# ---------------------------------------------------------------------------------------------------------------------- input sets
VOLUMES = [(19, 37, 50), (16, 16, 16), (48, 32, 17)]          # (x, y, z): ragged 2 x 3 x 4 cells, one cell, 3 x 2 x 2 cells
BATCH_SIZES = [1, 255, 256, 257, 5000]
WINDOWS = [(0.0, 1.0), (0.25, 0.7), (0.5, 0.5 + 2.0 ** -20), (-0.5, 0.4), (0.6, 7.0)]
# 1228 / 1229: the last pair of equal tables in the compose kernels' LDS and the first outside; 8192 / 8193: the last table the bound kernel
# stages in its own LDS and the first it reads from global memory; 16384 / 16385: 64 KB of fp32 and the first table beyond
ALPHA_LENGTHS = [1, 2, 3, 17, 256, 1228, 1229, 4096, 8192, 8193, 16384, 16385, 65536]
FAULTS = ("no_plus_apron", "il_without_minus_one", "no_window_clamp", "len_for_len_minus_one", "negative_channels_swapped")


def batch(dims, n, seed=0):
    """-> (coords [n, 3], values [n]) float32.  Coordinates uniform in [-0.1, 1.1]; on every axis up to 1000 of them (a third of a small
    batch) are exactly fp32(k / d), k = 0 .. d, so that voxel faces and, at multiples of 16, cell faces are hit; then the corners and a
    point far outside.  Values uniform in [-2, 3] with +-0 and +-1 among them, so that v - 1 and v + 1 cross zero."""
    rng = np.random.default_rng([seed, n, *dims])
    c = rng.uniform(-0.1, 1.1, (n, 3)).astype(F32)
    m = min(1000, n // 3)
    for a in range(3):
        rows = rng.choice(n, m, replace=False)
        k = rng.integers(0, dims[a] + 1, m)
        c[rows, a] = k.astype(F32) / F32(dims[a])
    special = np.array([(1e30, -1e30, 0.5), (0, 0, 0), (1, 1, 1)], F32)
    c[:min(n, 3)] = special[:min(n, 3)]
    v = rng.uniform(-2.0, 3.0, n).astype(F32)
    edge = np.array([0.0, -0.0, 1.0, -1.0], F32)
    at = (np.arange(4) + 3) % n
    v[at] = edge
    if n >= 13:
        # the ends of the value range sit in voxels 15 and 16 of every axis that has a second cell: the largest value of cell 1 comes over
        # the + apron of cell 0's last voxel, the smallest of cell 0 over the - apron of cell 1's first, and from nowhere else
        # (the other two coordinates keep the three pairs in cells of their own)
        for a in range(3):
            if dims[a] > CELL:
                c[7 + 2 * a], v[7 + 2 * a] = 0.01, 3.0
                c[8 + 2 * a], v[8 + 2 * a] = 0.01, -2.0
                c[8 + 2 * a, (a + 2) % 3] = 0.99
                c[7 + 2 * a, a] = (F32(CELL - 1) + F32(0.5)) / F32(dims[a])
                c[8 + 2 * a, a] = (F32(CELL) + F32(0.5)) / F32(dims[a])
    return c, v


def alpha_table(n, seed=0):
    """n opacities in [0, 1): white noise, so that a neighbouring entry is a new maximum about as often as not"""
    return np.random.default_rng([11, seed, n]).uniform(0.0, 1.0, n).astype(F32)


def bound_tables(n):
    """the opacity tables the bound is checked with: white noise, and a rising and a falling ramp, whose maximum over any index range is
    the range's last / first entry, so that a range one entry short at either end gives another bound whatever the cell"""
    ramp = (np.arange(n, dtype=np.float64) + 1.0) / n
    return {"noise": alpha_table(n), "rising": ramp.astype(F32), "falling": ramp[::-1].astype(F32)}


def color_table(n, seed=0):
    return np.random.default_rng([12, seed, n]).uniform(0.0, 1.0, (n, 3)).astype(F32)


def lookup_values(window, n_table, n=600, seed=0):
    """sample values for the lookup under `window` and a table of n_table entries: spread over and around the window, the window's ends,
    and the values that land on (and an ulp beside) the table's nodes"""
    lo, hi, _ = tfn_window(*window)
    rng = np.random.default_rng([13, seed, n_table])
    span = float(hi) - float(lo)
    v = rng.uniform(float(lo) - 0.3 * span - 0.1, float(hi) + 0.3 * span + 0.1, n).astype(F32)
    k = rng.integers(0, n_table, 64)
    nodes = (F32(lo) + (k.astype(F32) / F32(max(n_table - 1, 1))) * F32(span)).astype(F32)
    return np.concatenate([v, nodes, np.nextafter(nodes, F32(np.inf)), np.nextafter(nodes, F32(-np.inf)),
                           np.array([lo, hi, 0.0, -0.0, 1.0, -2.0, 3.0], F32)]).astype(F32)


def ragged_volume():
    """[z, y, x] = 50 x 37 x 19 voxels in [0, 1] with 0 and 1 among them (the load-time normalisation is then the identity): a ramp
    along the diagonal under a little noise, so that a cell sees a part of the value range only and its bound depends on where the
    ends of that part fall in the table"""
    x, y, z = VOLUMES[0]
    gz, gy, gx = np.meshgrid(np.linspace(0, 1, z), np.linspace(0, 1, y), np.linspace(0, 1, x), indexing="ij")
    v = 0.25 * gx + 0.3 * gy + 0.45 * gz + np.random.default_rng(14).uniform(-0.02, 0.02, (z, y, x))
    v = np.clip(v, 0.0, 1.0).astype(F32)
    v[0, 0, 0], v[-1, -1, -1] = 0.0, 1.0
    return v


def online_range():
    """the value range an online macrocell of the ragged volume holds after one batch squeezed to z < 0.71, with values that follow the
    position (from -2 to 3 along the diagonal, under a little noise): the cells of the last z layer are unvisited, (0, 0), the others
    hold a part of the range each, of either sign"""
    return explicit_update(empty_range(VOLUMES[0]), VOLUMES[0], *online_batch())


def online_batch():
    """the batch behind online_range(), for a library that is to build the same macrocell"""
    c, v = batch(VOLUMES[0], 5000, seed=5)
    c[:, 2] *= F32(0.64)
    ramp = np.clip(c, 0, 1).astype(np.float64) @ np.array([0.25, 0.3, 0.45 / 0.64])
    v[13:] = (-2.0 + 5.0 * ramp[13:] + np.random.default_rng(15).uniform(-0.1, 0.1, v.shape[0] - 13)).astype(F32)
    v[7:13] = v[13:19]
    return c, v


# --------------------------------------------------------------------------------------------------------------------- restatement
def cell_dims(dims):
    return tuple((int(d) + CELL - 1) // CELL for d in dims)


def empty_range(dims):
    cx, cy, cz = cell_dims(dims)
    return np.zeros((cz, cy, cx, 2), F32)


def tfn_window(lo, hi, data_lo=0.0, data_hi=1.0):
    """the range the library ends up with: the transfer function's clamped to the data's -> (lo', hi', 1 / (hi' - lo')) in fp32"""
    lo2, hi2 = max(F32(data_lo), F32(lo)), min(F32(data_hi), F32(hi))
    with np.errstate(divide="ignore"):
        return F32(lo2), F32(hi2), F32(F32(1.0) / F32(hi2 - lo2))


def _fma(a, b, c):
    """fp32 fused multiply-add: formed in float64 (24 bits x at most 17 bits, exact) and rounded once"""
    return (np.asarray(a, np.float64) * np.float64(b) + np.float64(c)).astype(F32)


def _normalise(window, values, fault):
    lo, hi, rcp = window
    v = np.asarray(values, F32)
    if fault != "no_window_clamp":
        v = np.minimum(np.maximum(v, lo), hi)
    return ((v - lo) * rcp).astype(F32)


def _nodal(table, v, fault):
    """array1dNodal + a linear, clamped, normalised 1-D texture fetch: entry k of a table of `len` sits at v = k / (len - 1)"""
    n = table.shape[0]
    scale = F32(n if fault == "len_for_len_minus_one" else n - 1)
    v = np.minimum(np.maximum(v, F32(0)), F32(1))
    t = (_fma(v, scale, 0.5) * (F32(1.0) / F32(n))).astype(F32)
    xb = (t * F32(n) - F32(0.5)).astype(F32)
    f0 = np.floor(xb)
    a = (xb - f0).astype(F32)
    i0 = np.clip(f0.astype(np.int64), 0, n - 1)
    i1 = np.clip(f0.astype(np.int64) + 1, 0, n - 1)
    if table.ndim == 2:
        a = a[:, None]
    return ((table[i0] * (F32(1.0) - a)).astype(F32) + (table[i1] * a).astype(F32)).astype(F32)


def tfn_lookup(colors, alphas, window, values, fault=None):
    """-> [n, 4] float32: rgb from the colour table, opacity from the opacity table (each of its own length; an empty table gives 0)"""
    v = _normalise(window, np.asarray(values, F32).ravel(), fault)
    out = np.zeros((v.shape[0], 4), F32)
    colors = np.asarray(colors, F32).reshape(-1, 3)
    alphas = np.asarray(alphas, F32).ravel()
    if colors.shape[0]:
        out[:, :3] = _nodal(colors, v, fault)
    if alphas.shape[0]:
        out[:, 3] = _nodal(alphas, v, fault)
    return out


def max_opacity(alphas, window, value_range, fault=None):
    """per cell, the largest opacity (at least 0) of the table entries that the cell's values can reach under the window: value_range
    holds (min - 1, max + 1), with (0, 0) for a cell nothing was seen in (its bounds cross and, on a table of more than three entries,
    select nothing)"""
    alphas = np.asarray(alphas, F32).ravel()
    n = alphas.shape[0]
    vr = np.asarray(value_range, F32)
    out = np.zeros(vr.shape[:-1], F32)
    if n == 0:
        return out
    scale = F32(n if fault == "len_for_len_minus_one" else n - 1)
    lower = _normalise(window, (vr[..., 0] + F32(1.0)).astype(F32), fault)
    upper = _normalise(window, (vr[..., 1] - F32(1.0)).astype(F32), fault)
    il = np.floor(_fma(lower, scale, 0.5)) - (0 if fault == "il_without_minus_one" else 1)
    iu = np.floor(_fma(upper, scale, 0.5)) + 1
    il = np.clip(il, 0, n - 1).astype(np.int64)
    iu = np.clip(iu, 0, n - 1).astype(np.int64)
    # the maximum over every [il, iu] at once: prefix maxima of the table from each block start, by doubling (a sparse table)
    levels = [alphas]
    while (1 << len(levels)) <= n:
        h = 1 << (len(levels) - 1)
        prev = levels[-1]
        levels.append(np.maximum(prev[:-h], prev[h:]))
    width = iu - il + 1
    some = width > 0
    k = np.zeros(width.shape, np.int64)
    k[some] = np.floor(np.log2(width[some])).astype(np.int64)
    flat = out.reshape(-1)
    for j, (a, b, kk, ok) in enumerate(zip(il.ravel(), iu.ravel(), k.ravel(), some.ravel())):
        if ok:
            t = levels[kk]
            flat[j] = max(F32(0), t[a], t[b - (1 << kk) + 1])
    return out


def explicit_update(value_range, dims, coords, values, fault=None):
    """a batch of samples merged into an online macrocell -> a new [cz, cy, cx, 2] array.  A sample lands in the voxel
    clamp(floor(fp32(c * d)), 0, d - 1); it counts for that voxel's cell and, where the voxel is the first or last of its 16 on an axis,
    for the neighbouring cell on that side too (and the diagonal ones), as far as the grid has them: min(., v - 1) and max(., v + 1)"""
    out = np.array(value_range, F32, copy=True)
    cz, cy, cx = out.shape[:3]
    cd = (cx, cy, cz)
    coords = np.asarray(coords, F32).reshape(-1, 3)
    values = np.asarray(values, F32).ravel()
    choices = []
    for a in range(3):
        d = int(dims[a])
        f = np.floor((coords[:, a] * F32(d)).astype(F32))
        vox = np.clip(f, 0, d - 1).astype(np.int64)
        own = vox // CELL
        side = np.where(vox % CELL == 0, -1, np.where(vox % CELL == CELL - 1, 1, 0))
        if fault == "no_plus_apron" and a == 1:
            side = np.where(side == 1, 0, side)
        other = own + side
        choices.append([(own, np.ones(own.shape, bool)), (other, (side != 0) & (other >= 0) & (other < cd[a]))])
    lo, hi = (values - F32(1.0)).astype(F32), (values + F32(1.0)).astype(F32)
    mins, maxs = out[..., 0].reshape(-1), out[..., 1].reshape(-1)
    for ix, okx in choices[0]:
        for iy, oky in choices[1]:
            for iz, okz in choices[2]:
                ok = okx & oky & okz
                cell = (ix + cx * (iy + cy * iz))[ok]
                if fault == "negative_channels_swapped":
                    neg = np.signbit(lo[ok])
                    np.minimum.at(mins, cell[~neg], lo[ok][~neg])
                    np.maximum.at(mins, cell[neg], lo[ok][neg])
                    neg = np.signbit(hi[ok])
                    np.maximum.at(maxs, cell[~neg], hi[ok][~neg])
                    np.minimum.at(maxs, cell[neg], hi[ok][neg])
                else:
                    np.minimum.at(mins, cell, lo[ok])
                    np.maximum.at(maxs, cell, hi[ok])
    out[..., 0], out[..., 1] = mins.reshape(cz, cy, cx), maxs.reshape(cz, cy, cx)
    return out
