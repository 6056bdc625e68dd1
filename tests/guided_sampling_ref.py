"""numpy restatement of error-guided sampling (include/vnr_amd.h "error-guided training batches"): the sampling table, the pcg32 stream,
the cell choice (Python integers for the 128-bit product), the coordinates in float32 and the trilinear value through the oracle.
Everything in the definition is an integer or a single fp32 / fp64 rounding, so every result here is meant to equal the library's
bit for bit.  A helper module of tests/test_guided_sampling_host.py and tests/test_gpu_guided_sampling.py, not a test file."""
import numpy as np

MULT = 0x5851F42D4C957F2D
M64 = (1 << 64) - 1
DEFAULT_SEED, DEFAULT_STREAM = 1337, 0xDA3E39CB94B95BDB
CELL = 16
ONE_BELOW = np.float32(1.0) - np.float32(2.0 ** -24)   # 0x1.fffffep-1f


def cell_dims(dims):
    return tuple((int(d) + CELL - 1) // CELL for d in dims)


def table(weights, uniform_fraction):
    """-> dict(q, cdf (uint64), total, threshold, n_cells); ValueError, by name, for what the library refuses"""
    w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
    f = np.float32(uniform_fraction)
    if not (f >= 0 and f <= 1):
        raise ValueError("uniform_fraction")
    if np.isnan(w).any() or np.isinf(w).any() or (w < 0).any():
        raise ValueError("invalid weights")
    bits = w.view(np.uint32) & np.uint32(0x7FFFFFFF)          # (-0.0f counts as 0)
    wmax = bits.max().reshape(1).view(np.float32)[0]          # the unsigned maximum over the float bits
    if wmax == 0:
        raise ValueError("all weights are zero")
    q = np.rint((w.astype(np.float64) / np.float64(wmax)) * 16777216.0).astype(np.uint64)
    q[(bits != 0) & (q == 0)] = 1
    cdf = np.cumsum(q, dtype=np.uint64)
    return {"q": q, "cdf": cdf, "total": int(cdf[-1]), "n_cells": int(w.size),
            "threshold": int(np.rint(np.float64(f) * 4294967296.0))}


def _seeded_state(seed, stream):
    inc = ((stream << 1) | 1) & M64
    state = inc                                   # state = 0, one step
    state = (state + seed) & M64
    state = (state * MULT + inc) & M64
    return state, inc


def _advance(state, inc, delta):
    """the LCG jump of pcg32's advance, for an array of distances -> uint64 states"""
    delta = np.asarray(delta, np.uint64)
    am, ap = np.ones_like(delta), np.zeros_like(delta)
    cm, cp = MULT, inc
    for bit in range(64):
        rest = delta >> np.uint64(bit)
        if not rest.any():
            break
        take = (rest & np.uint64(1)).astype(bool)
        am = np.where(take, am * np.uint64(cm), am)
        ap = np.where(take, ap * np.uint64(cm) + np.uint64(cp), ap)
        cp = ((cm + 1) * cp) & M64
        cm = (cm * cm) & M64
    return am * np.uint64(state) + ap


def _output(old):
    xs = (((old >> np.uint64(18)) ^ old) >> np.uint64(27)).astype(np.uint32)
    rot = (old >> np.uint64(59)).astype(np.uint32)
    return (xs >> rot) | (xs << ((np.uint32(32) - rot) & np.uint32(31)))


def pcg32_uints(n, offset=0, seed=DEFAULT_SEED, stream=DEFAULT_STREAM, per_element=1):
    """uint32 [n, per_element]: element e holds the draws at stream positions offset + per_element * e ... + per_element - 1"""
    state, inc = _seeded_state(seed, stream)
    s = _advance(state, inc, (np.uint64(offset) + np.uint64(per_element) * np.arange(n, dtype=np.uint64)))
    out = np.empty((n, per_element), np.uint32)
    for j in range(per_element):
        out[:, j] = _output(s)
        s = s * np.uint64(MULT) + np.uint64(inc)
    return out


def uint_to_float(u):
    """pcg32's next_float: (u >> 9) | 0x3f800000 as a float, minus 1"""
    return ((np.asarray(u, np.uint32) >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)


def uniform_coords(n, offset=0, seed=DEFAULT_SEED, stream=DEFAULT_STREAM):
    """what vnrAmdSimpleVolumeTakeSamples draws for the unit box: 3 floats per sample"""
    return uint_to_float(pcg32_uints(n, offset, seed, stream, 3))


def choose_cells(tab, r_hi, r_lo):
    """k = the high 64 bits of r * total; the first cell with cdf > k"""
    total = tab["total"]
    k = np.array([(((int(h) << 32) | int(l)) * total) >> 64 for h, l in zip(r_hi, r_lo)], dtype=np.uint64)
    return np.searchsorted(tab["cdf"], k, side="right")


def draw(tab, dims, n, offset=0, seed=DEFAULT_SEED, stream=DEFAULT_STREAM):
    """-> (coords float32 [n, 3], uniform mask [n], cell index [n] (of the weighted branch; also computed where the sample is uniform))"""
    u = pcg32_uints(n, offset, seed, stream, 6)
    uniform = u[:, 0].astype(np.uint64) < np.uint64(tab["threshold"]) if tab["threshold"] < (1 << 32) else np.ones(n, bool)
    cells = choose_cells(tab, u[:, 1], u[:, 2])
    uf = uint_to_float(u[:, 3:6])
    cd = cell_dims(dims)
    c_axis = (cells % cd[0], (cells // cd[0]) % cd[1], cells // (cd[0] * cd[1]))
    coords = np.empty((n, 3), np.float32)
    for a in range(3):
        lo = (CELL * c_axis[a]).astype(np.int64)
        size = np.minimum(CELL, int(dims[a]) - lo)
        t = (uf[:, a] * size.astype(np.float32)).astype(np.float32)
        t = (lo.astype(np.float32) + t).astype(np.float32)
        t = (t * (np.float32(1.0) / np.float32(dims[a]))).astype(np.float32)
        coords[:, a] = np.where(uniform, uf[:, a], np.minimum(t, ONE_BELOW))
    return coords, uniform, cells


def values(vol_zyx, coords):
    """the cell-centred trilinear lookup of the samplers, through the C oracle"""
    from oracle import oracle
    return oracle.sample_volume(vol_zyx, coords, nodal=False)
