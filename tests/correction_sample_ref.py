"""numpy restatement of random access to the corrected field (include/vnr_amd.h, "random access to the corrected field";
correction_gather_kernel and correction_sample_kernel of csrc/correction.hip): vnrAmdNeuralVolumeGatherVoxelsCorrected and
vnrAmdNeuralVolumeSampleCorrected from a serialised correction and the network's values alone.  Built on error_bound_ref (blob layout,
corrected_value) and correction_index_ref.code_at, so that both code routes are restated: "fixed" reads the cell table and the
fixed-width payload, "packed" reads the bit planes through the plane index.  Float steps are numpy float32 operations, double steps
numpy float64 operations, one rounding each and never an fma, so every comparison with the device has tolerance zero.

`broken` names one deliberate mistake (BROKEN); tests/test_correction_sample_host.py shows that each changes a result on the point
sets below, which is what makes a match with the device mean something."""
import struct

import numpy as np

import correction_index_ref as cir
import correction_pack_ref as cpr
import error_bound_ref as ebr

F32 = np.float32
BROKEN = ("i1-unclamped", "w-unclamped", "cx16", "no-zigzag", "neighbour-cell")


class Source:
    """a fixed-width blob as one route reads it"""

    def __init__(self, blob, route, broken=None):
        assert route in ("fixed", "packed") and broken in (None,) + BROKEN
        f = ebr.HEADER.unpack_from(blob, 0)
        assert f[0] == b"VNRCORR1" and f[1] == 1
        self.dtype, self.dims, self.kind, self.step = ebr.DTYPES[f[2]], tuple(f[3:6]), f[10], f[12]
        self.lo, self.hi = F32(f[8]), F32(f[9])
        self.route, self.broken = route, broken
        entries = [struct.unpack_from("<II", blob, ebr.HEADER.size + 8 * i) for i in range(f[6])]
        self.cells = np.array([c for c, _ in entries], np.int64)
        self.widths = [w for _, w in entries]
        self.voxels = [cpr.cell_voxels(self.dims, c) for c in self.cells]
        self.mc = [-(-d // 16) for d in self.dims]
        self.number = np.full(self.mc[0] * self.mc[1] * self.mc[2], -1, np.int64)      # cell -> its place among the flagged ones
        self.number[self.cells] = np.arange(len(entries))
        self.payload = blob[ebr.HEADER.size + 8 * len(entries):]
        self.offsets, at = [], 0
        for n, w in zip(self.voxels, self.widths):
            self.offsets.append(at)
            at += n * w + (-(n * w) % 16)
        assert at == len(self.payload)
        self.ix = cir.index(cpr.pack(blob)) if route == "packed" and entries else None

    def codes(self, x, y, z):
        """-> (q, flagged) of the voxels (x, y, z), arrays: the signed code (kind 2: the stored bit pattern, uint64), 0 in a cell
        that is not flagged"""
        x, y, z = (np.asarray(a, np.int64) for a in (x, y, z))
        dx, dy, _ = self.dims
        cell = (x >> 4) + self.mc[0] * ((y >> 4) + self.mc[1] * (z >> 4))
        cx, cy = np.minimum(16, dx - (x & ~15)), np.minimum(16, dy - (y & ~15))
        if self.broken == "cx16":
            cx = np.full_like(cx, 16)
        li = (x & 15) + cx * ((y & 15) + cy * (z & 15))
        number = self.number[cell]
        flagged = number >= 0
        if self.broken == "neighbour-cell" and len(self.cells):                    # a clean cell borrows the flagged cell below it
            below = np.maximum(np.searchsorted(self.cells, cell, side="right") - 1, 0)
            number = np.where(flagged, number, below)
        q = np.zeros(x.shape, np.uint64 if self.kind == 2 else np.int64)
        for i in np.unique(number[number >= 0]):
            m = number == i
            at = li[m] % self.voxels[i]                                          # (only a broken index leaves the cell)
            if self.route == "fixed":
                w = self.widths[i]
                c = np.frombuffer(self.payload, ("<u%d" if self.kind == 2 else "<i%d") % w, self.voxels[i], self.offsets[i])[at]
                q[m] = c.astype(q.dtype)
            elif self.broken == "no-zigzag" and self.kind != 2:
                q[m] = (cir.code_at({**self.ix, "kind": 2}, i, at) >> cir.ONE).astype(np.int64)
            else:
                q[m] = cir.code_at(self.ix, i, at)
        return q, flagged if self.broken != "neighbour-cell" else number >= 0


def gather(src, dec_at, voxels):
    """what vnrAmdNeuralVolumeGatherVoxelsCorrected stores: dec_at[j] is the typed decode of voxel voxels[j] = (x, y, z)"""
    voxels = np.asarray(voxels, np.int64).reshape(-1, 3)
    dec_at = np.asarray(dec_at)
    assert dec_at.dtype == src.dtype and dec_at.shape == (len(voxels),)
    q, flagged = src.codes(voxels[:, 0], voxels[:, 1], voxels[:, 2])
    if src.kind == 2:
        return np.where(flagged, q.astype(ebr.bits(dec_at).dtype).view(src.dtype), dec_at)
    return np.where(flagged, ebr.corrected_value(dec_at, q, src.kind, src.step), dec_at)


def convert(src, v):
    """the network's value in the data units of the correction's range, float32, not rounded to an integer type"""
    v = np.asarray(v, F32)
    return (v * F32(src.hi - src.lo) + src.lo).astype(F32) if src.lo < src.hi else v


def axis_place(p, dim, broken=None):
    """-> (i0, i1, w float32, t float32 after the clamp)"""
    with np.errstate(invalid="ignore"):
        t = np.asarray(p, F32) * F32(dim) - F32(0.5)                               # two float32 roundings
        tc = np.where(t >= 0, t, F32(0))                                           # (a NaN lands here)
        tc = np.where(tc > F32(dim - 1), F32(dim - 1), tc).astype(F32)
        i0 = np.floor(tc).astype(np.int64)
        i1 = i0 + 1 if broken == "i1-unclamped" else np.minimum(i0 + 1, dim - 1)
        w = ((t if broken == "w-unclamped" else tc) - i0.astype(F32)).astype(F32)
    return i0, i1, w, tc


def residual(src, q):
    if src.kind == 0:
        qmax = 2 ** 34 // src.step + 1
        return (np.clip(q, -qmax, qmax) * src.step).astype(np.float64)
    return q.astype(np.float64) * np.array(src.step, np.uint64).view(np.float64)     # one rounding


def lerp(a, b, w):
    w = w.astype(np.float64)
    return a * (1.0 - w) + b * w                                                   # three roundings, never an fma


def corners(src, coords):
    """-> (codes [2 z][2 y][2 x] of arrays, (wx, wy, wz), the clamped (tx, ty, tz))"""
    coords = np.asarray(coords, F32).reshape(-1, 3)
    px, py, pz = (axis_place(coords[:, a], src.dims[a], src.broken) for a in range(3))
    dx, dy, dz = src.dims
    q = [[[None, None], [None, None]], [[None, None], [None, None]]]
    for c, zz in enumerate(pz[:2]):
        for b, yy in enumerate(py[:2]):
            for a, xx in enumerate(px[:2]):
                lin = (xx + dx * (yy + dy * zz)) % (dx * dy * dz)                  # (only an unclamped i1 leaves the grid: the next voxel in memory)
                q[c][b][a] = src.codes(lin % dx, lin // dx % dy, lin // (dx * dy))[0]
    return q, (px[2], py[2], pz[2]), (px[3], py[3], pz[3])


def sample(src, v, coords):
    """what vnrAmdNeuralVolumeSampleCorrected stores: v[j] is what vnrAmdNeuralVolumeInference gives at coords[j]"""
    assert src.kind != 2, "a verbatim correction is refused"
    d = convert(src, v)
    q, (wx, wy, wz), _ = corners(src, coords)
    with np.errstate(invalid="ignore", over="ignore"):
        rows = [[lerp(residual(src, q[c][b][0]), residual(src, q[c][b][1]), wx) for b in range(2)] for c in range(2)]
        blend = lerp(lerp(rows[0][0], rows[0][1], wy), lerp(rows[1][0], rows[1][1], wy), wz)
        any_code = np.zeros(d.shape, bool)
        for c in range(2):
            for b in range(2):
                for a in range(2):
                    any_code |= q[c][b][a] != 0
        return np.where(any_code, (d.astype(np.float64) + blend).astype(F32), d)


def centre_bound(src, v, coords):
    """the convex bound of the header at `coords` -> (d + residual(nearest voxel) in double, (delta_x + delta_y + delta_z) * (max - min
    of the eight residuals))"""
    d = convert(src, v).astype(np.float64)
    q, _, t = corners(src, coords)
    r = np.stack([residual(src, q[c][b][a]) for c in range(2) for b in range(2) for a in range(2)])
    near = [np.rint(ta.astype(np.float64)).astype(np.int64) for ta in t]
    delta = sum(np.abs(ta.astype(np.float64) - na) for ta, na in zip(t, near))
    return d + residual(src, src.codes(*near)[0]), delta * (r.max(axis=0) - r.min(axis=0))


# ------------------------------------------------------------------------------------------------ the point sets
def voxel_centres(dims, voxels=None):
    """the coordinates the decode evaluates: ((float)x + 0.5f) * (1.0f / (float)dim), of `voxels` (n, 3) or of the whole grid x fastest"""
    if voxels is None:
        z, y, x = np.meshgrid(*(np.arange(d) for d in dims[::-1]), indexing="ij")
        voxels = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    voxels = np.asarray(voxels)
    return np.stack([(voxels[:, a].astype(F32) + F32(0.5)) * (F32(1.0) / F32(dims[a])) for a in range(3)], axis=1).astype(F32)


def integral_coord(i, dim):
    """a float32 p whose t = p * dim - 0.5 is exactly i"""
    p = F32((i + 0.5) / dim)
    for c in (p, np.nextafter(p, F32(0)), np.nextafter(p, F32(2))):
        if F32(c * F32(dim)) - F32(0.5) == F32(i):
            return c
    raise AssertionError((i, dim))


def uniform_points(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)).astype(F32)


def axis_edges(dim):
    """one axis: both ends, the last float below 1, points within half a voxel of both faces, and points whose t lies strictly between
    15 and 16 and between 31 and 32 (cell boundaries) where the axis has them"""
    p = [0.0, 1.0, float(np.nextafter(F32(1), F32(0))), 0.2 / dim, 0.5 / dim, 1.0 - 0.3 / dim, (dim - 1 + 0.1) / dim, 1.3 / dim]
    p += [(b + 0.5 + f) / dim for b in (15, 31) if b + 1 < dim for f in (0.25, 0.75)]
    return np.array(p, F32)


def edge_points(dims):
    """the product of the axes' edges, and on every row of the grid one point between x = 3 and 4 of each cell (in a cell with
    cx = 5 such pairs of codes wrap a group)"""
    ex, ey, ez = (axis_edges(d) for d in dims)
    z, y, x = np.meshgrid(ez, ey, ex, indexing="ij")
    product = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    xs = np.array([(x0 + 3 + 0.5 + 0.4) / dims[0] for x0 in range(0, dims[0], 16) if x0 + 4 < dims[0]], F32)
    z, y, x = np.meshgrid((np.arange(dims[2]) + 0.75) / dims[2], (np.arange(dims[1]) + 0.75) / dims[1], xs, indexing="ij")
    rows = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    return np.concatenate([product, rows]).astype(F32)
