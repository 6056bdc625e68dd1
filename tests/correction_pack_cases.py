"""Seeded fixed-width ("VNRCORR1") corrections for the packed-form tests, host and GPU: built by error_bound_ref.build from random
arrays whose residuals are shaped so that, per volume, cells of every code width, groups of zeros and clean cells occur; and blobs
crafted code by code for the edges of a group's bit width."""
import functools
import struct

import numpy as np

import error_bound_ref as ebr

DIMS = [(40, 24, 20), (17, 16, 33), (5, 3, 2)]       # (17, 16, 33): cells of 256 and of 16 voxels; (5, 3, 2): one group, 34 idle lanes
# (dtype, eps): kind 0 with codes of 1, 2 and 4 bytes, kind 0 of a narrow type, kind 1 of both float types, kind 2 of both
TYPES = [(np.int32, 1), (np.int16, 2), (np.float32, 1e-3), (np.float64, 1e-4), (np.float32, 0), (np.float64, 0)]
CASES = [(t, e, d) for t, e in TYPES for d in DIMS]
IDS = [f"{t.__name__}-{e}-{d[0]}x{d[1]}x{d[2]}" for t, e, d in CASES]


def fields(dtype, dims, eps, seed):
    """dec / ref [z, y, x] whose codes q are: x < 16 a few of -3 .. 3 among zeros (none at all from z = 16 on: clean cells),
    16 <= x < 32 thousands (2-byte codes), x >= 32 millions (4-byte codes; hundreds for a 16-bit type)"""
    rng = np.random.default_rng(seed)
    shape = dims[::-1]
    dt = np.dtype(dtype)
    x = np.arange(dims[0])
    wide = dt.itemsize > 2                           # (a 16-bit type holds no residual beyond its range)
    scale = np.where(x < 16, 1.0, np.where(x < 32, 6000.0 if wide else 1000.0, 3.0e6 if wide else 300.0))
    q = np.rint(rng.normal(0.0, 1.0, shape) * scale).astype(np.int64)
    q[:, :, :16] *= rng.uniform(size=shape)[:, :, :16] < 0.03
    q[16:, :, :16] = 0
    q[0, 0, 0] = -1
    if dt.kind == "f":
        dec = rng.uniform(-2.0, 5.0, shape).astype(dtype)
        ref = (dec.astype(np.float64) + q * (2.0 * eps if eps > 0 else 1.0e-3)).astype(dtype)
    else:
        dec = rng.integers(-1000, 1000, shape).astype(dtype)
        ref = (dec.astype(np.int64) + q * (2 * int(eps) + 1)).astype(dtype)
    return dec, ref


@functools.lru_cache(maxsize=None)
def case(dtype, eps, dims):
    """-> error_bound_ref.build's dict; ["bytes"] is the fixed-width blob"""
    dec, ref = fields(dtype, dims, eps, seed=dims[0] * 131 + np.dtype(dtype).itemsize)
    return ebr.build(dec, ref, eps, (-3.0, 9.5), params_hash=0x0123456789abcdef, n_params=4242)


@functools.lru_cache(maxsize=None)
def many_cells():
    """about 300 flagged cells of an int16 field: 8 x 8 x 5 cells, a few of them clean"""
    dims = (128, 120, 70)
    rng = np.random.default_rng(5)
    shape = dims[::-1]
    dec = rng.integers(-1000, 1000, shape).astype(np.int16)
    q = np.rint(rng.normal(0.0, 1.0, shape) * rng.choice([0.15, 30.0, 900.0], (5, 8, 8)).repeat(16, 0).repeat(16, 1).repeat(16, 2)[:70, :120, :128]).astype(np.int64)
    q[:, :32, :48] = 0
    return ebr.build(dec, (dec + 5 * q).astype(np.int16), 2, (0.0, 1.0))


CRAFTED = [(np.int16, 5.0, 1), (np.int16, 5.0, 2), (np.int32, 1.0, 4), (np.float32, 1e-3, 1), (np.float32, 0, 4), (np.float64, 0, 8)]


@functools.lru_cache(maxsize=None)
def crafted(dtype, eps, width):
    """-> (fixed-width blob of one cell of 16 x 16 x 2 voxels = 8 groups, nbits of its groups): a group of zeros, one of 0 and -1
    (kind 2: the pattern 1), the most negative and the largest code of the width (kind 2: the top bit alone, all ones), small codes"""
    kind = ebr.kind_of(dtype, eps)
    rng = np.random.default_rng(width)
    bits = 8 * width
    if kind == 2:
        codes = np.zeros(512, "<u%d" % width)
        codes[64:128:3] = 1
        codes[130] = 1 << (bits - 1)
        codes[200] = (1 << bits) - 1
        codes[256:320] = rng.integers(0, 6, 64)          # z up to 5: 3 bits
        codes[256] = 5
    else:
        codes = np.zeros(512, "<i%d" % width)
        codes[64:128:3] = -1                             # z = 1
        codes[130] = -(1 << (bits - 1))                  # z = 2^bits - 1
        codes[200] = (1 << (bits - 1)) - 1               # z = 2^bits - 2
        codes[256:320] = rng.integers(-2, 3, 64)         # z up to 4: 3 bits
        codes[256] = 2
    payload = codes.tobytes()
    header = ebr.HEADER.pack(b"VNRCORR1", 1, ebr.VALUE_TYPES[np.dtype(dtype)], 16, 16, 2, 1, float(eps), 0.0, 1.0, kind, 0, ebr.step_of(kind, eps), 7, 9,
                             len(payload), 0.25, 0)
    return header + struct.pack("<II", 0, width) + payload, [0, 1, bits, bits, 3, 0, 0, 0]
