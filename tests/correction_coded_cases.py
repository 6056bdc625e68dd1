"""Fixed-width ("VNRCORR1") corrections for the coded-form tests, host and GPU: every blob of correction_pack_cases.py, blobs crafted
code by code for the edges of the coded form (tests/correction_coded_ref.py), and a field of Gaussian residuals of sigma = eps."""
import functools
import struct

import numpy as np

import correction_pack_cases as cases
import error_bound_ref as ebr


def one_cell(dtype, eps, width, dims, codes):
    """-> the fixed-width blob of a volume of one cell (dims at most 16 each) whose codes are `codes` (signed; kind 2: the patterns)"""
    kind = ebr.kind_of(dtype, eps)
    n = dims[0] * dims[1] * dims[2]
    assert max(dims) <= 16 and len(codes) == n
    payload = np.asarray(codes, "<u%d" % width if kind == 2 else "<i%d" % width).tobytes()
    payload += b"\0" * (-len(payload) % 16)
    header = ebr.HEADER.pack(b"VNRCORR1", 1, ebr.VALUE_TYPES[np.dtype(dtype)], *dims, 1, float(eps), 0.0, 1.0, kind, 0, ebr.step_of(kind, eps), 7, 9,
                             len(payload), 0.25, 0)
    return header + struct.pack("<II", 0, width) + payload


def plane_counts():
    """16 x 16 x 2 = 8 groups of 4-byte codes.  Group 0: plane 2 with 1 bit set, plane 1 with 9 (the longest list), plane 0 with 10
    (the shortest dense plane).  Group 1: one code of 4, so planes 1 and 0 are lists of nothing.  Group 2 is zeros between groups 1
    and 3.  Group 3: -2^31 (mbits 32, legal only with its sign) beside 2^31 - 1.  The rest zeros."""
    q = np.zeros(512, np.int64)
    q[0:10] = [1, -1, 1, 1, -1, 1, 1, 1, -1, 1]
    q[10:19] = [2, -2, 2, 2, 2, -2, 2, 2, 2]
    q[20] = -4
    q[64 + 37] = 4
    q[192 + 5] = -(1 << 31)
    q[192 + 63] = (1 << 31) - 1
    return one_cell(np.int32, 1.0, 4, (16, 16, 2), q)


def pattern64():
    """kind 2, float64: a group with a 64-bit pattern (mbits 64: the top bit alone, all ones, a few small ones), a group of zeros, a group of ones"""
    u = np.zeros(256, np.uint64)
    u[3] = 1 << 63
    u[40] = (1 << 64) - 1
    u[41:60] = np.arange(1, 20)
    u[128:192] = 1
    return one_cell(np.float64, 0, 8, (16, 8, 2), u)


def idle_lanes():
    """the (5, 3, 2) volume: one group of 30 codes, 34 idle lanes; 1-byte codes with both extremes"""
    q = np.zeros(30, np.int64)
    q[[0, 7, 29]] = [-128, 127, -1]
    return one_cell(np.int16, 5.0, 1, (5, 3, 2), q)


def sixteen_voxels():
    """a cell of 16 voxels: one group, 48 idle lanes, every lane that has a voxel non-zero"""
    return one_cell(np.int16, 5.0, 2, (1, 16, 1), np.arange(16) * 1000 - 8000 + 1)


def longest(verbatim):
    """one full 16^3 cell of 64 groups at the greatest mbits with every plane dense and every lane non-zero, the longest stream
    there is: width 4, 64 * (7 + 32 * 65 + 64) bits = 2151 words; float64 verbatim, 64 * (7 + 64 * 65) bits = 4167 words"""
    if verbatim:
        return one_cell(np.float64, 0, 8, (16, 16, 16), np.full(4096, (1 << 64) - 1, np.uint64))
    q = np.where(np.arange(4096) % 64 < 32, -(1 << 31), (1 << 31) - 1)          # bit 31 alone in 32 lanes, bits 0 .. 30 in the other 32
    q[1::2] = np.where(q[1::2] > 0, -q[1::2], q[1::2])                          # (signs of both kinds)
    return one_cell(np.int32, 1.0, 4, (16, 16, 16), q)


LONGEST_WORDS = {False: 2151, True: 4167}


@functools.lru_cache(maxsize=None)
def gaussian(eps=0.01):
    """float32, 64 x 64 x 32 (32 cells): residuals that are seeded Gaussian noise of sigma = eps"""
    rng = np.random.default_rng(2026)
    dec = rng.uniform(0.0, 1.0, (32, 64, 64)).astype(np.float32)
    ref = (dec.astype(np.float64) + rng.normal(0.0, eps, dec.shape)).astype(np.float32)
    return ebr.build(dec, ref, eps, (0.0, 1.0))


@functools.lru_cache(maxsize=None)
def crafted():
    """(name, fixed-width bytes) of the blobs made here for the edges of the coded form"""
    return [("plane-counts", plane_counts()), ("pattern64", pattern64()), ("idle-lanes", idle_lanes()), ("sixteen-voxels", sixteen_voxels()),
            ("longest-w4", longest(False)), ("longest-f64", longest(True))]


@functools.lru_cache(maxsize=None)
def all_blobs():
    """(name, fixed-width bytes): the packed tests' built and crafted blobs, the ones crafted here, many_cells() and the Gaussian field"""
    out = [(i, cases.case(*c)["bytes"]) for i, c in zip(cases.IDS, cases.CASES)]
    out += [(f"crafted-{t.__name__}-{e}-w{w}", cases.crafted(t, e, w)[0]) for t, e, w in cases.CRAFTED]
    return out + list(crafted()) + [("many-cells", cases.many_cells()["bytes"]), ("gaussian", gaussian()["bytes"])]
