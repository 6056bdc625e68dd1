"""numpy restatement of the error-bounded round trip (include/vnr_amd.h, "error-bounded round trip"): the quantiser, the per-cell
code widths, the serialised bytes, the apply (from the bytes alone) and the FNV-1a hash.  Arrays are [z, y, x] of the value type.
The device code (csrc/correction.hip) and the host reader / writer (csrc/correction_format.cpp) are held to this with tolerance zero."""
import struct

import numpy as np

VALUE_TYPES = {np.dtype(np.uint8): 0, np.dtype(np.int8): 1, np.dtype(np.uint16): 2, np.dtype(np.int16): 3,
               np.dtype(np.uint32): 4, np.dtype(np.int32): 5, np.dtype(np.float32): 8, np.dtype(np.float64): 12}
DTYPES = {v: k for k, v in VALUE_TYPES.items()}
HEADER = struct.Struct("<8sIIiiiIdffIIQQQQdQ")
assert HEADER.size == 104
MAX_INTEGER_EPS = 2.0 ** 40


def fnv1a64(b):
    h = 0xcbf29ce484222325
    for x in bytes(b):
        h = ((h ^ x) * 0x100000001b3) & 0xffffffffffffffff
    return h


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def kind_of(dtype, eps):
    return 0 if np.dtype(dtype).kind != "f" else (1 if eps > 0 else 2)


def step_of(kind, eps):
    if kind == 0:
        return 2 * int(np.floor(min(eps, MAX_INTEGER_EPS))) + 1
    if kind == 1:
        return int(np.float64(2.0 * eps).view(np.uint64))
    return 0


def quantise(dec, ref, eps):
    """-> (q int64 (kind 2: 1 where the bit patterns differ), NaN mask)"""
    kind = kind_of(dec.dtype, eps)
    if kind == 0:
        E = int(np.floor(min(eps, MAX_INTEGER_EPS)))
        r = ref.astype(np.int64) - dec.astype(np.int64)
        return np.floor_divide(r + E, 2 * E + 1), np.zeros(dec.shape, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        r = ref.astype(np.float64) - dec.astype(np.float64)
        nan = np.isnan(r)
        if kind == 2:
            return (bits(dec) != bits(ref)).astype(np.int64).reshape(dec.shape), nan
        qd = np.rint(np.where(nan, 0.0, r) / np.float64(2.0 * eps))
        if np.abs(qd).max() > 2 ** 31 - 1:
            raise ValueError("the tolerance needs codes wider than 32 bits")
        return qd.astype(np.int64), nan


def corrected_value(dec, q, kind, step):
    """what the apply stores for voxels of a flagged cell with the codes q (kinds 0 and 1)"""
    if kind == 0:
        info = np.iinfo(dec.dtype)
        qmax = 2 ** 34 // step + 1      # beyond it every type saturates: the clamp keeps q * s inside int64 and changes nothing
        return np.clip(dec.astype(np.int64) + np.clip(q, -qmax, qmax) * step, info.min, info.max).astype(dec.dtype)
    s = np.array(step, np.uint64).view(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = q.astype(np.float64) * s                     # one rounding
        cd = dec.astype(np.float64) + prod                  # one rounding, never an fma
        return np.where(q == 0, dec, cd.astype(dec.dtype))


def cells_of(dims):
    """yields (cell index, slices [z, y, x]) in ascending cell index"""
    m = [-(-d // 16) for d in dims]
    for iz in range(m[2]):
        for iy in range(m[1]):
            for ix in range(m[0]):
                yield ix + m[0] * (iy + m[1] * iz), (slice(16 * iz, 16 * iz + 16), slice(16 * iy, 16 * iy + 16), slice(16 * ix, 16 * ix + 16))


def max_and_first(a):
    """max of |.| and its first x-fastest index as (x, y, z); a NaN never wins -> (NaN, (-1, -1, -1)) if nothing else is there"""
    a = np.where(np.isnan(a), -1.0, a)
    k = int(np.argmax(a))
    if a.ravel()[k] < 0:
        return float("nan"), (-1, -1, -1)
    z, y, x = np.unravel_index(k, a.shape)
    return float(a.ravel()[k]), (int(x), int(y), int(z))


def build(dec, ref, eps, value_range, params_hash=0, n_params=0):
    """-> dict: bytes (the serialised correction), corrected, cells [(cell, width)], and the fields of the build's report"""
    assert dec.dtype == ref.dtype and dec.shape == ref.shape
    dims = dec.shape[::-1]
    dt = dec.dtype
    kind = kind_of(dt, eps)
    step = step_of(kind, eps)
    q, nan = quantise(dec, ref, eps)
    corrected = dec.copy()
    cells, payload = [], []
    for cell, sl in cells_of(dims):
        qc = q[sl]
        m = int(np.abs(qc).max())
        if m == 0:
            continue
        if m > 2 ** 31 - 1:
            raise ValueError("the tolerance needs codes wider than 32 bits")
        if kind == 2:
            width, codes = dt.itemsize, bits(ref[sl]).astype("<u4" if dt.itemsize == 4 else "<u8").tobytes()
            corrected[sl] = ref[sl]
        else:
            width = 1 if m <= 127 else (2 if m <= 32767 else 4)
            codes = qc.astype({1: "<i1", 2: "<i2", 4: "<i4"}[width]).tobytes()      # C order of [z, y, x]: lx + cx (ly + cy lz)
            corrected[sl] = corrected_value(dec[sl], qc, kind, step)
        cells.append((cell, width))
        payload.append(codes + b"\0" * (-len(codes) % 16))
    payload = b"".join(payload)
    with np.errstate(invalid="ignore", over="ignore"):
        before, _ = max_and_first(np.abs(dec.astype(np.float64) - ref.astype(np.float64)))
        after, worst = max_and_first(np.abs(corrected.astype(np.float64) - ref.astype(np.float64)))
    lo, hi = value_range if value_range is not None else (1.0, 0.0)
    header = HEADER.pack(b"VNRCORR1", 1, VALUE_TYPES[dt], dims[0], dims[1], dims[2], len(cells), float(eps), lo, hi, kind, 0, step, params_hash, n_params,
                         len(payload), after, 0)
    entries = b"".join(struct.pack("<II", c, w) for c, w in cells)
    return {"bytes": header + entries + payload, "corrected": corrected, "cells": cells, "q": q, "kind": kind, "n_flagged": len(cells),
            "n_voxels_flagged": int((q != 0).sum()), "n_nan": int(nan.sum()), "max_abs_before": before, "max_abs_after": after, "worst_after": worst,
            "payload_bytes": len(payload)}


def apply(dec, blob):
    """the corrected array from the decoded one and the serialised bytes alone"""
    f = HEADER.unpack_from(blob, 0)
    assert f[0] == b"VNRCORR1" and f[1] == 1
    dt, dims, n_flagged, kind, step = DTYPES[f[2]], f[3:6], f[6], f[10], f[12]
    assert dec.dtype == dt and dec.shape == tuple(dims[::-1])
    table = dict(struct.unpack_from("<II", blob, HEADER.size + 8 * i) for i in range(n_flagged))
    at = HEADER.size + 8 * n_flagged
    out = dec.copy()
    for cell, sl in cells_of(dims):
        if cell not in table:
            continue
        width, shape = table[cell], dec[sl].shape
        n = shape[0] * shape[1] * shape[2]
        if kind == 2:
            out[sl] = np.frombuffer(blob, "<u4" if width == 4 else "<u8", n, at).view(dt).reshape(shape)
        else:
            q = np.frombuffer(blob, {1: "<i1", 2: "<i2", 4: "<i4"}[width], n, at).astype(np.int64).reshape(shape)
            out[sl] = corrected_value(dec[sl], q, kind, step)
        at += n * width + (-(n * width) % 16)
    assert at == len(blob)
    return out


def float_bound(corrected, ref, dec, eps):
    """eps + 2^-50 (|ref| + |dec| + eps) + ulp_T(corrected) / 2, per voxel, in double"""
    f = lambda a: np.abs(a.astype(np.float64))
    return eps + 2.0 ** -50 * (f(ref) + f(dec) + eps) + np.spacing(np.abs(corrected)).astype(np.float64) / 2
