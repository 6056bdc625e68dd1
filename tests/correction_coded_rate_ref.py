"""numpy restatement of "byte budgets in the coded form" (include/vnr_amd.h): the size of the coded form ("VNRCORC1") of the correction
a tolerance would build, in closed form from the codes, without making a byte of it.  A record is 7 bits of mbits, then 5 + 6 c bits
for a plane with c <= 9 lanes set and 65 otherwise, then (kinds 0 and 1) a sign bit per code != 0; a cell's stream is its records
filled up to whole 64-bit words.  The codes, the counts and the refusal are correction_rate_ref.rate's and error_bound_ref.quantise's.
The device pass (correction_rate_coded_kernel in csrc/correction.hip) and the host function correction_coded_record_bits
(csrc/correction_coded_format.cpp) are held to this with tolerance zero, and this to what correction_coded_ref.encode really writes.

list_max, sign_every_lane and words_per_group exist for the tests alone: they break the closed form on purpose."""
import numpy as np

import correction_rate_ref as crr
import error_bound_ref as ebr

FIELDS = ("coded_stream_words", "coded_payload_bytes", "coded_serialized_bytes")
LIST_MAX = 9
ONE = np.uint64(1)


def group_bits(m, signed, list_max=LIST_MAX, sign_every_lane=False):
    """m [groups, 64] uint64, the magnitudes (kind 2: the patterns) -> the bits of every group's record, int64 [groups]"""
    mbits = np.array([int(t).bit_length() for t in m.max(axis=1)], np.int64)
    bits = np.full(len(m), 7, np.int64)
    for b in range(int(mbits.max(initial=0))):
        c = ((m >> np.uint64(b)) & ONE).sum(axis=1).astype(np.int64)
        bits += np.where(b < mbits, np.where(c <= list_max, 5 + 6 * c, 65), 0)
    if signed:
        bits += np.where(mbits > 0, 64, 0) if sign_every_lane else (m != 0).sum(axis=1)
    return bits


def cell_words(bits, words_per_group=False):
    """the 64-bit words of the stream of a cell whose records have `bits` bits"""
    if words_per_group:
        return int((-(-bits // 64)).sum())
    return -(-int(bits.sum()) // 64)


def flagged_cells(dec, ref, eps):
    """yields (cell, m [groups, 64] uint64, signed) for every flagged cell of the build at eps, in ascending cell index; lanes beyond
    the cell's voxels are 0.  The build must not be refused."""
    kind = ebr.kind_of(dec.dtype, eps)
    q, _ = ebr.quantise(dec, ref, eps)
    for cell, sl in ebr.cells_of(dec.shape[::-1]):
        qc = q[sl].ravel()                               # C order of [z, y, x]: lx + cx (ly + cy lz)
        if not qc.any():
            continue
        m = ebr.bits(ref[sl]).ravel().astype(np.uint64) if kind == 2 else np.abs(qc).astype(np.uint64)
        yield cell, np.concatenate([m, np.zeros(-qc.size % 64, np.uint64)]).reshape(-1, 64), kind != 2


def rate(dec, ref, eps, **broken):
    """one entry of vnrAmdCorrectionRateCoded as a flat dict: correction_rate_ref.rate's and the three coded fields"""
    out = crr.rate(dec, ref, eps)
    out.update({k: 0 for k in FIELDS})
    if out["refused"]:
        return out
    per_group = broken.pop("words_per_group", False)
    words = n = 0
    for _, m, signed in flagged_cells(dec, ref, eps):
        words += cell_words(group_bits(m, signed, **broken), per_group)
        n += 1
    assert n == out["n_flagged"]
    payload = 4 * n + (-4 * n % 8) + 8 * words
    out.update(coded_stream_words=words, coded_payload_bytes=payload, coded_serialized_bytes=104 + 8 * n + payload)
    return out


def rates(dec, ref, tolerances):
    """-> one dict a tolerance, in their order; equal tolerances are computed once"""
    done = {}
    out = []
    for eps in tolerances:
        key = float(eps)
        if key not in done:
            done[key] = rate(dec, ref, key)
        out.append(dict(done[key]))
    return out
