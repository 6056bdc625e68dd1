"""numpy restatement of "corrections to a byte budget" (include/vnr_amd.h): rates() gives, for a list of tolerances, the counts and
the sizes in both serialised forms that a build would report, computed from the codes q directly (no byte of either form is made);
budget_search() is the search of the build within a byte budget, every step one IEEE double operation.  The device pass
(csrc/correction.hip) and the host search (csrc/correction_budget.cpp) are held to this with tolerance zero."""
import math

import numpy as np

import error_bound_ref as ebr

FIELDS = ("n_flagged", "n_voxels_flagged", "n_groups", "payload_bytes", "serialized_bytes", "packed_payload_bytes", "packed_serialized_bytes")


def rate(dec, ref, eps):
    """one entry of vnrAmdCorrectionRate as a dict; arrays are [z, y, x]"""
    kind = ebr.kind_of(dec.dtype, eps)
    out = {"eps": float(eps), "kind": kind, "refused": False, **{k: 0 for k in FIELDS}}
    try:
        q, _ = ebr.quantise(dec, ref, eps)
    except ValueError:                                   # a float code beyond 32 bits somewhere
        out["refused"] = True
        return out
    n_flagged = n_groups = payload = nbits = 0
    for _, sl in ebr.cells_of(dec.shape[::-1]):
        qc = q[sl].ravel()                               # C order of [z, y, x]: lx + cx (ly + cy lz)
        m = int(np.abs(qc).max())
        if m == 0:
            continue
        if m > 2 ** 31 - 1:
            out["refused"] = True
            return out
        width = dec.dtype.itemsize if kind == 2 else (1 if m <= 127 else (2 if m <= 32767 else 4))
        if kind == 2:
            z = ebr.bits(ref[sl]).ravel().astype(np.uint64)
        else:
            z = ((qc << 1) ^ (qc >> 63)).view(np.uint64)
        groups = -(-qc.size // 64)
        z = np.concatenate([z, np.zeros(groups * 64 - qc.size, np.uint64)]).reshape(groups, 64)
        n_flagged += 1
        n_groups += groups
        payload += qc.size * width + (-(qc.size * width) % 16)
        nbits += sum(int(g).bit_length() for g in z.max(axis=1))
    packed = n_groups + (-n_groups % 8) + 8 * nbits
    out.update(n_flagged=n_flagged, n_voxels_flagged=int((q != 0).sum()), n_groups=n_groups, payload_bytes=payload,
               serialized_bytes=104 + 8 * n_flagged + payload, packed_payload_bytes=packed, packed_serialized_bytes=104 + 8 * n_flagged + packed)
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


def budget_search(size_of, max_bytes, eps_hi, rounds):
    """size_of(list of tolerances) -> their serialised sizes, None where the build is refused.
    -> dict(eps, bytes, eps_tighter, bytes_tighter, rate_passes); ValueError where eps_hi itself does not fit"""
    eps_hi = float(eps_hi)
    assert math.isfinite(eps_hi) and eps_hi > 0 and math.ldexp(eps_hi, -15) >= 2.0 ** -1022 and 0 <= rounds <= 8
    r = {"eps_tighter": float("nan"), "bytes_tighter": 0, "rate_passes": 0}

    def probe(points):
        sizes = list(size_of(list(points)))
        assert len(sizes) == len(points)
        r["rate_passes"] += 1
        fits = [s is not None and s <= max_bytes for s in sizes]
        for e, s, f in zip(points, sizes, fits):
            if not f and not e <= r["eps_tighter"]:
                r["eps_tighter"], r["bytes_tighter"] = e, (0 if s is None else s)
        return sizes, fits

    t = [math.ldexp(eps_hi, -j) for j in range(16)]
    sizes, fits = probe(t)
    if not fits[0]:
        raise ValueError(f"the correction does not fit max_bytes {max_bytes} at eps_hi {eps_hi!r}: its size there is {sizes[0]}")
    J = 0
    while J + 1 < 16 and fits[J + 1]:
        J += 1
    hi, hi_bytes = t[J], sizes[J]
    if J < 15:
        lo = t[J + 1]
        for _ in range(rounds):
            p = [lo + (hi - lo) * (i / 16) for i in range(1, 16)]      # Python floats: IEEE doubles, one rounding an operation
            sizes, fits = probe(p)
            i_first = 16                                                # the smallest i with every p_i', i' >= i, fitting; 16: none
            while i_first > 1 and fits[i_first - 2]:
                i_first -= 1
            if i_first == 16:
                lo = p[14]
                continue
            hi, hi_bytes = p[i_first - 1], sizes[i_first - 1]
            if i_first > 1:
                lo = p[i_first - 2]
    r.update(eps=hi, bytes=hi_bytes)
    return r
