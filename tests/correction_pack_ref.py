"""numpy restatement of the packed form of a correction (include/vnr_amd.h, "packed corrections") on top of error_bound_ref.py:
pack() turns serialised "VNRCORR1" bytes into "VNRCORP1" bytes, unpack() turns them back.  The device code
(csrc/correction_pack.hip) and the host reader, writer and unpack (csrc/correction_packed_format.cpp) are held to this byte for byte."""
import struct

import numpy as np

import error_bound_ref as ebr

HEADER = ebr.HEADER
CODE = {1: "<i1", 2: "<i2", 4: "<i4", 8: "<i8"}
LANES = np.arange(64, dtype=np.uint64)
ONE = np.uint64(1)


def split(blob, magic):
    """-> (header fields as a list, [(cell, width)], payload)"""
    f = list(HEADER.unpack_from(blob, 0))
    assert f[0] == magic and f[1] == 1
    n = f[6]
    cells = [struct.unpack_from("<II", blob, HEADER.size + 8 * i) for i in range(n)]
    payload = blob[HEADER.size + 8 * n:]
    assert len(payload) == f[15]
    return f, cells, payload


def join(f, magic, cells, payload):
    f = list(f)
    f[0], f[15] = magic, len(payload)
    return HEADER.pack(*f) + b"".join(struct.pack("<II", c, w) for c, w in cells) + payload


def cell_voxels(dims, cell):
    m = [-(-d // 16) for d in dims]
    i = (cell % m[0], cell // m[0] % m[1], cell // (m[0] * m[1]))
    return int(np.prod([min(16, d - 16 * k) for d, k in zip(dims, i)]))


def pack(v1):
    f, cells, payload = split(v1, b"VNRCORR1")
    dims, kind = f[3:6], f[10]
    table, planes, at = [], [], 0
    for cell, width in cells:
        n = cell_voxels(dims, cell)
        q = np.frombuffer(payload, CODE[width], n, at)
        at += n * width + (-(n * width) % 16)
        if kind == 2:
            z = q.view("<u%d" % width).astype(np.uint64)                      # the bit pattern, zero-extended
        else:
            q = q.astype(np.int64)
            z = ((q << 1) ^ (q >> 63)).view(np.uint64)
        z = np.concatenate([z, np.zeros(-n % 64, np.uint64)]).reshape(-1, 64)   # groups of 64, the last filled up with zeros
        for group in z:
            nbits = int(group.max()).bit_length()
            table.append(nbits)
            b = np.arange(nbits, dtype=np.uint64)[:, None]
            planes.append(np.bitwise_or.reduce(((group[None, :] >> b) & ONE) << LANES[None, :], axis=1, initial=np.uint64(0)))   # word b: bit l = bit b of z[l]
    assert at == len(payload)
    packed = bytes(table) + b"\0" * (-len(table) % 8) + np.concatenate(planes + [np.zeros(0, np.uint64)]).astype("<u8").tobytes()
    return join(f, b"VNRCORP1", cells, packed)


def unpack(packed):
    f, cells, payload = split(packed, b"VNRCORP1")
    dims, kind = f[3:6], f[10]
    groups = [-(-cell_voxels(dims, cell) // 64) for cell, _ in cells]
    n_groups = sum(groups)
    table = payload[:n_groups]
    at = n_groups + (-n_groups % 8)
    assert not any(payload[n_groups:at])
    out, g = [], 0
    for (cell, width), ng in zip(cells, groups):
        n = cell_voxels(dims, cell)
        z = np.zeros((ng, 64), np.uint64)
        for k in range(ng):
            words = np.frombuffer(payload, "<u8", table[g], at).astype(np.uint64)
            at += 8 * table[g]
            g += 1
            b = np.arange(len(words), dtype=np.uint64)[:, None]
            z[k] = np.bitwise_or.reduce(((words[:, None] >> LANES[None, :]) & ONE) << b, axis=0, initial=np.uint64(0))
        z = z.ravel()
        assert not z[n:].any()
        z = z[:n]
        if kind == 2:
            codes = z.astype("<u%d" % width).tobytes()
        else:
            q = (z >> ONE).view(np.int64) ^ -(z & ONE).view(np.int64)
            assert (q >= -(1 << (8 * width - 1))).all() and (q < (1 << (8 * width - 1))).all()
            codes = q.astype(CODE[width]).tobytes()
        out.append(codes + b"\0" * (-len(codes) % 16))
    assert at == len(payload)
    return join(f, b"VNRCORR1", cells, b"".join(out))
