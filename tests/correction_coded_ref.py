"""numpy restatement of the coded form of a correction (include/vnr_amd.h, "coded corrections") on top of correction_pack_ref.py:
encode() turns serialised "VNRCORR1" bytes into "VNRCORC1" bytes, decode() turns them back.  The host reader, writer and transcoders
(csrc/correction_coded_format.cpp) and the device code (csrc/correction_code.hip) are held to this byte for byte.

A cell's stream is a run of u64 words, stream bit i = bit i % 64 of word i / 64, fields appended least significant bit first; here a
stream is one Python integer, which is the same thing."""
import struct

import numpy as np

import correction_pack_ref as cpr

MAGIC = b"VNRCORC1"
CODE = cpr.CODE
LANES = cpr.LANES
ONE = cpr.ONE
LIST_MAX = 9                                             # a list costs 5 + 6 c bits against 65: 9 is the largest count that pays


def split(blob, magic=MAGIC):
    """-> (header fields as a list, [(cell, width)], payload)"""
    return cpr.split(blob, magic)


def magnitudes(payload, at, n, width, kind):
    """-> (m [groups, 64] uint64, s [groups, 64] bool or None) of the n codes of a cell at byte `at`"""
    q = np.frombuffer(payload, CODE[width], n, at)
    if kind == 2:
        m, s = q.view("<u%d" % width).astype(np.uint64), None
    else:
        q = q.astype(np.int64)
        m, s = np.abs(q).view(np.uint64), q < 0          # (|-2^31| fits 64 bits)
        s = np.concatenate([s, np.zeros(-n % 64, bool)]).reshape(-1, 64)
    return np.concatenate([m, np.zeros(-n % 64, np.uint64)]).reshape(-1, 64), s


def group_record(m, s):
    """-> (the record of one group as an integer, its bits)"""
    mbits = int(m.max()).bit_length()
    acc, pos = mbits, 7
    if mbits == 0:
        return acc, pos
    b = np.arange(mbits, dtype=np.uint64)[:, None]
    planes = np.bitwise_or.reduce(((m[None, :] >> b) & ONE) << LANES[None, :], axis=1)
    for plane in planes[::-1]:
        plane = int(plane)
        c = bin(plane).count("1")
        if c <= LIST_MAX:
            acc |= (1 | c << 1) << pos
            pos += 5
            for lane in range(64):
                if plane >> lane & 1:
                    acc |= lane << pos
                    pos += 6
        else:
            acc |= plane << (pos + 1)
            pos += 65
    if s is not None:
        for lane in np.flatnonzero(m):
            acc |= int(s[lane]) << pos
            pos += 1
    return acc, pos


def encode(v1):
    f, cells, payload = cpr.split(v1, b"VNRCORR1")
    dims, kind = f[3:6], f[10]
    table, streams, at = [], [], 0
    for cell, width in cells:
        n = cpr.cell_voxels(dims, cell)
        m, s = magnitudes(payload, at, n, width, kind)
        at += n * width + (-(n * width) % 16)
        acc, pos = 0, 0
        for g in range(len(m)):
            r, bits = group_record(m[g], None if s is None else s[g])
            acc |= r << pos
            pos += bits
        words = -(-pos // 64)
        table.append(words)
        streams.append(acc.to_bytes(8 * words, "little"))
    assert at == len(payload)
    head = struct.pack("<%dI" % len(table), *table)
    return cpr.join(f, MAGIC, cells, head + b"\0" * (-len(head) % 8) + b"".join(streams))


def decode(coded):
    f, cells, payload = split(coded)
    dims, kind = f[3:6], f[10]
    n_cells = len(cells)
    table = struct.unpack_from("<%dI" % n_cells, payload, 0)
    at = 4 * n_cells + (-(4 * n_cells) % 8)
    assert not any(payload[4 * n_cells:at])
    out = []
    for (cell, width), words in zip(cells, table):
        n = cpr.cell_voxels(dims, cell)
        acc = int.from_bytes(payload[at:at + 8 * words], "little")
        assert len(payload) >= at + 8 * words
        at += 8 * words
        pos = 0
        q = np.zeros((-(-n // 64), 64), np.int64 if kind != 2 else np.uint64)
        for g in range(len(q)):
            mbits = acc >> pos & 127
            pos += 7
            assert mbits <= 8 * width
            m = [0] * 64
            for b in range(mbits - 1, -1, -1):
                if acc >> pos & 1:
                    c = acc >> (pos + 1) & 15
                    pos += 5
                    assert c <= LIST_MAX and (c > 0 or b < mbits - 1)
                    lanes = [acc >> (pos + 6 * j) & 63 for j in range(c)]
                    pos += 6 * c
                    assert all(x < y for x, y in zip(lanes, lanes[1:]))
                else:
                    plane = acc >> (pos + 1) & (1 << 64) - 1
                    pos += 65
                    lanes = [l for l in range(64) if plane >> l & 1]
                    assert len(lanes) > LIST_MAX
                for l in lanes:
                    m[l] |= 1 << b
            for l in range(64):
                if kind == 2:
                    q[g, l] = m[l]
                elif m[l]:
                    q[g, l] = -m[l] if acc >> pos & 1 else m[l]
                    pos += 1
        assert -(-pos // 64) == words and acc >> pos == 0
        q = q.ravel()
        assert not q[n:].any()
        if kind != 2:
            assert (q >= -(1 << (8 * width - 1))).all() and (q < (1 << (8 * width - 1))).all()
        codes = q[:n].astype(CODE[width] if kind != 2 else "<u%d" % width).tobytes()
        out.append(codes + b"\0" * (-len(codes) % 16))
    assert at == len(payload)
    return cpr.join(f, b"VNRCORR1", cells, b"".join(out))
