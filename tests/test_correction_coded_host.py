"""Coded corrections, the host side (include/vnr_amd.h, "coded corrections"): the numpy restatement of the format
(tests/correction_coded_ref.py) round-trips the fixed-width form, the library's coded reader, writer and transcoders
(csrc/correction_coded_format.cpp behind vnrAmdCreateCorrectionFromCodedBytes and vnrAmdCorrectionSerializeCoded, pure host code for a
correction that holds nothing on the device) agree with it byte for byte, every rule of the reader is broken once, the coded payload
is smaller than the packed one where it was built to be, and reader, transcoders and writer run under address / undefined-behaviour
sanitizers in a stand-alone program.  CPU only; every comparison has tolerance zero."""
import ctypes as C
import itertools
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from instantvnr_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import correction_coded_cases as ccc  # noqa: E402
import correction_coded_ref as ccr  # noqa: E402
import correction_pack_cases as cases  # noqa: E402
import correction_pack_ref as cpr  # noqa: E402
import error_bound_ref as ebr  # noqa: E402

BLOBS = ccc.all_blobs()
NAMES = [b[0] for b in BLOBS]
PREFIX = "malformed coded correction bytes: "


def payload_bytes(blob, magic):
    return cpr.split(blob, magic)[0][15]


def cell_table(coded):
    f, cells, payload = ccr.split(coded)
    return list(struct.unpack_from("<%dI" % len(cells), payload, 0))


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("name,v1", BLOBS, ids=NAMES)
def test_reference_round_trip(name, v1):
    coded = ccr.encode(v1)
    assert ccr.decode(coded) == v1
    f, cells, payload = ccr.split(coded)
    table = cell_table(coded)
    pad8 = 4 * len(cells) + (-4 * len(cells) % 8)
    assert len(payload) == pad8 + 8 * sum(table)
    widths = [w for _, w in cells]
    groups = [-(-cpr.cell_voxels(f[3:6], c) // 64) for c, _ in cells]
    # no stream is longer than all planes dense and every sign: 7 + 65 * 8 * width + 64 bits a group (kind 2: no signs)
    assert all(64 * t <= g * (7 + 65 * 8 * w + (64 if f[10] != 2 else 0)) + 63 for t, g, w in zip(table, groups, widths))


def test_the_crafted_blobs_are_the_edges_they_were_made_for():
    def records(v1):
        """-> per group of the one cell: (mbits, [count of plane mbits - 1 .. 0])"""
        f, cells, payload = cpr.split(v1, b"VNRCORR1")
        m, s = ccr.magnitudes(payload, 0, cpr.cell_voxels(f[3:6], 0), cells[0][1], f[10])
        out = []
        for g in m:
            mbits = int(g.max()).bit_length()
            out.append((mbits, [int(((g >> np.uint64(b)) & np.uint64(1)).sum()) for b in range(mbits - 1, -1, -1)]))
        return out

    r = records(ccc.plane_counts())
    assert r[0] == (3, [1, 9, 10]) and r[1] == (3, [1, 0, 0]) and r[2] == (0, []) and r[3][0] == 32 and r[3][1][0] == 1 and r[4] == (0, [])
    assert records(ccc.pattern64())[0][0] == 64 and records(ccc.pattern64())[1] == (0, []) and records(ccc.pattern64())[2] == (1, [64])
    assert len(records(ccc.idle_lanes())) == 1 and records(ccc.idle_lanes())[0][0] == 8
    assert len(records(ccc.sixteen_voxels())) == 1
    for verbatim in (False, True):
        r = records(ccc.longest(verbatim))
        assert len(r) == 64 and all(mbits == (64 if verbatim else 32) and min(counts) > ccr.LIST_MAX for mbits, counts in r)
        assert cell_table(ccr.encode(ccc.longest(verbatim))) == [ccc.LONGEST_WORDS[verbatim]]
    # q = -2^31 and 2^31 - 1 come back
    f, cells, payload = cpr.split(ccr.decode(ccr.encode(ccc.plane_counts())), b"VNRCORR1")
    q = np.frombuffer(payload, "<i4", 512)
    assert q[192 + 5] == -(1 << 31) and q[192 + 63] == (1 << 31) - 1


# ------------------------------------------------------------------------------------------------ the library on the host
def same_info(a, b):
    return all(v == b[k] or (isinstance(v, float) and math.isnan(v) and math.isnan(b[k])) for k, v in a.items()) and a.keys() == b.keys()


@pytest.mark.parametrize("name,v1", BLOBS, ids=NAMES)
def test_library_reads_transcodes_and_writes_what_numpy_codes(name, v1):
    coded, packed = ccr.encode(v1), cpr.pack(v1)
    c = api.Correction.from_coded_bytes(coded)
    assert c.to_coded_bytes() == coded                       # (before the host transcode, and after it)
    assert c.to_packed_bytes() == packed
    assert c.to_bytes() == v1
    assert c.to_coded_bytes() == coded
    assert not c.residency()["on_device"]                    # all of that on the host
    fixed, from_packed = api.Correction.from_bytes(v1), api.Correction.from_packed_bytes(packed)
    assert fixed.to_coded_bytes() == coded and from_packed.to_coded_bytes() == coded
    assert not fixed.residency()["on_device"] and not from_packed.residency()["on_device"]
    assert fixed.to_coded_device() == len(coded) == from_packed.to_coded_device() == c.to_coded_device()   # (the size alone)
    d = api.Correction.from_coded_bytes(coded)               # info() first: the transcode it triggers is the same
    assert same_info(d.info(), fixed.info()) and same_info(from_packed.info(), fixed.info()) and d.to_bytes() == v1
    assert d.info()["payload_bytes"] == payload_bytes(v1, b"VNRCORR1")
    for h in (c, d, fixed, from_packed):
        h.release()


def test_a_correction_without_a_flagged_cell_codes_on_the_host():
    dec = np.zeros((3, 4, 5), np.float32)
    v1 = ebr.build(dec, dec, 0.5, None)["bytes"]
    coded = ccr.encode(v1)
    assert len(coded) == ebr.HEADER.size and ccr.decode(coded) == v1
    assert api.Correction.from_bytes(v1).to_coded_bytes() == coded
    c = api.Correction.from_coded_bytes(coded)
    assert c.to_bytes() == v1 and c.to_packed_bytes() == cpr.pack(v1) and c.to_coded_bytes() == coded


def small_blobs():
    """(name, fixed-width bytes): the blobs crafted for the packed and the coded form, and a correction without a flagged cell"""
    dec = np.zeros((3, 4, 5), np.float32)
    out = [(f"crafted-{t.__name__}-{e}-w{w}", cases.crafted(t, e, w)[0]) for t, e, w in cases.CRAFTED] + ccc.crafted()
    return out + [("empty", ebr.build(dec, dec, 0.5, None)["bytes"])]


@pytest.mark.parametrize("name,v1", small_blobs(), ids=[b[0] for b in small_blobs()])
def test_every_order_of_the_serialisers_stays_on_the_host(name, v1):
    """a correction read from bytes and never applied answers every serialisation, every size query and info() without a device,
    whichever conversion comes first: each of the six orders on ONE object, whose caches fill up, and on a fresh one per order"""
    want = {"to_bytes": v1, "to_packed_bytes": cpr.pack(v1), "to_coded_bytes": ccr.encode(v1)}
    f, cells, _ = cpr.split(v1, b"VNRCORR1")
    info = api.Correction.from_bytes(v1).info()
    assert (info["payload_bytes"], info["serialized_bytes"], info["n_flagged"]) == (f[15], len(v1), len(cells))

    def run(c, order, sizes=("to_packed_device", "to_coded_device")):
        for call in order:
            assert getattr(c, call)() == want[call], (order, call)
            for size in sizes:
                assert getattr(c, size)() == len(want[size.replace("device", "bytes")]), (order, call, size)   # (None: the size alone)
            assert same_info(c.info(), info) and not c.residency()["on_device"], (order, call)

    for read, form in ((api.Correction.from_packed_bytes, "to_packed_bytes"), (api.Correction.from_coded_bytes, "to_coded_bytes")):
        one = read(want[form])
        for order in itertools.permutations(want):
            run(one, order)
            fresh = read(want[form])
            run(fresh, order)
            fresh.release()
        one.release()
    # read from fixed-width bytes: its packed form is the device pack's; everything else is the host's
    for order in itertools.permutations(("to_bytes", "to_coded_bytes")):
        c = api.Correction.from_bytes(v1)
        run(c, order, sizes=("to_coded_device",))
        c.release()


# ------------------------------------------------------------------------------------------------ the size statement
@pytest.mark.parametrize("name", ["many-cells", "gaussian"])
def test_the_coded_payload_is_smaller_than_the_packed_one(name):
    v1 = dict(BLOBS)[name]
    coded, packed = payload_bytes(ccr.encode(v1), ccr.MAGIC), payload_bytes(cpr.pack(v1), b"VNRCORP1")
    voxels = sum(cpr.cell_voxels(cpr.split(v1, b"VNRCORR1")[0][3:6], c) for c, _ in cpr.split(v1, b"VNRCORR1")[1])
    print(f"{name}: packed {packed} bytes = {8 * packed / voxels:.3f} bits a voxel of a flagged cell, coded {coded} bytes = {8 * coded / voxels:.3f}")
    assert coded < packed


# ------------------------------------------------------------------------------------------------ refusals
def patched(b, offset, fmt, value):
    return b[:offset] + struct.pack(fmt, value) + b[offset + struct.calcsize(fmt):]


def good():
    return ccr.encode(cases.case(np.int16, 2, (40, 24, 20))["bytes"])


def stream_of(fields, words=None):
    """[(value, bits)] -> the words of one cell's stream, filled up with zero bits (to `words` words if given)"""
    acc = pos = 0
    for v, n in fields:
        assert 0 <= v < 1 << n
        acc |= v << pos
        pos += n
    n = -(-pos // 64) if words is None else words
    return (acc & (1 << 64 * n) - 1).to_bytes(8 * n, "little")      # (a stream cut short on purpose loses its end)


def one_cell_coded(fields, dims=(16, 16, 1), width=1, words=None, table=None, pad=b"\0\0\0\0", groups_after=None):
    """the coded blob of a one-cell int16 volume whose stream is `fields` followed by a record of zeros for every other group"""
    head = ccc.one_cell(np.int16, 5.0, width, dims, np.zeros(dims[0] * dims[1] * dims[2], np.int64))
    f, cells, _ = cpr.split(head, b"VNRCORR1")
    n_groups = -(-dims[0] * dims[1] * dims[2] // 64)
    stream = stream_of(list(fields) + [(0, 7)] * (n_groups - 1 if groups_after is None else groups_after), words)
    return cpr.join(f, ccr.MAGIC, cells, struct.pack("<I", len(stream) // 8 if table is None else table) + pad + stream)


def lst(*lanes):
    """a plane stored as a list"""
    return [(1, 1), (len(lanes), 4)] + [(l, 6) for l in lanes]


ONE = [(1, 7)] + lst(3) + [(1, 1)]                           # one group: the code -1 in lane 3


def valid_crafted_streams():
    return [("one code", one_cell_coded(ONE)),
            ("the most negative code of the width", one_cell_coded([(8, 7)] + lst(0) + lst() * 7 + [(1, 1)])),
            ("a list of nine", one_cell_coded([(1, 7)] + lst(*range(0, 18, 2)) + [(0, 1)] * 9)),
            ("a dense plane of ten", one_cell_coded([(1, 7), (0, 1), (0x3ff, 64)] + [(1, 1)] * 10)),
            ("the last lane that has a voxel", one_cell_coded([(1, 7)] + lst(29) + [(0, 1)], dims=(5, 3, 2)))]


def broken_blobs():
    """(name, bytes, a word of the refusal): every rule of the coded reader broken once, everything else left valid"""
    g = good()
    f, cells, payload = ccr.split(g)
    n = len(cells)
    assert n >= 3
    e0 = ebr.HEADER.size
    cell = lambda i: cells[i][0]
    dbl = ccr.encode(cases.case(np.float64, 0, (40, 24, 20))["bytes"])
    flt = ccr.encode(cases.case(np.float32, 1e-3, (40, 24, 20))["bytes"])
    nd = ccr.split(dbl)[0][6]
    d0 = e0 + 8 * nd + 4 * nd + (-4 * nd % 8)                        # the first stream of dbl: its first 7 bits are an mbits
    one = one_cell_coded(ONE)
    o0 = e0 + 8                                                      # its cell table; its stream starts 8 bytes on
    assert len(one) == o0 + 16
    return [
        # the header and entry rules of the fixed-width reader
        ("empty", b"", "shorter than the header"),
        ("short header", g[:103], "shorter than the header"),
        ("magic", b"VNRCORC2" + g[8:], "bad magic"),
        ("fixed-width bytes", cases.case(np.int16, 2, (40, 24, 20))["bytes"], "bad magic"),
        ("packed bytes", cpr.pack(cases.case(np.int16, 2, (40, 24, 20))["bytes"]), "bad magic"),
        ("version", patched(g, 8, "<I", 2), "unsupported version"),
        ("type 6", patched(g, 12, "<I", 6), "unknown value type"),
        ("type 13", patched(g, 12, "<I", 13), "unknown value type"),
        ("dims zero", patched(g, 20, "<i", 0), "dims must be positive"),
        ("dims negative", patched(g, 16, "<i", -40), "dims must be positive"),
        ("n_flagged", patched(g, 28, "<I", 13), "exceeds the number of cells"),
        ("cells descending", patched(patched(g, e0, "<I", cell(1)), e0 + 8, "<I", cell(0)), "strictly ascending"),
        ("cells equal", patched(g, e0 + 8, "<I", cell(0)), "strictly ascending"),
        ("cell out of range", patched(g, e0 + 8 * (n - 1), "<I", 12), "out of range"),
        ("width 3", patched(g, e0 + 4, "<I", 3), "illegal code width"),
        ("width 8 for kind 0", patched(g, e0 + 4, "<I", 8), "illegal code width"),
        ("verbatim double with width 4", patched(dbl, e0 + 4, "<I", 4), "illegal code width"),
        ("kind 1 for an integer type", patched(g, 48, "<I", 1), "inconsistent"),
        ("kind 0 for a float type", patched(flt, 48, "<I", 0), "inconsistent"),
        ("kind 2 with eps > 0", patched(patched(flt, 48, "<I", 2), 56, "<Q", 0), "inconsistent"),
        ("kind 3", patched(g, 48, "<I", 3), "unknown kind"),
        ("step", patched(g, 56, "<Q", 13), "inconsistent"),
        ("eps negative", patched(g, 32, "<d", -5.0), "inconsistent"),
        ("eps NaN", patched(g, 32, "<d", float("nan")), "inconsistent"),
        ("eps infinite", patched(flt, 32, "<d", float("inf")), "inconsistent"),
        ("reserved 32", patched(g, 52, "<I", 1), "reserved"),
        ("reserved 64", patched(g, 96, "<Q", 1 << 40), "reserved"),
        ("entries cut", g[:e0 + 8 * n - 4], "size"),
        ("one byte short", g[:-1], "size differs from header + entries + payload"),
        ("one byte long", g + b"\0", "size differs from header + entries + payload"),
        ("payload_bytes against the size", patched(g, 80, "<Q", f[15] + 8), "size differs from header + entries + payload"),
        # the rules of the coded payload
        ("cell table padding", one_cell_coded(ONE, pad=b"\0\0\1\0"), "cell table padding"),
        ("payload shorter than the cell table", patched(one[:o0 + 4], 80, "<Q", 4), "shorter than the cell table"),
        ("payload_bytes against the table", patched(g + b"\0" * 8, 80, "<Q", f[15] + 8), "the sum the cell table gives"),
        ("streams cut", patched(g[:-8], 80, "<Q", f[15] - 8), "the sum the cell table gives"),
        ("payload not whole words", patched(g + b"\0" * 4, 80, "<Q", f[15] + 4), "the sum the cell table gives"),
        ("a record past its cell's words", one_cell_coded([(2, 7), (0, 1), ((1 << 64) - 1, 64)], words=1, groups_after=0), "runs past its cell's words"),
        ("the last group past its cell's words", one_cell_coded([(0, 7)] * 10, dims=(16, 16, 3), words=1, groups_after=0), "runs past its cell's words"),
        ("table entry above the records' length", one_cell_coded(ONE, words=2), "differs from the length its records have"),
        ("stream padding", patched(one, o0 + 8 + 7, "<B", 0x80), "stream padding"),
        ("mbits above 8 * width", one_cell_coded([(9, 7)] + lst(0) + lst() * 8 + [(1, 1)]), "exceeds 8 * width"),
        ("mbits above 64", patched(dbl, d0, "<B", 0x7f), "exceeds 8 * width"),
        ("2^(8 width - 1) without its sign", one_cell_coded([(8, 7)] + lst(0) + lst() * 7 + [(0, 1)]), "does not fit the width"),
        ("a code beyond the width", one_cell_coded([(8, 7)] + lst(0) + lst() * 6 + lst(0) + [(1, 1)]), "does not fit the width"),
        ("top plane empty", one_cell_coded([(2, 7)] + lst() + lst(0) + [(0, 1)]), "top plane is empty"),
        ("list count above 9", one_cell_coded([(1, 7)] + lst(*range(10)) + [(0, 1)] * 10), "list count is above 9"),
        ("dense with 9 bits set", one_cell_coded([(1, 7), (0, 1), (0x1ff, 64)] + [(0, 1)] * 9), "stored dense with 9 or fewer"),
        ("list lanes equal", one_cell_coded([(1, 7)] + lst(5, 5) + [(0, 1)] * 2), "not strictly ascending"),
        ("list lanes descending", one_cell_coded([(1, 7)] + lst(6, 5) + [(0, 1)] * 2), "not strictly ascending"),
        ("a list lane beyond the voxels", one_cell_coded([(1, 7)] + lst(30) + [(0, 1)], dims=(5, 3, 2)), "beyond the cell's voxels"),
        ("a dense bit beyond the voxels", one_cell_coded([(1, 7), (0, 1), (0x1ff | 1 << 63, 64)] + [(0, 1)] * 10, dims=(5, 3, 2)), "beyond the cell's voxels"),
    ]


@pytest.mark.parametrize("name,data", valid_crafted_streams(), ids=[b[0].replace(" ", "_") for b in valid_crafted_streams()])
def test_streams_written_by_hand_at_the_edge_of_a_rule_are_read(name, data):
    c = api.Correction.from_coded_bytes(data)
    assert c.to_coded_bytes() == data and ccr.encode(c.to_bytes()) == data and ccr.decode(data) == c.to_bytes()


@pytest.mark.parametrize("name,data,word", broken_blobs(), ids=[b[0].replace(" ", "_") for b in broken_blobs()])
def test_coded_reader_refuses_every_broken_rule_by_name(name, data, word):
    h = api.lib().vnrAmdCreateCorrectionFromCodedBytes(data, len(data))
    msg = api._lib.last_error()
    assert not h and PREFIX in msg and word in msg, msg


def test_each_reader_refuses_the_other_two_forms():
    v1 = cases.case(np.int16, 2, (40, 24, 20))["bytes"]
    forms = {"fixed": (v1, api.Correction.from_bytes, "malformed correction bytes: bad magic"),
             "packed": (cpr.pack(v1), api.Correction.from_packed_bytes, "malformed packed correction bytes: bad magic"),
             "coded": (ccr.encode(v1), api.Correction.from_coded_bytes, PREFIX + "bad magic")}
    for reader, (_, read, message) in forms.items():
        for form, (data, _, _) in forms.items():
            if form == reader:
                read(data).release()
            else:
                with pytest.raises(api.VnrAmdError, match=message):
                    read(data)


def test_null_arguments_are_refused():
    L = api.lib()
    h, msg = L.vnrAmdCreateCorrectionFromCodedBytes(None, 200), api._lib.last_error()
    assert not h and "null bytes" in msg
    out, n = C.c_void_p(), C.c_size_t()
    assert L.vnrAmdCorrectionSerializeCoded(None, C.byref(out), C.byref(n)) != 0 and "null correction" in api._lib.last_error()
    assert L.vnrAmdCorrectionSerializeCodedToDevice(None, None, 0, C.byref(n), None) != 0 and "null correction" in api._lib.last_error()
    c = api.Correction.from_coded_bytes(good())
    assert L.vnrAmdCorrectionSerializeCoded(c.h, None, C.byref(n)) != 0 and "null result" in api._lib.last_error()
    assert L.vnrAmdCorrectionSerializeCoded(c.h, C.byref(out), None) != 0 and "null result" in api._lib.last_error()
    assert L.vnrAmdCorrectionSerializeCodedToDevice(c.h, None, 0, None, None) != 0 and "null result" in api._lib.last_error()
    c.release()


# ------------------------------------------------------------------------------------------------ sanitizers
def test_coded_reader_transcoders_and_writer_are_clean_under_sanitizers(tmp_path):
    """valid coded blobs of every kind, the broken ones above and a few thousand seeded truncations and byte flips (mostly in the
    header, the entries, the cell table and the first words of streams, where the rules are) through
    csrc/correction_coded_format.cpp, csrc/correction_packed_format.cpp and csrc/correction_format.cpp compiled with
    -fsanitize=address,undefined into a stand-alone program (a CPU build; a subprocess): whatever parses is transcoded both ways and
    written back to the same bytes there"""
    rng = np.random.default_rng(13)
    valid = [ccr.encode(v1) for name, v1 in BLOBS if name not in ("many-cells", "gaussian")] + [b[1] for b in valid_crafted_streams()]
    corpus = list(valid) + [ccr.encode(dict(BLOBS)["gaussian"])] + [b[1] for b in broken_blobs()]
    for i in range(3000):
        b = bytearray(valid[i % len(valid)])
        if i % 3 == 0:
            b = b[:int(rng.integers(0, len(b)))]
        else:
            n_flagged = struct.unpack_from("<I", b, 28)[0]
            head = 104 + 8 * n_flagged + 4 * n_flagged + 8 + 32      # header, entries, the cell table and the first words of the first stream
            for _ in range(int(rng.integers(1, 4))):
                at = int(rng.integers(0, min(head, len(b)) if rng.uniform() < 0.8 else len(b)))
                b[at] = (b[at] ^ (1 << int(rng.integers(0, 8)))) if rng.uniform() < 0.5 else int(rng.integers(0, 256))
        corpus.append(bytes(b))
    path = str(tmp_path / "corpus.bin")
    with open(path, "wb") as f:
        for b in corpus:
            f.write(struct.pack("<I", len(b)) + b)
    exe = str(tmp_path / "correction_coded_asan")
    csrc = os.path.join(os.path.dirname(HERE), "instantvnr_amd", "csrc")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        os.path.join(HERE, "correction_coded_asan_harness.cpp"), os.path.join(csrc, "correction_coded_format.cpp"),
                        os.path.join(csrc, "correction_packed_format.cpp"), os.path.join(csrc, "correction_format.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    h = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert h.returncode == 0, (h.returncode, h.stdout[-500:], h.stderr[-3000:])
    parsed, refused = (int(x) for x in h.stdout.split() if x.isdigit())
    assert parsed >= len(valid) + 1 and refused > 1500 and parsed + refused == len(corpus), h.stdout


def test_the_series_tool_offers_the_coded_form():
    root = os.path.dirname(HERE)
    assert "--coded" in open(os.path.join(root, "tools", "README.md")).read()
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "insitu_series.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--coded" in out.stdout
