"""Packed corrections, the host side (include/vnr_amd.h, "packed corrections"): the numpy restatement of the format
(tests/correction_pack_ref.py) round-trips the fixed-width form, the library's packed reader, writer and host unpack
(csrc/correction_packed_format.cpp behind vnrAmdCreateCorrectionFromPackedBytes, pure host code) agree with it byte for byte, every
rule of the reader is broken once, and reader, unpack and writer run under address / undefined-behaviour sanitizers in a stand-alone
program.  CPU only; every comparison has tolerance zero."""
import ctypes as C
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
import correction_pack_cases as cases  # noqa: E402
import correction_pack_ref as cpr  # noqa: E402
import error_bound_ref as ebr  # noqa: E402


def all_blobs():
    """(name, fixed-width bytes) of every case: built ones, crafted ones"""
    out = [(i, cases.case(*c)["bytes"]) for i, c in zip(cases.IDS, cases.CASES)]
    return out + [(f"crafted-{t.__name__}-{e}-w{w}", cases.crafted(t, e, w)[0]) for t, e, w in cases.CRAFTED]


def table_of(packed):
    """-> (nbits of every group, widths per group)"""
    f, cells, payload = cpr.split(packed, b"VNRCORP1")
    groups = [-(-cpr.cell_voxels(f[3:6], c) // 64) for c, _ in cells]
    return list(payload[:sum(groups)]), [w for (_, w), g in zip(cells, groups) for _ in range(g)]


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("name,v1", all_blobs(), ids=[b[0] for b in all_blobs()])
def test_reference_round_trip_and_size_bound(name, v1):
    packed = cpr.pack(v1)
    assert cpr.unpack(packed) == v1
    nbits, widths = table_of(packed)
    payload_bytes = cpr.split(packed, b"VNRCORP1")[0][15]
    pad8 = len(nbits) + (-len(nbits) % 8)
    assert payload_bytes == pad8 + 8 * sum(nbits)
    assert payload_bytes <= pad8 + 64 * sum(widths)          # nbits <= 8 * width for every group
    assert all(n <= 8 * w for n, w in zip(nbits, widths))


def test_the_cases_cover_the_format():
    """code widths 1, 2 and 4 in kinds 0 and 1, verbatim float32 and float64, groups of zeros, idle lanes, cells of 16 voxels;
    the crafted blobs have exactly the group widths they were made for"""
    seen, zero_groups = set(), 0
    for c in cases.CASES:
        out = cases.case(*c)
        seen.update((out["kind"], w) for _, w in out["cells"])
        zero_groups += table_of(cpr.pack(out["bytes"]))[0].count(0)
    assert seen >= {(0, 1), (0, 2), (0, 4), (1, 1), (1, 2), (1, 4), (2, 4), (2, 8)}, seen
    assert zero_groups > 50
    assert any(cpr.cell_voxels((17, 16, 33), c) == 16 for c, _ in cases.case(np.int32, 1, (17, 16, 33))["cells"])
    assert cases.case(np.int32, 1, (5, 3, 2))["cells"] == [(0, 1)]
    for t, e, w in cases.CRAFTED:
        v1, want = cases.crafted(t, e, w)
        assert table_of(cpr.pack(v1))[0] == want
    assert cases.crafted(np.float64, 0, 8)[1][2] == 64
    assert 250 <= cases.many_cells()["n_flagged"] <= 320


# ------------------------------------------------------------------------------------------------ the library on the host
def same_info(a, b):
    return all(v == b[k] or (isinstance(v, float) and math.isnan(v) and math.isnan(b[k])) for k, v in a.items()) and a.keys() == b.keys()


@pytest.mark.parametrize("name,v1", all_blobs(), ids=[b[0] for b in all_blobs()])
def test_library_reads_unpacks_and_writes_what_numpy_packs(name, v1):
    packed = cpr.pack(v1)
    c = api.Correction.from_packed_bytes(packed)
    assert c.to_packed_bytes() == packed                     # (before the host unpack, and after it)
    assert c.to_bytes() == v1
    assert c.to_packed_bytes() == packed
    fixed = api.Correction.from_bytes(v1)
    assert same_info(c.info(), fixed.info()) and c.info()["payload_bytes"] == cpr.split(v1, b"VNRCORR1")[0][15]
    # info() first: the unpack it triggers is the same
    d = api.Correction.from_packed_bytes(packed)
    assert same_info(d.info(), fixed.info()) and d.to_bytes() == v1
    for h in (c, d, fixed):
        h.release()


def test_a_correction_without_a_flagged_cell_packs_on_the_host():
    dec = np.zeros((3, 4, 5), np.float32)
    v1 = ebr.build(dec, dec, 0.5, None)["bytes"]
    packed = cpr.pack(v1)
    assert len(packed) == ebr.HEADER.size and cpr.unpack(packed) == v1
    assert api.Correction.from_bytes(v1).to_packed_bytes() == packed      # (no group: no device is asked for)
    assert api.Correction.from_packed_bytes(packed).to_bytes() == v1


# ------------------------------------------------------------------------------------------------ refusals
def patched(b, offset, fmt, value):
    return b[:offset] + struct.pack(fmt, value) + b[offset + struct.calcsize(fmt):]


def good():
    return cpr.pack(cases.case(np.int16, 2, (40, 24, 20))["bytes"])


def broken_blobs():
    """(name, bytes, a word of the refusal): every rule of the packed reader broken once, everything else left valid"""
    g = good()
    f, cells, payload = cpr.split(g, b"VNRCORP1")
    n = len(cells)
    assert n >= 3
    e0 = ebr.HEADER.size
    p0 = e0 + 8 * n
    cell = lambda i: cells[i][0]
    dbl = cpr.pack(cases.case(np.float64, 0, (40, 24, 20))["bytes"])
    flt = cpr.pack(cases.case(np.float32, 1e-3, (40, 24, 20))["bytes"])
    one = cpr.pack(cases.crafted(np.int16, 5.0, 1)[0])               # one cell of 8 groups, 1-byte codes: nbits 0, 1, 8, 8, 3, 0, 0, 0
    o0 = e0 + 8                                                      # its group table; its planes start 8 bytes on
    tiny = cpr.pack(cases.case(np.int32, 1, (5, 3, 2))["bytes"])     # one group of 30 codes, 7 bytes of table padding
    assert cpr.split(tiny, b"VNRCORP1")[2][0] >= 1 and cpr.split(one, b"VNRCORP1")[2][:8] == bytes([0, 1, 8, 8, 3, 0, 0, 0])
    return [
        # the header and entry rules of the fixed-width reader
        ("empty", b"", "shorter than the header"),
        ("short header", g[:103], "shorter than the header"),
        ("magic", b"VNRCORP2" + g[8:], "bad magic"),
        ("fixed-width bytes", cases.case(np.int16, 2, (40, 24, 20))["bytes"], "bad magic"),
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
        # the rules of the packed payload
        ("nbits above 8 * width", patched(one, o0 + 1, "<B", 9), "exceeds 8 * width"),
        ("top plane zero", patched(one, o0 + 8, "<Q", 0), "top plane"),
        ("bit in an idle lane", patched(tiny, e0 + 8 + 8, "<Q", struct.unpack_from("<Q", tiny, e0 + 16)[0] | 1 << 30), "beyond the cell's voxels"),
        ("table padding", patched(tiny, e0 + 8 + 5, "<B", 1), "padding"),
        ("one byte short", g[:-1], "size differs from header + entries + payload"),
        ("one byte long", g + b"\0", "size differs from header + entries + payload"),
        ("payload_bytes against the size", patched(g, 80, "<Q", f[15] + 8), "size differs from header + entries + payload"),
        ("payload_bytes against the table", patched(g + b"\0" * 8, 80, "<Q", f[15] + 8), "the sum the group table gives"),
        ("planes cut", patched(g[:-8], 80, "<Q", f[15] - 8), "the sum the group table gives"),
        ("payload shorter than the table", patched(g[:p0 + 8], 80, "<Q", 8), "shorter than the group table"),
    ]


@pytest.mark.parametrize("name,data,word", broken_blobs(), ids=[b[0].replace(" ", "_") for b in broken_blobs()])
def test_packed_reader_refuses_every_broken_rule_by_name(name, data, word):
    h = api.lib().vnrAmdCreateCorrectionFromPackedBytes(data, len(data))
    msg = api._lib.last_error()
    assert not h and "malformed packed correction bytes: " in msg and word in msg, msg


def test_each_reader_refuses_the_other_form():
    h = api.lib().vnrAmdCreateCorrectionFromBytes(good(), len(good()))
    msg = api._lib.last_error()
    assert not h and "malformed correction bytes" in msg and "bad magic" in msg
    with pytest.raises(api.VnrAmdError, match="malformed packed correction bytes: bad magic"):
        api.Correction.from_packed_bytes(cases.case(np.int16, 2, (40, 24, 20))["bytes"])


def test_null_arguments_are_refused():
    L = api.lib()
    h, msg = L.vnrAmdCreateCorrectionFromPackedBytes(None, 200), api._lib.last_error()
    assert not h and "null bytes" in msg
    out, n = C.c_void_p(), C.c_size_t()
    assert L.vnrAmdCorrectionSerializePacked(None, C.byref(out), C.byref(n)) != 0 and "null correction" in api._lib.last_error()
    c = api.Correction.from_packed_bytes(good())
    assert L.vnrAmdCorrectionSerializePacked(c.h, None, C.byref(n)) != 0 and "null result" in api._lib.last_error()
    assert L.vnrAmdCorrectionSerializePacked(c.h, C.byref(out), None) != 0 and "null result" in api._lib.last_error()
    c.release()


# ------------------------------------------------------------------------------------------------ sanitizers
def test_packed_reader_unpack_and_writer_are_clean_under_sanitizers(tmp_path):
    """valid packed blobs of every kind, the broken ones above and a few thousand seeded truncations and byte flips (mostly in the
    header, the entries and the group table, where the rules are) through csrc/correction_packed_format.cpp and
    csrc/correction_format.cpp compiled with -fsanitize=address,undefined into a stand-alone program (a CPU build; a subprocess):
    whatever parses is unpacked and written back to the same bytes there"""
    rng = np.random.default_rng(12)
    valid = [cpr.pack(v1) for _, v1 in all_blobs()]
    corpus = list(valid) + [b[1] for b in broken_blobs()]
    for i in range(3000):
        b = bytearray(valid[i % len(valid)])
        if i % 3 == 0:
            b = b[:int(rng.integers(0, len(b)))]
        else:
            n_flagged = struct.unpack_from("<I", b, 28)[0]
            head = 104 + 8 * n_flagged + 64 * n_flagged              # header, entries and (at least) the group table
            for _ in range(int(rng.integers(1, 4))):
                at = int(rng.integers(0, min(head, len(b)) if rng.uniform() < 0.8 else len(b)))
                b[at] = (b[at] ^ (1 << int(rng.integers(0, 8)))) if rng.uniform() < 0.5 else int(rng.integers(0, 256))
        corpus.append(bytes(b))
    path = str(tmp_path / "corpus.bin")
    with open(path, "wb") as f:
        for b in corpus:
            f.write(struct.pack("<I", len(b)) + b)
    exe = str(tmp_path / "correction_packed_asan")
    csrc = os.path.join(os.path.dirname(HERE), "instantvnr_amd", "csrc")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        os.path.join(HERE, "correction_packed_asan_harness.cpp"), os.path.join(csrc, "correction_packed_format.cpp"),
                        os.path.join(csrc, "correction_format.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    h = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert h.returncode == 0, (h.returncode, h.stdout[-500:], h.stderr[-3000:])
    parsed, refused = (int(x) for x in h.stdout.split() if x.isdigit())
    assert parsed >= len(valid) and refused > 1500 and parsed + refused == len(corpus), h.stdout


def test_the_series_tool_offers_the_packed_form():
    root = os.path.dirname(HERE)
    assert "--packed" in open(os.path.join(root, "tools", "README.md")).read()
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "insitu_series.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--packed" in out.stdout
