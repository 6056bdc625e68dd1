"""The index over a packed correction, the host side (include/vnr_amd.h, "resident form"): the numpy restatement
tests/correction_index_ref.py reads every code of every flagged cell out of the planes and finds what correction_pack_ref.unpack puts
into the fixed-width payload, and correction_plane_index of csrc/correction_packed_format.cpp gives the same index, in a stand-alone
program under address / undefined-behaviour sanitizers.  CPU only; every comparison has tolerance zero."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import correction_index_ref as cir  # noqa: E402
import correction_pack_cases as cases  # noqa: E402
import correction_pack_ref as cpr  # noqa: E402
import error_bound_ref as ebr  # noqa: E402


def all_blobs():
    """(name, fixed-width bytes) of every case: built ones, the one of about 300 cells, crafted ones"""
    out = [(i, lambda c=c: cases.case(*c)["bytes"]) for i, c in zip(cases.IDS, cases.CASES)]
    out += [("many-cells", lambda: cases.many_cells()["bytes"])]
    return out + [(f"crafted-{t.__name__}-{e}-w{w}", lambda k=(t, e, w): cases.crafted(*k)[0]) for t, e, w in cases.CRAFTED]


def fixed_codes(v1):
    """the codes of every flagged cell of a fixed-width blob: int64 (kinds 0 and 1) or uint64 bit patterns (kind 2)"""
    f, cells, payload = cpr.split(v1, b"VNRCORR1")
    out, at = [], 0
    for cell, width in cells:
        n = cpr.cell_voxels(f[3:6], cell)
        q = np.frombuffer(payload, cpr.CODE[width], n, at)
        out.append(q.view("<u%d" % width).astype(np.uint64) if f[10] == 2 else q.astype(np.int64))
        at += n * width + (-(n * width) % 16)
    return out


@pytest.mark.parametrize("name,make", all_blobs(), ids=[b[0] for b in all_blobs()])
def test_code_at_reads_every_code_of_the_fixed_width_payload(name, make):
    v1 = make()
    packed = cpr.pack(v1)
    ix = cir.index(packed)
    want = fixed_codes(cpr.unpack(packed))
    assert len(want) == len(ix["cells"]) > 0
    for i, codes in enumerate(want):
        got = cir.code_at(ix, i, np.arange(len(codes)))
        assert got.dtype == codes.dtype and np.array_equal(got, codes), (name, i)
    # one voxel at a time gives the same: the first, the last and a lane in the middle of the last cell
    for li in (0, len(want[-1]) // 2, len(want[-1]) - 1):
        assert cir.code_at(ix, len(want) - 1, li) == want[-1][li]


def test_the_index_of_the_crafted_blobs_covers_nbits_0_1_full_width_and_64():
    seen = set()
    for t, e, w in cases.CRAFTED:
        v1, nbits = cases.crafted(t, e, w)
        ix = cir.index(cpr.pack(v1))
        assert list(ix["nbits"]) == nbits and list(ix["group_word"]) == [0] + list(np.cumsum(nbits)[:-1]) and ix["cell_group0"] == [0] and ix["cell_word0"] == [0]
        seen.update(nbits)
        codes = fixed_codes(v1)[0]
        assert cir.code_at(ix, 0, 130) == codes[130] and cir.code_at(ix, 0, 200) == codes[200] and cir.code_at(ix, 0, 5) == 0
    assert seen >= {0, 1, 8, 16, 32, 64}


def test_the_index_of_many_cells_counts_what_the_residency_cap_counts():
    out = cases.many_cells()
    packed = cpr.pack(out["bytes"])
    ix = cir.index(packed)
    f, cells, payload = cpr.split(packed, b"VNRCORP1")
    assert len(ix["group_word"]) == 14788 and len(payload) == 876616 and cpr.split(out["bytes"], b"VNRCORR1")[0][15] == 1313280
    assert ix["cell_group0"][1] == 64 and ix["cell_word0"][1] == int(ix["nbits"][:64].sum())


# ------------------------------------------------------------------------------------------------ the library's index function
def patched(b, offset, fmt, value):
    return b[:offset] + struct.pack(fmt, value) + b[offset + struct.calcsize(fmt):]


def refused_blobs():
    """packed bytes the reader refuses, each with a group table that would take an unguarded index beyond the planes"""
    one = cpr.pack(cases.crafted(np.int16, 5.0, 1)[0])       # one cell of 8 groups, 1-byte codes: nbits 0, 1, 8, 8, 3, 0, 0, 0
    g = cpr.pack(cases.case(np.int16, 2, (40, 24, 20))["bytes"])
    o0 = ebr.HEADER.size + 8
    return [patched(one, o0 + 1, "<B", 200), patched(one, o0 + 7, "<B", 64), g[:-8], g[:ebr.HEADER.size + 4], patched(g, 28, "<I", 2), b""]


def test_library_index_equals_numpy_under_sanitizers(tmp_path):
    """csrc/correction_packed_format.cpp and csrc/correction_format.cpp compiled with -fsanitize=address,undefined into a stand-alone
    program (a CPU build; a subprocess): the index it prints for every valid blob is the numpy one, it gathers every code through the
    index and finds the host unpack's, and a blob the reader refuses never reaches the index function"""
    valid = [cpr.pack(make()) for _, make in all_blobs()]
    blobs = valid + refused_blobs()
    paths = []
    for i, b in enumerate(blobs):
        paths.append(str(tmp_path / f"blob{i}.bin"))
        with open(paths[-1], "wb") as f:
            f.write(b)
    exe = str(tmp_path / "correction_index_harness")
    csrc = os.path.join(os.path.dirname(HERE), "instantvnr_amd", "csrc")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        os.path.join(HERE, "correction_index_harness.cpp"), os.path.join(csrc, "correction_packed_format.cpp"),
                        os.path.join(csrc, "correction_format.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    h = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=600)
    assert h.returncode == 0, (h.returncode, h.stdout[-500:], h.stderr[-3000:])
    want = "".join(f"file {i}\n" + (cir.index_text(cir.index(b)) if i < len(valid) else "refused\n") for i, b in enumerate(blobs))
    assert h.stdout == want


def test_the_series_tool_offers_the_resident_form_and_a_region():
    root = os.path.dirname(HERE)
    text = open(os.path.join(root, "tools", "README.md")).read()
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "insitu_series.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--resident", "--roi"):
        assert flag in text and flag in out.stdout
