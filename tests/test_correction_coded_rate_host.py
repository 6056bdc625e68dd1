"""Byte budgets in the coded form, the host side (include/vnr_amd.h, "byte budgets in the coded form"): the closed form of a coded
record's length (tests/correction_coded_rate_ref.py) equals, record by record and cell by cell, what the numpy encoder
tests/correction_coded_ref.py really produces; csrc/correction_coded_format.cpp's correction_coded_record_bits gives the same counts
and they are what its writer writes, in a stand-alone program under address / undefined-behaviour sanitizers; three broken closed
forms are told from the true one; coded sizes can grow with the tolerance and the search still chooses what numpy chooses; the
interface is there.  CPU only; every comparison has tolerance zero."""
import ctypes as C
import functools
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from instantvnr_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "instantvnr_amd", "csrc")
sys.path.insert(0, HERE)
import correction_coded_cases as ccc  # noqa: E402
import correction_coded_rate_ref as ccrr  # noqa: E402
import correction_coded_ref as ccr  # noqa: E402
import correction_pack_ref as cpr  # noqa: E402
import correction_rate_ref as crr  # noqa: E402
import error_bound_ref as ebr  # noqa: E402


def random_codes():
    """(name, fixed-width bytes) of one-cell corrections with seeded random codes: per group a magnitude scale and a density of
    non-zero lanes, so that planes with counts on both sides of the list / dense boundary, empty planes and groups of zeros occur;
    ragged cells with short last groups; 1-, 2- and 4-byte codes and both verbatim types"""
    rng = np.random.default_rng(77)
    out = []
    for name, dtype, eps, width, dims in (("w1", np.int16, 5.0, 1, (16, 16, 3)), ("w2", np.int16, 5.0, 2, (5, 3, 2)), ("w2-ragged", np.int16, 5.0, 2, (7, 16, 9)),
                                          ("w4", np.int32, 1.0, 4, (16, 16, 16)), ("f32", np.float32, 0, 4, (16, 9, 5)), ("f64", np.float64, 0, 8, (13, 16, 4))):
        n = dims[0] * dims[1] * dims[2]
        groups = -(-n // 64)
        top = 8 * width if ebr.kind_of(dtype, eps) == 2 else 8 * width - 1
        scale = rng.integers(0, top + 1, groups)                                      # bit length of the group's largest magnitude
        density = rng.choice([0.0, 0.05, 0.15, 0.3, 1.0], groups)
        mag = np.array([int(rng.integers(0, 1 << 62)) & ((1 << int(s)) - 1) for s in scale.repeat(64)], np.uint64)[:n]
        mag = np.where(rng.uniform(size=n) < density.repeat(64)[:n], mag, np.uint64(0))
        if ebr.kind_of(dtype, eps) == 2:
            codes = mag
        else:
            codes = mag.astype(np.int64) * rng.choice([-1, 1], n)
        out.append((f"random-{name}", ccc.one_cell(dtype, eps, width, dims, codes)))
    return out


@functools.lru_cache(maxsize=None)
def blobs():
    return ccc.all_blobs() + random_codes()


NAMES = [b[0] for b in blobs()]


def cells_of_blob(v1):
    """yields (m [groups, 64], s or None) for every flagged cell of a fixed-width blob, in entry order"""
    f, cells, payload = cpr.split(v1, b"VNRCORR1")
    at = 0
    for cell, width in cells:
        n = cpr.cell_voxels(f[3:6], cell)
        yield ccr.magnitudes(payload, at, n, width, f[10])
        at += n * width + (-(n * width) % 16)
    assert at == len(payload)


def cell_table(coded):
    f, cells, payload = ccr.split(coded)
    return list(struct.unpack_from("<%dI" % len(cells), payload, 0))


@functools.lru_cache(maxsize=None)
def closed_form(name):
    """-> [(words, [bits of every record])] of the blob's flagged cells by the closed form"""
    out = []
    for m, s in cells_of_blob(dict(blobs())[name]):
        bits = ccrr.group_bits(m, s is not None)
        out.append((ccrr.cell_words(bits), [int(b) for b in bits]))
    return out


# ------------------------------------------------------------------------------------------------ the closed form against the encoder
@pytest.mark.parametrize("name", NAMES)
def test_the_closed_form_is_the_length_the_encoder_produces(name):
    v1 = dict(blobs())[name]
    table = cell_table(ccr.encode(v1))                          # what the encoder really wrote, cell by cell
    closed = closed_form(name)
    assert [w for w, _ in closed] == table
    seen = set()
    for (m, s), (_, bits) in zip(cells_of_blob(v1), closed):
        for g in range(len(m)):
            key = (m[g].tobytes(), None if s is None else s[g].tobytes())
            if key in seen:                                     # (a record already checked: mostly the groups of zeros)
                continue
            seen.add(key)
            assert ccr.group_record(m[g], None if s is None else s[g])[1] == bits[g], (name, g)
    f, cells, payload = ccr.split(ccr.encode(v1))
    n = len(cells)
    assert len(payload) == 4 * n + (-4 * n % 8) + 8 * sum(table)


def test_the_inputs_meet_the_edges_of_the_closed_form():
    counts = set()
    for name, v1 in blobs():
        for m, s in cells_of_blob(v1):
            for b in range(int(m.max()).bit_length()):
                counts.update(int(c) for c in ((m >> np.uint64(b)) & np.uint64(1)).sum(axis=1))
    assert {0, 1, 8, 9, 10, 11, 64} <= counts
    assert any(b == 7 for w, bits in closed_form("plane-counts") for b in bits)                  # a group of zeros in a flagged cell
    assert closed_form("longest-w4")[0][0] == ccc.LONGEST_WORDS[False] and closed_form("longest-f64")[0][0] == ccc.LONGEST_WORDS[True]


# ------------------------------------------------------------------------------------------------ the C++ function
def test_the_host_function_counts_what_numpy_counts_and_what_the_writer_writes_under_sanitizers(tmp_path):
    """correction_coded_record_bits of csrc/correction_coded_format.cpp in a stand-alone program built with -fsanitize=address,undefined
    (a CPU build; a subprocess): every record of every blob, and every cell's words against the cell table its writer makes"""
    exe = str(tmp_path / "correction_coded_rate_harness")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                        os.path.join(HERE, "correction_coded_rate_harness.cpp"), os.path.join(CSRC, "correction_coded_format.cpp"),
                        os.path.join(CSRC, "correction_packed_format.cpp"), os.path.join(CSRC, "correction_format.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    path = str(tmp_path / "corpus.bin")
    with open(path, "wb") as f:
        for _, v1 in blobs():
            f.write(struct.pack("<I", len(v1)) + v1)
    h = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert h.returncode == 0 and h.stderr == "", (h.returncode, h.stdout[-500:], h.stderr[-3000:])
    lines = h.stdout.splitlines()
    at = 0
    for name, _ in blobs():
        closed = closed_form(name)
        assert lines[at] == "blob %d" % len(closed), (name, lines[at])
        for i, (words, bits) in enumerate(closed):
            assert [int(x) for x in lines[at + 1 + i].split()] == [words] + bits, (name, i)
        at += 1 + len(closed)
    assert at == len(lines)


# ------------------------------------------------------------------------------------------------ sharpness
def totals(**broken):
    """-> (the bits of all records, the words of all cells) over all blobs under a variant of the closed form"""
    per_group = broken.pop("words_per_group", False)
    bits = words = 0
    for _, v1 in blobs():
        for m, s in cells_of_blob(v1):
            b = ccrr.group_bits(m, s is not None, **broken)
            bits += int(b.sum())
            words += ccrr.cell_words(b, per_group)
    return bits, words


def test_broken_closed_forms_differ_from_the_encoder():
    true_bits, true_words = totals()
    assert true_words == sum(sum(cell_table(ccr.encode(v1))) for _, v1 in blobs())               # the encoder's, on the same inputs
    for broken in ({"list_max": 8}, {"list_max": 11}, {"sign_every_lane": True}):
        bits, words = totals(**broken)
        assert bits != true_bits and words != true_words, broken
    # a list of ten lanes costs 5 + 6 * 10 = 65 bits, exactly the dense plane: a threshold of 10 changes the bytes of a stream and
    # never its length, so no size can tell it from 9 (the format stores such a plane dense; the reader refuses the list)
    assert totals(list_max=10) == (true_bits, true_words)
    bits, words = totals(words_per_group=True)
    assert bits == true_bits and words > true_words
    # ... and record by record, on the blob made for it: planes of 1, 9 and 10 lanes
    m, s = next(cells_of_blob(ccc.plane_counts()))
    assert int(ccrr.group_bits(m, True)[0]) == 7 + 11 + 59 + 65 + 20
    assert int(ccrr.group_bits(m, True, list_max=8)[0]) == 7 + 11 + 65 + 65 + 20
    assert int(ccrr.group_bits(m, True, sign_every_lane=True)[0]) == 7 + 11 + 59 + 65 + 64


# ------------------------------------------------------------------------------------------------ sizes that grow with the tolerance
def growing_fields():
    """one cell of 16 x 16 x 1 float32 voxels, decoded as 0, with twelve residuals of 1.0 in each of its four groups.  At eps = 1/8
    every code is 4: one dense plane and two empty lists a group.  At the LARGER eps = 1/6 every code is 3: two dense planes."""
    dec = np.zeros((1, 16, 16), np.float32)
    ref = dec.copy()
    ref.reshape(4, 64)[:, 5:17] = 1.0
    return dec, ref


TIGHT, LOOSE = 0.125, 1.0 / 6.0


def test_a_coded_size_can_grow_with_the_tolerance():
    dec, ref = growing_fields()
    tight, loose = ccrr.rate(dec, ref, TIGHT), ccrr.rate(dec, ref, LOOSE)
    for eps, r in ((TIGHT, tight), (LOOSE, loose)):                                              # both are what is really written
        coded = ccr.encode(ebr.build(dec, ref, eps, (0.0, 1.0))["bytes"])
        assert len(coded) == r["coded_serialized_bytes"] and cell_table(coded) == [r["coded_stream_words"]]
    assert [int(b) for b in ccrr.group_bits(*next(ccrr.flagged_cells(dec, ref, TIGHT))[1:])] == [7 + 65 + 5 + 5 + 12] * 4
    assert [int(b) for b in ccrr.group_bits(*next(ccrr.flagged_cells(dec, ref, LOOSE))[1:])] == [7 + 65 + 65 + 12] * 4
    assert TIGHT < LOOSE and tight["coded_serialized_bytes"] == 104 + 8 + 8 + 8 * 6 < loose["coded_serialized_bytes"] == 104 + 8 + 8 + 8 * 10
    assert tight["packed_serialized_bytes"] >= loose["packed_serialized_bytes"] and tight["serialized_bytes"] >= loose["serialized_bytes"]


def bits(d):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", d))[0]


def test_the_search_over_sizes_that_grow_chooses_what_numpy_chooses(tmp_path):
    """csrc/correction_budget.cpp, unchanged, in tests/correction_budget_harness.cpp under sanitizers, over step functions of sizes
    that are NOT monotone: the prefix / suffix rule defines the outcome and correction_rate_ref.budget_search restates it"""
    exe = str(tmp_path / "correction_budget_harness")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                        os.path.join(HERE, "correction_budget_harness.cpp"), os.path.join(CSRC, "correction_budget.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    eps_hi = 0.8125
    # (name, max_bytes, rounds, base, [(threshold, bytes)]): size(eps) = the bytes of the largest threshold <= eps
    searches = [
        ("a bump on the ladder", 1000, 2, 9000, [(0.01, 5000), (0.07, 900), (0.15, 2000), (0.25, 600), (0.5, 104)]),
        ("a bump inside a round", 1000, 3, 9000, [(0.051, 900), (0.07, 1200), (0.08, 800)]),
        ("a dip below the bracket", 1000, 2, 9000, [(0.02, 700), (0.03, 5000), (0.3, 400)]),
        ("sizes of the growing field", 175, 2, 232, [(TIGHT, 168), (LOOSE, 200), (0.21, 168)]),       # (0.125 fits, too, and is never probed)
    ]
    for name, max_bytes, rounds, base, steps in searches:
        assert any(a[1] < b[1] for a, b in zip(steps, steps[1:])), name                           # not monotone
        h = subprocess.run([exe, str(max_bytes), bits(eps_hi), str(rounds), bits(0.0), str(base)] + [f"{bits(t)}:{s}" for t, s in steps],
                           capture_output=True, text=True, timeout=120)
        assert h.returncode == 0 and h.stderr == "", (h.returncode, h.stdout[-500:], h.stderr[-3000:])
        probes = []

        def size_of(points):
            probes.append("probe " + " ".join(bits(e) for e in points) + "\n")
            return [dict(steps)[max(t for t, _ in steps if t <= e)] if any(t <= e for t, _ in steps) else base for e in points]

        r = crr.budget_search(size_of, max_bytes, eps_hi, rounds)
        want = f"eps {bits(r['eps'])} bytes {r['bytes']} tighter {bits(r['eps_tighter'])} bytes_tighter {r['bytes_tighter']} passes {r['rate_passes']}\n" + "".join(probes)
        assert h.stdout == want, (name, h.stdout, want)
        assert r["bytes"] <= max_bytes < r["bytes_tighter"] and r["eps_tighter"] < r["eps"]       # what is chosen fits
    # the steps of the last search are real sizes of the growing field
    dec, ref = growing_fields()
    assert [ccrr.rate(dec, ref, e)["coded_serialized_bytes"] for e in (TIGHT, LOOSE, 0.21)] == [168, 200, 168]


# ------------------------------------------------------------------------------------------------ the interface
def test_header_library_and_bindings_know_the_coded_entry_points():
    text = open(os.path.join(ROOT, "include", "vnr_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("vnrAmdNeuralVolumeCorrectionRatesCoded", 10), ("vnrAmdNeuralVolumeBuildCorrectionCodedWithinBytes", 11)):
        assert re.search(r"\b%s\s*\(" % name, code)
        assert name in api._lib.declared_symbols()
        f = getattr(api.lib(), name)                                    # exported
        assert f.argtypes is not None and len(f.argtypes) == n_args
    assert re.search(r"typedef struct vnrAmdCorrectionRateCoded \{", code)
    assert re.search(r"^#define VNR_AMD_CORRECTION_FORM_CODED 2\b", code, flags=re.M)
    R, RC = api._lib.CorrectionRate, api._lib.CorrectionRateCoded
    assert C.sizeof(RC) == 96 and C.sizeof(R) == 72
    assert [n for n, _ in RC._fields_] == ["rate"] + list(ccrr.FIELDS) and RC._fields_[0][1] is R and RC.rate.offset == 0
    assert [getattr(RC, n).offset for n in ccrr.FIELDS] == [72, 80, 88]
    assert [(n, getattr(R, n).offset) for n, _ in R._fields_] == [("eps", 0), ("kind", 8), ("refused", 12)] + [(n, 16 + 8 * i) for i, n in enumerate(crr.FIELDS)]
    assert api.CORRECTION_FORMS == {"fixed": 0, "packed": 1} and api.CORRECTION_FORM_CODED == 2
    assert "Coded sizes CAN grow with the tolerance" in text
    assert not re.search(r"Not built:[^.]*rate call", text)


def test_refusals_of_the_coded_calls_that_need_no_device_are_reported_by_name():
    L = api.lib()
    out = (api._lib.CorrectionRateCoded * 64)()
    eps = (C.c_double * 64)(*([0.5] * 64))
    fake = C.c_void_p(256)                                              # never dereferenced: every call below is refused before

    def rates(word, e, n, o):
        st = L.vnrAmdNeuralVolumeCorrectionRatesCoded(None, fake, 8, None, 1.0, 0.0, e, n, None, o)
        msg = api._lib.last_error()
        assert st != 0 and word in msg, (word, msg)
        return msg

    rates("null eps", None, 3, out)
    rates("null result", eps, 3, None)
    for n in (0, -1, 65):
        assert str(n) in rates("n_eps must be 1 .. 64", eps, n, out)
    for k, bad, shown in ((0, -0.25, "-0.25"), (63, float("nan"), "nan"), (17, float("inf"), "inf")):
        e = (C.c_double * 64)(*([0.5] * 64))
        e[k] = bad
        msg = rates("eps[%d]" % k, e, 64, out)
        assert shown in msg and "finite tolerance >= 0" in msg
    rates("null volume", eps, 64, out)

    report = api._lib.CorrectionBudget()

    def within(word, eps_hi=1.0, rounds=2, rep=C.byref(report)):
        h = L.vnrAmdNeuralVolumeBuildCorrectionCodedWithinBytes(None, fake, 8, None, 1.0, 0.0, 1000, eps_hi, rounds, None, rep)
        msg = api._lib.last_error()
        assert not h and word in msg, (word, msg)

    within("null result", rep=None)
    within("eps_hi must be a finite tolerance > 0", eps_hi=0.0)
    within("eps_hi must be a finite tolerance > 0", eps_hi=float("nan"))
    within("normal number", eps_hi=2.0 ** -1010)
    within("rounds must be 0 .. 8", rounds=9)
    within("rounds must be 0 .. 8", rounds=-1)
    within("null volume")
    # the existing call still refuses the form the new define names, and Python still refuses a word it does not know
    h = L.vnrAmdNeuralVolumeBuildCorrectionWithinBytes(None, fake, 8, None, 1.0, 0.0, 1000, api.CORRECTION_FORM_CODED, 1.0, 2, None, C.byref(report))
    assert not h and "unknown serialised form 2" in api._lib.last_error()
    with pytest.raises(api.VnrAmdError, match="form must be"):
        api.vnrNeuralVolumeBuildCorrectionWithinBytes(None, 256, np.float32, 1000, 1.0, form="planes")
    with pytest.raises(api.VnrAmdError, match="1 to 64"):
        api.vnrNeuralVolumeCorrectionRates(None, 256, np.float32, [], coded=True)


def test_the_series_tool_offers_a_coded_byte_budget():
    text = open(os.path.join(ROOT, "tools", "README.md")).read()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "insitu_series.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    assert "--budget-form coded" in text and re.search(r"--budget-form \{[^}]*coded[^}]*\}", out.stdout)
