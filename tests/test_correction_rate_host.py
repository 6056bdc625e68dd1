"""Corrections to a byte budget, the host side (include/vnr_amd.h, "corrections to a byte budget"): the numpy restatement
tests/correction_rate_ref.py computes the rates of a ladder of tolerances from the codes alone and finds, for every case of
tests/correction_pack_cases.py, the sizes and counts of error_bound_ref.build followed by correction_pack_ref.pack; the search of
csrc/correction_budget.cpp, in a stand-alone program under address / undefined-behaviour sanitizers and fed a step function of sizes,
chooses the double that budget_search chooses, bit for bit.  CPU only; every comparison has tolerance zero."""
import ctypes as C
import functools
import math
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
sys.path.insert(0, HERE)
import correction_pack_cases as cases  # noqa: E402
import correction_pack_ref as cpr  # noqa: E402
import correction_rate_ref as crr  # noqa: E402
import error_bound_ref as ebr  # noqa: E402


def many_cells_fields():
    """dec / ref of correction_pack_cases.many_cells, restated (the case itself keeps only what the build made of them)"""
    dims = (128, 120, 70)
    rng = np.random.default_rng(5)
    shape = dims[::-1]
    dec = rng.integers(-1000, 1000, shape).astype(np.int16)
    q = np.rint(rng.normal(0.0, 1.0, shape) * rng.choice([0.15, 30.0, 900.0], (5, 8, 8)).repeat(16, 0).repeat(16, 1).repeat(16, 2)[:70, :120, :128]).astype(np.int64)
    q[:, :32, :48] = 0
    return dec, (dec + 5 * q).astype(np.int16)


def fields_of(name):
    if name == "many-cells":
        return many_cells_fields()
    t, e, d = cases.CASES[cases.IDS.index(name)]
    return cases.fields(t, d, e, seed=d[0] * 131 + np.dtype(t).itemsize)


def ladder(dec, ref):
    """max |ref - dec| * 2^-j, j = 0 .. 15; 0 (kind 2 for floats, E = 0 for integers); for floats one tolerance small enough to be
    refused: the largest residual over twice it is 2^32, a code beyond 32 bits"""
    with np.errstate(invalid="ignore", over="ignore"):
        top = float(np.nanmax(np.abs(ref.astype(np.float64) - dec.astype(np.float64))))
    assert top > 0
    return [math.ldexp(top, -j) for j in range(16)] + [0.0] + ([math.ldexp(top, -33)] if dec.dtype.kind == "f" else [])


@functools.lru_cache(maxsize=None)
def ladder_rates(name):
    dec, ref = fields_of(name)
    tol = ladder(dec, ref)
    return tol, crr.rates(dec, ref, tol)


ALL = cases.IDS + ["many-cells"]


@pytest.mark.parametrize("name", ALL)
def test_rates_equal_the_sizes_of_build_and_pack(name):
    dec, ref = fields_of(name)
    if name == "many-cells":
        assert ebr.build(dec, ref, 2, (0.0, 1.0))["bytes"] == cases.many_cells()["bytes"]          # the restated fields are the case's
    tol, got = ladder_rates(name)
    n_refused = 0
    for eps, r in zip(tol, got):
        assert r["eps"] == eps and r["kind"] == ebr.kind_of(dec.dtype, eps)
        try:
            b = ebr.build(dec, ref, eps, (-3.0, 9.5))
        except ValueError:
            n_refused += 1
            assert r["refused"] and all(r[k] == 0 for k in crr.FIELDS), (name, eps, r)
            continue
        packed = cpr.pack(b["bytes"])
        n_groups = sum(-(-cpr.cell_voxels(dec.shape[::-1], c) // 64) for c, _ in b["cells"])
        want = {"n_flagged": b["n_flagged"], "n_voxels_flagged": b["n_voxels_flagged"], "n_groups": n_groups, "payload_bytes": b["payload_bytes"],
                "serialized_bytes": len(b["bytes"]), "packed_payload_bytes": len(packed) - 104 - 8 * b["n_flagged"], "packed_serialized_bytes": len(packed)}
        assert not r["refused"] and {k: r[k] for k in crr.FIELDS} == want, (name, eps)
    assert n_refused == (1 if dec.dtype.kind == "f" else 0)                                       # the last of the ladder, and nothing else
    assert got[0]["n_flagged"] == 0 and got[0]["serialized_bytes"] == got[0]["packed_serialized_bytes"] == 104      # eps = the maximum error
    assert got[16]["n_flagged"] > 0 and got[16]["kind"] in (0, 2)


@pytest.mark.parametrize("name", ALL)
def test_sizes_do_not_grow_with_the_tolerance(name):
    tol, got = ladder_rates(name)
    order = sorted((e, i) for i, e in enumerate(tol) if not got[i]["refused"])
    for form in ("serialized_bytes", "packed_serialized_bytes"):
        sizes = [got[i][form] for _, i in order]
        assert all(a >= b for a, b in zip(sizes, sizes[1:])), (name, form, sizes)
    assert got[order[0][1]]["serialized_bytes"] > got[order[-1][1]]["serialized_bytes"]


# ------------------------------------------------------------------------------------------------ the search
def bits(d):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", d))[0]


def step_function(base, steps, refused_below):
    def size_of(points):
        out = []
        for e in points:
            under = [t for t, _ in steps if t <= e]
            size = dict(steps)[max(under)] if under else base
            out.append(None if e < refused_below else size)
        return out
    return size_of


# (name, max_bytes, eps_hi, rounds, refused_below, base, [(threshold, bytes)])
EPS_HI = 0.8125
SEARCHES = [
    ("t0-does-not-fit", 1000, EPS_HI, 2, 0.0, 9000, [(EPS_HI, 1001)]),
    ("t0-refused", 1000, EPS_HI, 2, 1.0, 9000, [(EPS_HI, 500)]),
    ("all-fit", 1000, EPS_HI, 2, 0.0, 1000, []),
    ("no-point-of-a-round-fits", 1000, EPS_HI, 3, 0.0, 9000, [(math.ldexp(EPS_HI, -3), 400)]),
    ("rounds-0", 1000, EPS_HI, 0, 0.0, 9000, [(0.01, 5000), (0.07, 900), (0.3, 104)]),
    ("two-rounds", 1000, EPS_HI, 2, 0.0, 9000, [(0.01, 5000), (0.07, 900), (0.3, 104)]),
    ("eight-rounds", 1000, 1.0e-3 / 3, 8, 0.0, 9000, [(1.0e-5 / 7, 1000), (1.0e-4 / 3, 104)]),
    ("first-point-fits", 1000, EPS_HI, 1, 0.0, 9000, [(math.ldexp(EPS_HI, -4) * (1 + 1 / 32), 700)]),
    ("refused-below", 1000, EPS_HI, 2, 0.011, 600, []),
    ("t0-budget-zero", 0, EPS_HI, 1, 0.0, 104, []),
]
REFUSED_ARGUMENTS = [("eps_hi must be a finite tolerance > 0", 0.0, 2), ("eps_hi must be a finite tolerance > 0", -1.0, 2),
                     ("eps_hi must be a finite tolerance > 0", float("inf"), 2), ("eps_hi must be a finite tolerance > 0", float("nan"), 2),
                     ("normal number", 2.0 ** -1010, 2), ("rounds must be 0 .. 8", 1.0, 9), ("rounds must be 0 .. 8", 1.0, -1)]


@functools.lru_cache(maxsize=None)
def harness(tmp):
    exe = os.path.join(tmp, "correction_budget_harness")
    csrc = os.path.join(ROOT, "instantvnr_amd", "csrc")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        os.path.join(HERE, "correction_budget_harness.cpp"), os.path.join(csrc, "correction_budget.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def run_harness(exe, max_bytes, eps_hi, rounds, refused_below, base, steps):
    h = subprocess.run([exe, str(max_bytes), bits(eps_hi), str(rounds), bits(refused_below), str(base)] + [f"{bits(t)}:{s}" for t, s in steps],
                       capture_output=True, text=True, timeout=120)
    assert h.returncode == 0 and h.stderr == "", (h.returncode, h.stdout[-500:], h.stderr[-3000:])
    return h.stdout


def test_the_search_chooses_the_double_numpy_chooses_under_sanitizers(tmp_path_factory):
    exe = harness(str(tmp_path_factory.mktemp("budget")))
    seen = set()
    for name, max_bytes, eps_hi, rounds, refused_below, base, steps in SEARCHES:
        out = run_harness(exe, max_bytes, eps_hi, rounds, refused_below, base, steps)
        probes = []
        size_of = step_function(base, steps, refused_below)

        def recording(points):
            probes.append("probe " + " ".join(bits(e) for e in points) + "\n")
            return size_of(points)

        try:
            r = crr.budget_search(recording, max_bytes, eps_hi, rounds)
        except ValueError:
            assert out.startswith("refused: ") and str(max_bytes) in out and repr(eps_hi) in out and "size there is" in out, (name, out)
            seen.add("refused")
            continue
        tighter = "nan" if math.isnan(r["eps_tighter"]) else bits(r["eps_tighter"])
        want = f"eps {bits(r['eps'])} bytes {r['bytes']} tighter {tighter} bytes_tighter {r['bytes_tighter']} passes {r['rate_passes']}\n" + "".join(probes)
        assert out == want, (name, out, want)
        assert r["bytes"] <= max_bytes and r["eps"] <= eps_hi and r["rate_passes"] <= 1 + rounds
        if name == "all-fit":
            assert r["eps"] == math.ldexp(eps_hi, -15) and r["rate_passes"] == 1 and tighter == "nan" and r["bytes_tighter"] == 0
        if name == "no-point-of-a-round-fits":
            assert r["eps"] == math.ldexp(eps_hi, -3) and r["rate_passes"] == 4 and r["eps_tighter"] < r["eps"] and r["bytes_tighter"] == 9000
        if name == "rounds-0":
            assert r["rate_passes"] == 1 and r["eps"] == math.ldexp(eps_hi, -3) and r["eps_tighter"] == math.ldexp(eps_hi, -4)
        if name == "two-rounds":
            assert r["rate_passes"] == 3 and 0.07 <= r["eps"] < 0.07 * (1 + 2.0 ** -7) and r["eps_tighter"] < 0.07
        if name == "refused-below":
            assert r["bytes_tighter"] == 0 and r["eps_tighter"] < 0.011 <= r["eps"]
        seen.add(name)
    assert seen == {s[0] for s in SEARCHES if not s[0].startswith("t0-")} | {"refused"}
    for word, eps_hi, rounds in REFUSED_ARGUMENTS:
        out = run_harness(exe, 1000, eps_hi, rounds, 0.0, 100, [])
        assert out.startswith("refused: ") and word in out and out.count("\n") == 1, (word, out)


# ------------------------------------------------------------------------------------------------ the interface
def test_header_library_and_bindings_know_both_entry_points():
    text = open(os.path.join(ROOT, "include", "vnr_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("vnrAmdNeuralVolumeCorrectionRates", "vnrAmdNeuralVolumeBuildCorrectionWithinBytes"):
        assert re.search(r"\b%s\s*\(" % name, code)
        assert name in api._lib.declared_symbols()
        f = getattr(api.lib(), name)                                    # exported
        assert f.argtypes is not None and len(f.argtypes) == (10 if name.endswith("Rates") else 12)
    for struct_name in ("vnrAmdCorrectionRate", "vnrAmdCorrectionBudget"):
        assert re.search(r"typedef struct %s \{" % struct_name, code)
    assert "#define VNR_AMD_CORRECTION_FORM_FIXED  0" in code and "#define VNR_AMD_CORRECTION_FORM_PACKED 1" in code
    assert C.sizeof(api._lib.CorrectionRate) == 72 and C.sizeof(api._lib.CorrectionBudget) == 40
    assert [n for n, _ in api._lib.CorrectionRate._fields_] == ["eps", "kind", "refused"] + list(crr.FIELDS)
    assert callable(api.vnrNeuralVolumeCorrectionRates) and callable(api.vnrNeuralVolumeBuildCorrectionWithinBytes)


def test_refusals_that_need_no_device_are_reported_by_name():
    L = api.lib()
    out = (api._lib.CorrectionRate * 64)()
    eps = (C.c_double * 64)(*([0.5] * 64))
    fake = C.c_void_p(256)                                              # never dereferenced: every call below is refused before

    def rates(word, e, n, o):
        st = L.vnrAmdNeuralVolumeCorrectionRates(None, fake, 8, None, 1.0, 0.0, e, n, None, o)
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

    def within(word, form=1, eps_hi=1.0, rounds=2, rep=C.byref(report)):
        h = L.vnrAmdNeuralVolumeBuildCorrectionWithinBytes(None, fake, 8, None, 1.0, 0.0, 1000, form, eps_hi, rounds, None, rep)
        msg = api._lib.last_error()
        assert not h and word in msg, (word, msg)

    within("null result", rep=None)
    within("unknown serialised form 2", form=2)
    within("unknown serialised form -1", form=-1)
    within("eps_hi must be a finite tolerance > 0", eps_hi=0.0)
    within("eps_hi must be a finite tolerance > 0", eps_hi=float("nan"))
    within("normal number", eps_hi=2.0 ** -1010)
    within("rounds must be 0 .. 8", rounds=9)
    within("null volume")
    with pytest.raises(api.VnrAmdError, match="form must be"):
        api.vnrNeuralVolumeBuildCorrectionWithinBytes(None, 256, np.float32, 1000, 1.0, form="planes")
    with pytest.raises(api.VnrAmdError, match="1 to 64"):
        api.vnrNeuralVolumeCorrectionRates(None, 256, np.float32, [])
    with pytest.raises(api.VnrAmdError, match="1 to 64"):
        api.vnrNeuralVolumeCorrectionRates(None, 256, np.float32, [0.5] * 65)


def test_the_series_tool_offers_a_byte_budget():
    text = open(os.path.join(ROOT, "tools", "README.md")).read()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "insitu_series.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--byte-budget", "--budget-form", "--budget-rounds"):
        assert flag in text and flag in out.stdout
