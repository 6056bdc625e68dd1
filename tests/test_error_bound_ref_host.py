"""Error-bounded round trip, the host side (include/vnr_amd.h, "error-bounded round trip"): the guarantees of the arithmetic on seeded
random data in numpy (tests/error_bound_ref.py), the serialised form through the library's reader and writer
(csrc/correction_format.cpp behind vnrAmdCreateCorrectionFromBytes, pure host code), every rule of the reader broken once, and the
reader under address / undefined-behaviour sanitizers in a stand-alone program.  CPU only."""
import ctypes as C
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from instantvnr_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import error_bound_ref as ebr  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DIMS = [(40, 24, 20), (17, 16, 33)]
ALL_TYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
# (eps per type: 0 = exact / verbatim; small ones give wide codes, large ones leave cells unflagged)
EPS = {np.uint8: [0, 0.5, 3, 40.7], np.int8: [0, 2.2, 60], np.uint16: [0, 1, 9.99, 700], np.int16: [0, 5, 20000],
       np.uint32: [2, 300.5, 1.0e6, 3.0e9], np.int32: [1, 1000, 5.0e8], np.float32: [0, 1e-7, 1e-3, 0.25, 3.0], np.float64: [0, 1e-6, 1e-4, 0.5]}


def fields(dtype, dims, seed):
    """seeded dec / ref [z, y, x]: the residual grows from nothing to the whole type range along x, so that cells range from
    untouched to far off; dec is pinned at both type limits in places (integers), with ref on either side"""
    rng = np.random.default_rng(seed)
    shape = dims[::-1]
    ramp = (np.arange(dims[0]) / max(dims[0] - 1, 1)) ** 4
    if np.dtype(dtype).kind == "f":
        dec = rng.uniform(-2.0, 5.0, shape).astype(dtype)
        ref = (dec.astype(np.float64) + rng.normal(0.0, 1.0, shape) * ramp * 40.0).astype(dtype)
        ref[:, :, :8] = dec[:, :, :8]                    # bit-identical columns
        ref[1, 2, 3] = dec[1, 2, 3] + dtype(2.0 ** -20)
        return dec, ref
    info = np.iinfo(dtype)
    span = float(info.max) - float(info.min)
    dec = rng.integers(info.min, info.max, shape, dtype=np.int64, endpoint=True)
    dec[2::5, 1::3, 1::7] = info.min
    dec[3::5, 2::3, 2::7] = info.max
    ref = np.clip(dec + np.rint(rng.normal(0.0, 1.0, shape) * ramp * span * 0.4).astype(np.int64), info.min, info.max)
    ref[2, 1, 1], ref[3, 2, 2] = info.max, info.min      # the farthest a voxel can be off, at both limits
    return dec.astype(dtype), ref.astype(dtype)


CASES = [(t, d, e) for t in ALL_TYPES for d in DIMS for e in EPS[t]]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@functools.lru_cache(maxsize=None)
def case(dtype, dims, eps):
    dec, ref = fields(dtype, dims, seed=dims[0] * 131 + np.dtype(dtype).itemsize)
    return dec, ref, ebr.build(dec, ref, eps, (0.0, 1.0))


@pytest.mark.parametrize("dtype,dims,eps", CASES, ids=[f"{t.__name__}-{d[0]}x{d[1]}x{d[2]}-{e}" for t, d, e in CASES])
def test_bounds_hold_and_the_bytes_apply_to_the_same_array(dtype, dims, eps):
    dec, ref, out = case(dtype, dims, eps)
    corrected, q = out["corrected"], out["q"]
    flagged = np.zeros(dec.shape, bool)
    by_cell = dict(out["cells"])
    for cell, sl in ebr.cells_of(dims):
        assert (cell in by_cell) == bool((q[sl] != 0).any())
        flagged[sl] = cell in by_cell
    assert same(corrected[~flagged], dec[~flagged])
    if np.dtype(dtype).kind != "f":
        E = int(np.floor(eps))
        r = ref.astype(np.int64) - dec.astype(np.int64)
        assert int(np.abs(corrected.astype(np.int64) - ref.astype(np.int64)).max()) <= E <= eps
        assert ((q == 0) == (np.abs(r) <= E)).all()
        assert ((dec == np.iinfo(dtype).min) & (q != 0)).any() and ((dec == np.iinfo(dtype).max) & (q != 0)).any()
        assert out["max_abs_after"] <= E
    elif eps > 0:
        r = ref.astype(np.float64) - dec.astype(np.float64)
        err = np.abs(corrected.astype(np.float64) - ref.astype(np.float64))
        assert (err <= ebr.float_bound(corrected, ref, dec, eps)).all()
        assert (np.abs(r[q == 0]) <= eps * (1 + 2.0 ** -50)).all() and (np.abs(r[q != 0]) >= eps * (1 - 2.0 ** -50)).all()
    else:
        assert same(corrected[flagged], ref[flagged])
        assert ((q != 0) == (ebr.bits(dec) != ebr.bits(ref)).reshape(dec.shape)).all()
    assert 0 < out["n_flagged"] and out["max_abs_after"] <= out["max_abs_before"]
    assert same(ebr.apply(dec, out["bytes"]), corrected)


def test_every_code_width_occurs_in_the_cases_above():
    """1, 2 and 4 byte codes, and verbatim float32 / float64"""
    seen = set()
    for c in CASES:
        out = case(*c)[2]
        seen.update((out["kind"] == 2, w) for _, w in out["cells"])
    assert seen >= {(False, 1), (False, 2), (False, 4), (True, 4), (True, 8)}, seen


def test_a_32_bit_type_far_off_needs_codes_wider_than_32_bits():
    dec, ref = fields(np.uint32, DIMS[1], seed=3)         # one voxel is 2^32 - 1 off
    with pytest.raises(ValueError, match="wider than 32 bits"):
        ebr.build(dec, ref, 0, (0.0, 1.0))


def test_some_cases_leave_cells_unflagged():
    n = 0
    for dtype, eps in ((np.uint8, 40.7), (np.float32, 8.0), (np.int16, 20000)):
        dec, ref = fields(dtype, DIMS[0], seed=5)
        out = ebr.build(dec, ref, eps, (0.0, 1.0))
        n += 0 < out["n_flagged"] < 12
    assert n == 3


def test_fnv1a64_test_vectors():
    assert ebr.fnv1a64(b"") == 0xcbf29ce484222325 and ebr.fnv1a64(b"a") == 0xaf63dc4c8601ec8c and ebr.fnv1a64(b"foobar") == 0x85944171f73967e8


# ------------------------------------------------------------------------------------------------ the library's reader and writer
def from_bytes(b):
    h = api.lib().vnrAmdCreateCorrectionFromBytes(b, len(b))
    return h, api._lib.last_error()


@functools.lru_cache(maxsize=None)
def blob(dtype=np.int16, eps=5.0, dims=DIMS[0]):
    dec, ref = fields(dtype, dims, seed=77)
    return ebr.build(dec, ref, eps, (-3.0, 9.5), params_hash=0x0123456789abcdef, n_params=4242)


@pytest.mark.parametrize("dtype,eps", [(np.uint8, 3), (np.int16, 5.0), (np.uint32, 300.5), (np.float32, 1e-3), (np.float32, 0), (np.float64, 0), (np.float64, 0.5)])
@pytest.mark.parametrize("dims", DIMS)
def test_numpy_bytes_round_trip_through_the_library(dtype, eps, dims):
    want = blob(dtype, eps, dims)
    c = api.Correction.from_bytes(want["bytes"])
    info = c.info()
    assert info["dims"] == dims and info["value_type"] == ebr.VALUE_TYPES[np.dtype(dtype)] and info["kind"] == want["kind"] and info["eps"] == float(eps)
    assert (info["range_lo"], info["range_hi"]) == (-3.0, 9.5)
    assert info["n_cells"] == np.prod([-(-d // 16) for d in dims]) and info["n_flagged"] == want["n_flagged"]
    assert info["payload_bytes"] == want["payload_bytes"] and info["serialized_bytes"] == len(want["bytes"])
    assert info["params_hash"] == 0x0123456789abcdef and info["n_params"] == 4242
    assert info["max_abs_after"] == want["max_abs_after"] and np.isnan(info["max_abs_before"])
    assert info["worst_after"] == (-1, -1, -1) and info["n_nan"] == 0
    assert c.to_bytes() == want["bytes"]
    c.release()


def patched(b, offset, fmt, value):
    return b[:offset] + struct.pack(fmt, value) + b[offset + struct.calcsize(fmt):]


def broken_blobs():
    """(name, bytes, a word of the refusal): every rule of the reader's list broken once, everything else left valid"""
    good = blob()["bytes"]
    n = blob()["n_flagged"]
    assert n >= 3
    e0 = ebr.HEADER.size
    cell = lambda i: struct.unpack_from("<I", good, e0 + 8 * i)[0]
    dbl = blob(np.float64, 0)["bytes"]
    flt = blob(np.float32, 1e-3)["bytes"]
    return [
        ("empty", b"", "shorter than the header"),
        ("short header", good[:103], "shorter than the header"),
        ("magic", b"VNRCORR2" + good[8:], "bad magic"),
        ("version", patched(good, 8, "<I", 2), "unsupported version"),
        ("type 6", patched(good, 12, "<I", 6), "unknown value type"),
        ("type 13", patched(good, 12, "<I", 13), "unknown value type"),
        ("dims zero", patched(good, 20, "<i", 0), "dims must be positive"),
        ("dims negative", patched(good, 16, "<i", -40), "dims must be positive"),
        ("n_flagged", patched(good, 28, "<I", 13), "exceeds the number of cells"),
        ("cells descending", patched(patched(good, e0, "<I", cell(1)), e0 + 8, "<I", cell(0)), "strictly ascending"),
        ("cells equal", patched(good, e0 + 8, "<I", cell(0)), "strictly ascending"),
        ("cell out of range", patched(good, e0 + 8 * (n - 1), "<I", 12), "out of range"),
        ("width 3", patched(good, e0 + 4, "<I", 3), "illegal code width"),
        ("width 8 for kind 0", patched(good, e0 + 4, "<I", 8), "illegal code width"),
        ("verbatim double with width 4", patched(dbl, e0 + 4, "<I", 4), "illegal code width"),
        ("kind 1 for an integer type", patched(good, 48, "<I", 1), "inconsistent"),
        ("kind 0 for a float type", patched(flt, 48, "<I", 0), "inconsistent"),
        ("kind 2 with eps > 0", patched(patched(flt, 48, "<I", 2), 56, "<Q", 0), "inconsistent"),
        ("kind 3", patched(good, 48, "<I", 3), "unknown kind"),
        ("step", patched(good, 56, "<Q", 13), "inconsistent"),
        ("eps negative", patched(good, 32, "<d", -5.0), "inconsistent"),
        ("eps NaN", patched(good, 32, "<d", float("nan")), "inconsistent"),
        ("eps infinite", patched(flt, 32, "<d", float("inf")), "inconsistent"),
        ("reserved 32", patched(good, 52, "<I", 1), "reserved"),
        ("reserved 64", patched(good, 96, "<Q", 1 << 40), "reserved"),
        ("payload_bytes", patched(good, 80, "<Q", blob()["payload_bytes"] + 16), "payload_bytes"),
        ("one byte short", good[:-1], "size"),
        ("one byte long", good + b"\0", "size"),
        ("entries cut", good[:e0 + 8 * n - 4], "size"),
    ]


@pytest.mark.parametrize("name,data,word", broken_blobs(), ids=[b[0].replace(" ", "_") for b in broken_blobs()])
def test_reader_refuses_every_broken_rule_by_name(name, data, word):
    h, msg = from_bytes(data)
    assert not h and "malformed correction bytes" in msg and word in msg, msg


def test_null_arguments_are_refused():
    L = api.lib()
    h, msg = L.vnrAmdCreateCorrectionFromBytes(None, 200), api._lib.last_error()
    assert not h and "null bytes" in msg
    assert L.vnrAmdCorrectionGetInfo(None, C.byref(api._lib.CorrectionInfo())) != 0 and "null correction" in api._lib.last_error()
    out, n = C.c_void_p(), C.c_size_t()
    assert L.vnrAmdCorrectionSerialize(None, C.byref(out), C.byref(n)) != 0 and "null correction" in api._lib.last_error()
    L.vnrAmdReleaseCorrection(None)
    c = api.Correction.from_bytes(blob()["bytes"])
    assert L.vnrAmdCorrectionGetInfo(c.h, None) != 0 and "null result" in api._lib.last_error()
    with pytest.raises(api.VnrAmdError, match="bad magic"):
        api.Correction.from_bytes(b"x" * 200)


def test_reader_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """valid blobs of every kind, the broken ones above and a few thousand seeded truncations and byte flips through
    csrc/correction_format.cpp compiled with -fsanitize=address,undefined into a stand-alone program (a CPU build; a subprocess)"""
    rng = np.random.default_rng(11)
    valid = [blob(t, e, d)["bytes"] for t, e in ((np.uint8, 3), (np.int16, 5.0), (np.uint32, 300.5), (np.float32, 1e-3), (np.float32, 0), (np.float64, 0)) for d in DIMS]
    corpus = list(valid) + [b[1] for b in broken_blobs()]
    for i in range(3000):
        b = bytearray(valid[i % len(valid)])
        if i % 3 == 0:
            b = b[:int(rng.integers(0, len(b)))]
        else:
            head = 104 + 8 * 12
            for _ in range(int(rng.integers(1, 4))):        # mostly in the header and the entries, where the rules are
                at = int(rng.integers(0, head if rng.uniform() < 0.8 else len(b)))
                b[at] = (b[at] ^ (1 << int(rng.integers(0, 8)))) if rng.uniform() < 0.5 else int(rng.integers(0, 256))
        corpus.append(bytes(b))
    path = str(tmp_path / "corpus.bin")
    with open(path, "wb") as f:
        for b in corpus:
            f.write(struct.pack("<I", len(b)) + b)
    exe = str(tmp_path / "correction_asan")
    csrc = os.path.join(os.path.dirname(HERE), "instantvnr_amd", "csrc")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        os.path.join(HERE, "correction_asan_harness.cpp"), os.path.join(csrc, "correction_format.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    h = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert h.returncode == 0, (h.returncode, h.stdout[-500:], h.stderr[-3000:])
    parsed, refused = (int(x) for x in h.stdout.split() if x.isdigit())
    assert parsed >= len(valid) and refused > 1500 and parsed + refused == len(corpus), h.stdout


def test_the_series_tool_offers_the_error_bound():
    root = os.path.dirname(HERE)
    assert "--error-bound" in open(os.path.join(root, "tools", "README.md")).read()
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "insitu_series.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--error-bound" in out.stdout
