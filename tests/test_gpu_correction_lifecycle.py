"""The life of a correction (include/vnr_amd.h: "error-bounded round trip", "packed corrections", "resident form", "coded corrections"):
every origin -- the two-call build, the direct build, fixed-width, packed and coded bytes -- taken through two sequences of applies,
serialisations and form changes that cross the lazy conversions in different orders.  After every step what was serialised equals
the numpy restatements' bytes, the corrected decode equals tests/error_bound_ref.py, and residency() equals a formula of the format's
sizes: which of {fixed-width payload + table, planes + index} the device holds then.  Only the public api is used; tolerance ZERO.

The setup is the (21, 10, 3) volume of tests/test_gpu_correction_direct.py (two cells of 480 and 150 voxels: a ragged cell, groups
that straddle rows, a short last group), shared with that file."""
import os
import sys

import numpy as np
import pytest

from instantvnr_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correction_coded_ref as ccr  # noqa: E402
import correction_index_ref as cir  # noqa: E402
import correction_pack_ref as cpr  # noqa: E402
import test_gpu_correction_direct as setup  # noqa: E402

pytestmark = pytest.mark.gpu

DIMS = setup.TAIL_DIMS
TYPES = [(np.float32, 1e-3), (np.int16, 2), (np.float64, 0)]
TYPE_IDS = [t.__name__ for t, _ in TYPES]
ORIGINS = ["built", "direct", "fixed-bytes", "packed-bytes", "coded-bytes"]
N_CELLS = 2

# what the device holds after a step: nothing; the fixed-width payload and its table; the planes and their index
NONE, FIXED, PLANES = "none", "fixed", "planes"
# (operation, its argument).  "device": the serialised bytes into device memory; "size": the size query of the same call
SEQUENCE_A = [("apply", None), ("packed_bytes", None), ("form", "packed"), ("apply", None), ("coded_bytes", None), ("form", "fixed"), ("apply", None),
              ("bytes", None), ("packed_device", "device"), ("coded_device", "device")]
SEQUENCE_B = [("coded_device", "size"), ("form", "packed"), ("coded_bytes", None), ("apply", None), ("bytes", None), ("form", "fixed"),
              ("packed_device", "device"), ("apply", None), ("packed_bytes", None)]
# (resident form, what the device holds) after every step.  A correction made on the device holds what its build left until a form
# change converts it; one read from bytes holds nothing, and only notes a form, until its first apply brings that form.
HELD = {
    "A": {"device-made": {"built": [("fixed", FIXED)] * 2 + [("packed", PLANES)] * 3 + [("fixed", FIXED)] * 5,
                          "direct": [("packed", PLANES)] * 5 + [("fixed", FIXED)] * 5}},
    "B": {"device-made": {"built": [("fixed", FIXED)] + [("packed", PLANES)] * 4 + [("fixed", FIXED)] * 4,
                          "direct": [("packed", PLANES)] * 5 + [("fixed", FIXED)] * 4}},
}
HELD["A"]["bytes"] = HELD["A"]["device-made"]["built"]
HELD["B"]["bytes"] = [("fixed", NONE)] + [("packed", NONE)] * 2 + [("packed", PLANES)] * 2 + [("fixed", FIXED)] * 4


def held_after(sequence, origin):
    return HELD[sequence]["device-made"][origin] if origin in ("built", "direct") else HELD[sequence]["bytes"]


def residency_of(form, held, blob, packed):
    """vnrAmdCorrectionResidency by the sizes of include/vnr_amd.h: the table is 16 bytes a cell of the grid, the index 16 bytes a
    cell and 4 bytes a group"""
    fixed_bytes, packed_bytes = cpr.split(blob, b"VNRCORR1")[0][15], cpr.split(packed, b"VNRCORP1")[0][15]
    n_groups = len(cir.index(packed)["group_word"])
    payload = {NONE: 0, FIXED: fixed_bytes, PLANES: packed_bytes}[held]
    index = 16 * N_CELLS + 4 * n_groups if held == PLANES else 0
    table = 16 * N_CELLS if held == FIXED else 0
    return {"form": form, "on_device": held != NONE, "payload_device_bytes": payload, "index_device_bytes": index, "device_bytes": payload + index + table}


def make(origin, dtype, eps, build_eps, forms):
    """a fresh correction of `origin`; forms: the numpy bytes {"bytes", "packed_bytes", "coded_bytes"}"""
    if origin in ("built", "direct"):
        build = api.vnrNeuralVolumeBuildCorrection if origin == "built" else api.vnrNeuralVolumeBuildCorrectionPacked
        d, _, ptr, strides = setup.device_reference(setup.reference(dtype, eps, DIMS), "ghost")
        try:
            return build(setup.trained(DIMS)[1], ptr, dtype, eps if build_eps is None else build_eps, strides, setup.RANGES[dtype])
        finally:
            d.free()
    read = {"fixed-bytes": (api.Correction.from_bytes, "bytes"), "packed-bytes": (api.Correction.from_packed_bytes, "packed_bytes"),
            "coded-bytes": (api.Correction.from_coded_bytes, "coded_bytes")}[origin]
    return read[0](forms[read[1]])


def to_device(call, want):
    """the bytes a ...ToDevice call writes equal `want`, and what lies behind them is untouched"""
    fill = np.full(len(want) + 24, 0xa5, np.uint8)
    d = api.DeviceArray.from_numpy(fill)
    try:
        assert call(d) == len(want)
        got = d.numpy()
        assert got[:len(want)].tobytes() == want and np.array_equal(got[len(want):], fill[len(want):])
    finally:
        d.free()


def run(corr, steps, held, dtype, forms, corrected, non_empty):
    blob, packed = forms["bytes"], forms["packed_bytes"]
    for i, ((op, arg), (form, what)) in enumerate(zip(steps, held)):
        where = (i, op, arg)
        if op == "apply":
            got, expect, offset, strides = setup.device_apply(corr, dtype, "ghost", DIMS)
            setup.box_view(expect, offset, strides, DIMS)[...] = corrected
            assert setup.same_bytes(got, expect), where
        elif op == "form":
            corr.set_resident_form(arg)
        elif op in ("bytes", "packed_bytes", "coded_bytes"):
            assert getattr(corr, "to_" + op)() == forms[op], where
        elif arg == "size":
            assert getattr(corr, "to_" + op)() == len(forms[op.replace("device", "bytes")]), where
        else:
            to_device(getattr(corr, "to_" + op), forms[op.replace("device", "bytes")])
        assert corr.residency() == residency_of(form, what if non_empty else NONE, blob, packed), where
    # at the end every form is there, whichever way it came
    assert (corr.to_bytes(), corr.to_packed_bytes(), corr.to_coded_bytes()) == (blob, packed, forms["coded_bytes"])
    assert corr.residency() == residency_of(held[-1][0], held[-1][1] if non_empty else NONE, blob, packed)


def numpy_forms(dtype, eps, build_eps=None):
    blob, packed, corrected = setup.expected(dtype, eps, DIMS, build_eps)
    return {"bytes": blob, "packed_bytes": packed, "coded_bytes": ccr.encode(blob)}, corrected


@pytest.mark.parametrize("sequence", ["A", "B"])
@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("dtype,eps", TYPES, ids=TYPE_IDS)
def test_every_step_of_a_corrections_life_keeps_bytes_results_and_residency(dtype, eps, origin, sequence, monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    forms, corrected = numpy_forms(dtype, eps)
    assert len(cpr.split(forms["bytes"], b"VNRCORR1")[1]) == N_CELLS and not setup.same_bytes(corrected, setup.decoded(dtype, DIMS))
    corr = make(origin, dtype, eps, None, forms)
    before = {"built": ("fixed", FIXED), "direct": ("packed", PLANES)}.get(origin, ("fixed", NONE))
    assert corr.residency() == residency_of(*before, forms["bytes"], forms["packed_bytes"])
    run(corr, SEQUENCE_A if sequence == "A" else SEQUENCE_B, held_after(sequence, origin), dtype, forms, corrected, True)
    corr.release()


@pytest.mark.parametrize("origin", ORIGINS)
def test_an_empty_correction_never_touches_the_device(origin, monkeypatch):
    monkeypatch.delenv("VNR_AMD_DECODE_CHUNK", raising=False)
    dtype, eps = TYPES[0]
    loose = 2.0 * setup.top_error(dtype, eps, DIMS) + 1.0
    forms, corrected = numpy_forms(dtype, eps, loose)
    assert cpr.split(forms["bytes"], b"VNRCORR1")[1] == [] and setup.same_bytes(corrected, setup.decoded(dtype, DIMS))
    assert len(forms["bytes"]) == len(forms["packed_bytes"]) == len(forms["coded_bytes"]) == 104
    corr = make(origin, dtype, eps, loose, forms)
    run(corr, SEQUENCE_A, held_after("A", origin), dtype, forms, corrected, False)
    corr.release()
