"""CPU checks of the in-situ ingest surface (include/vnr_amd.h "in-situ ground truth"): the C-ABI declares and exports
the three entry points, the Python layer binds and wraps them, bad arguments are refused before the library is called, and a machine
without a device answers Create with an error, not a crash.  No kernel runs here."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from instantvnr_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vnrAmdCreateSimpleVolumeFromDevice", "vnrAmdSimpleVolumeUpdateFromDevice", "vnrAmdSimpleVolumeAppendTimeStepFromDevice"]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


def test_header_declares_the_three_functions():
    text = open(_lib.HEADER).read()
    assert re.search(r"vnrAmdVolume\s+vnrAmdCreateSimpleVolumeFromDevice\(const void\* d_data, const int dims\[3\], int value_type,\s*"
                     r"const int64_t strides\[3\],\s*float range_lo, float range_hi, void\* stream, float used_range\[2\]\);", text)
    for n in NAMES[1:]:
        assert re.search(r"int\s+" + n + r"\(vnrAmdVolume, const void\* d_data, int value_type, const int64_t strides\[3\],\s*"
                         r"float range_lo, float range_hi, void\* stream, float used_range\[2\]\);", text)
    for n in NAMES:
        assert n in _lib.declared_symbols()


def test_library_exports_them_and_lib_binds_them(L):
    for n, n_args in zip(NAMES, (8, 8, 8)):
        assert hasattr(L, n)
        fn = getattr(L, n)
        assert fn.argtypes is not None and len(fn.argtypes) == n_args
        assert C.POINTER(C.c_int64) in fn.argtypes
    assert L.vnrAmdCreateSimpleVolumeFromDevice.restype is C.c_void_p
    assert L.vnrAmdSimpleVolumeUpdateFromDevice.restype is C.c_int and L.vnrAmdSimpleVolumeAppendTimeStepFromDevice.restype is C.c_int


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) for arguments the wrapper must refuse itself")


@pytest.mark.parametrize("kwargs,match", [
    (dict(dtype=np.uint64), "data type"), (dict(dtype=np.float16), "data type"), (dict(dtype="no such type"), "data type"),
    (dict(dims=(4, 4)), "dims"), (dict(dims=(4, 0, 4)), "dims"), (dict(dims=(4, 4, 4, 4)), "dims"),
    (dict(strides=(1, 4)), "strides"), (dict(strides=(1, 0, 16)), "strides"), (dict(strides=(1, -4, 16)), "strides"),
    (dict(d_ptr=0), "null")])
def test_wrappers_refuse_bad_arguments_without_calling_the_library(monkeypatch, kwargs, match):
    monkeypatch.setattr(api, "lib", lambda: _NoLibrary())
    a = dict(d_ptr=0x1000, dims=(4, 4, 4), dtype=np.uint8, strides=None)
    a.update(kwargs)
    with pytest.raises(api.VnrAmdError, match=match):
        api.vnrCreateSimpleVolumeFromDevice(a["d_ptr"], a["dims"], a["dtype"], a["strides"])
    if "dims" in kwargs:
        return
    volume = type("V", (), {"h": 0x2000})()
    with pytest.raises(api.VnrAmdError, match=match):
        api.vnrSimpleVolumeUpdateFromDevice(volume, a["d_ptr"], a["dtype"], a["strides"])
    with pytest.raises(api.VnrAmdError, match=match):
        api.vnrSimpleVolumeAppendTimeStepFromDevice(volume, a["d_ptr"], a["dtype"], a["strides"])


def test_null_volume_and_null_data_are_errors_not_crashes(L):
    used = (C.c_float * 2)()
    dims = (C.c_int * 3)(4, 4, 4)
    assert L.vnrAmdSimpleVolumeUpdateFromDevice(None, C.c_void_p(0x1000), 0, None, 1.0, 0.0, None, used) != 0
    assert "null volume" in _lib.last_error()
    assert L.vnrAmdSimpleVolumeAppendTimeStepFromDevice(None, C.c_void_p(0x1000), 0, None, 1.0, 0.0, None, used) == -1
    assert "null volume" in _lib.last_error()
    # the argument checks of Create come before the first device call
    assert not L.vnrAmdCreateSimpleVolumeFromDevice(None, dims, 0, None, 1.0, 0.0, None, used)
    assert "null device data" in _lib.last_error()
    assert not L.vnrAmdCreateSimpleVolumeFromDevice(C.c_void_p(0x1000), (C.c_int * 3)(4, -1, 4), 0, None, 1.0, 0.0, None, used)
    assert "dimensions must be positive" in _lib.last_error()
    assert not L.vnrAmdCreateSimpleVolumeFromDevice(C.c_void_p(0x1000), dims, 0, (C.c_int64 * 3)(1, 0, 16), 1.0, 0.0, None, used)
    assert "strides must be positive" in _lib.last_error()
    for t, word in ((6, "64-bit"), (7, "64-bit"), (9, "vector"), (10, "vector"), (11, "vector"), (13, "unknown value type")):
        assert not L.vnrAmdCreateSimpleVolumeFromDevice(C.c_void_p(0x1000), dims, t, None, 1.0, 0.0, None, used)
        assert word in _lib.last_error()


def test_create_without_a_device_is_an_error_with_a_message():
    """in a child process: the test session itself must not initialise a HIP runtime.  With a device present the pointer below
    would be read, so the child only reports that there is one."""
    code = ("import sys, ctypes as C; sys.path.insert(0, %r)\n"
            "from instantvnr_amd import _lib\n"
            "L = _lib.lib()\n"
            "if L.vnrAmdDeviceCount() > 0:\n"
            "    print('HAS_DEVICE'); sys.exit(0)\n"
            "h = L.vnrAmdCreateSimpleVolumeFromDevice(C.c_void_p(0x1000), (C.c_int * 3)(4, 4, 4), 0, None, 1.0, 0.0, None, None)\n"
            "print('HANDLE', h, 'MESSAGE', _lib.last_error())\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    if "HAS_DEVICE" in out.stdout:
        return
    assert "HANDLE None MESSAGE" in out.stdout
    assert "no HIP capable devices" in out.stdout


def test_documents_describe_the_feature():
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "In situ" in integration and "vnrAmdSimpleVolumeUpdateFromDevice" in integration
    assert "insitu_series.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "insitu_series.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--compare-host" in out.stdout and "--steps-per-frame" in out.stdout
