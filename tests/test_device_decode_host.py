"""CPU checks of the in-situ round trip surface (include/vnr_amd.h "in-situ round trip"): the C-ABI declares and exports
the two entry points with the agreed signatures, the Python layer binds and wraps them, bad arguments are refused before the library is
called, the documents name the chunk variable, and a machine without a device answers with an error, not a crash.  No kernel runs here."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from instantvnr_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vnrAmdNeuralVolumeDecodeToDevice", "vnrAmdNeuralVolumeErrorAgainstDevice"]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


def test_header_declares_both_functions_with_the_agreed_signatures():
    text = open(_lib.HEADER).read()
    assert re.search(r"int\s+vnrAmdNeuralVolumeDecodeToDevice\(vnrAmdVolume neural, void\* d_out, int value_type, const int64_t strides\[3\],\s*"
                     r"const int box_lo\[3\], const int box_size\[3\], const int grid_dims\[3\],\s*"
                     r"float range_lo, float range_hi, void\* stream\);", text)
    assert re.search(r"typedef struct vnrAmdDecodeError \{ uint64_t n_voxels; double max_abs; int worst\[3\]; double sum_abs, sum_sq, psnr_db; \} "
                     r"vnrAmdDecodeError;", text)
    assert re.search(r"int\s+vnrAmdNeuralVolumeErrorAgainstDevice\(vnrAmdVolume neural, const void\* d_ref, int value_type, const int64_t strides\[3\],\s*"
                     r"const int box_lo\[3\], const int box_size\[3\], float range_lo, float range_hi,\s*"
                     r"void\* stream, vnrAmdDecodeError\* out, float\* d_block_max\);", text)
    for n in NAMES:
        assert n in _lib.declared_symbols()
    assert "NaN" in text[text.index("in-situ round trip"):text.index("typedef struct vnrAmdDecodeError")]      # what a NaN does is stated


def test_library_exports_them_and_lib_binds_them(L):
    for n, n_args in zip(NAMES, (10, 11)):
        fn = getattr(L, n)
        assert fn.restype is C.c_int and fn.argtypes is not None and len(fn.argtypes) == n_args
        assert C.POINTER(C.c_int64) in fn.argtypes
    assert C.POINTER(_lib.DecodeError) in L.vnrAmdNeuralVolumeErrorAgainstDevice.argtypes
    # the structure of the header: 8 + 8 + 12 (+ 4 padding) + 3 * 8 bytes
    assert C.sizeof(_lib.DecodeError) == 56 and _lib.DecodeError.worst.offset == 16 and _lib.DecodeError.sum_abs.offset == 32
    assert [f[0] for f in _lib.DecodeError._fields_] == ["n_voxels", "max_abs", "worst", "sum_abs", "sum_sq", "psnr_db"]


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) for arguments the wrapper must refuse itself")


@pytest.mark.parametrize("kwargs,match", [
    (dict(dtype=np.uint64), "data type"), (dict(dtype=np.float16), "data type"), (dict(dtype="no such type"), "data type"),
    (dict(strides=(1, 4)), "strides"), (dict(strides=(1, 0, 16)), "strides"), (dict(strides=(1, -4, 16)), "strides"),
    (dict(d_ptr=0), "null"),
    (dict(box=((0, 0, 0), (4, 4))), "box"), (dict(box=((0, 0, 0), (4, 0, 4))), "box"), (dict(box=((0, -1, 0), (4, 4, 4))), "box"), (dict(box=(1, 2, 3)), "box"),
    (dict(dtype=np.uint8, value_range=None), "value range"), (dict(dtype=np.int32, value_range=None), "value range"),
    (dict(value_range=(2.0, 2.0)), "value range"), (dict(value_range=(3.0, 1.0)), "value range")])
def test_wrappers_refuse_bad_arguments_without_calling_the_library(monkeypatch, kwargs, match):
    monkeypatch.setattr(api, "lib", lambda: _NoLibrary())
    a = dict(d_ptr=0x1000, dtype=np.float32, strides=None, box=None, value_range=(0.0, 1.0))
    a.update(kwargs)
    volume = type("V", (), {"h": 0x2000})()
    with pytest.raises(api.VnrAmdError, match=match):
        api.vnrNeuralVolumeDecodeToDevice(volume, a["d_ptr"], a["dtype"], a["strides"], a["box"], None, a["value_range"])
    with pytest.raises(api.VnrAmdError, match=match):
        api.vnrNeuralVolumeErrorAgainstDevice(volume, a["d_ptr"], a["dtype"], a["strides"], a["box"], a["value_range"])


@pytest.mark.parametrize("grid_dims", [(4, 4), (4, 0, 4), (4, 4, 4, 4)])
def test_decode_wrapper_refuses_bad_grid_dims(monkeypatch, grid_dims):
    monkeypatch.setattr(api, "lib", lambda: _NoLibrary())
    volume = type("V", (), {"h": 0x2000})()
    with pytest.raises(api.VnrAmdError, match="grid dims"):
        api.vnrNeuralVolumeDecodeToDevice(volume, 0x1000, np.float32, grid_dims=grid_dims)


def test_null_and_simple_volumes_are_errors_not_crashes(L):
    e = _lib.DecodeError()
    assert L.vnrAmdNeuralVolumeDecodeToDevice(None, C.c_void_p(0x1000), 8, None, None, None, None, 1.0, 0.0, None) != 0
    assert "null volume" in _lib.last_error()
    assert L.vnrAmdNeuralVolumeErrorAgainstDevice(None, C.c_void_p(0x1000), 8, None, None, None, 1.0, 0.0, None, C.byref(e), None) != 0
    assert "null volume" in _lib.last_error()


def test_calls_without_a_device_are_errors_with_a_message():
    """in a child process: the test session itself must not initialise a HIP runtime.  Without a device no neural volume can exist, so the
    calls meet the handle the failed creation returned; with one, the GPU suite covers them and the child only reports that."""
    code = ("import sys, ctypes as C; sys.path.insert(0, %r)\n"
            "from instantvnr_amd import _lib\n"
            "L = _lib.lib()\n"
            "if L.vnrAmdDeviceCount() > 0:\n"
            "    print('HAS_DEVICE'); sys.exit(0)\n"
            "cfg = b'{\"encoding\": {\"otype\": \"HashGrid\"}, \"network\": {\"otype\": \"FullyFusedMLP\"}}'\n"
            "h = L.vnrAmdCreateNeuralVolumeFromDims(cfg, len(cfg), 0, (C.c_int * 3)(8, 8, 8))\n"
            "print('HANDLE', h, 'MESSAGE', _lib.last_error())\n"
            "e = _lib.DecodeError()\n"
            "a = L.vnrAmdNeuralVolumeDecodeToDevice(h, C.c_void_p(0x1000), 8, None, None, None, None, 1.0, 0.0, None)\n"
            "print('DECODE', a, _lib.last_error())\n"
            "b = L.vnrAmdNeuralVolumeErrorAgainstDevice(h, C.c_void_p(0x1000), 8, None, None, None, 1.0, 0.0, None, C.byref(e), None)\n"
            "print('ERROR', b, _lib.last_error())\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    if "HAS_DEVICE" in out.stdout:
        return
    assert "HANDLE None MESSAGE" in out.stdout and "no HIP capable devices" in out.stdout
    assert "DECODE 1 null volume" in out.stdout and "ERROR 1 null volume" in out.stdout


def test_documents_describe_the_feature():
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "VNR_AMD_DECODE_CHUNK" in integration and "vnrAmdNeuralVolumeDecodeToDevice" in integration
    assert "vnrAmdNeuralVolumeErrorAgainstDevice" in integration
    assert "vnrAmdNeuralVolumeDecodeToDevice" in open(os.path.join(ROOT, "README.md")).read()
    assert "decode.hip" in open(os.path.join(ROOT, "DESIGN.md")).read()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "insitu_series.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--round-trip" in out.stdout
