"""CPU checks of the deterministic-training surface: the C-ABI declares and exports it, the Python layer wraps it, the
command-line trainer offers it and INTEGRATION.md lists its environment switch.  No compute call is made here."""
import os
import re
import subprocess
import sys

import pytest

from instantvnr_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vnrAmdNeuralVolumeSetDeterministicTraining", "vnrAmdNeuralVolumeGetDeterministicTraining"]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


def test_header_declares_the_two_functions_and_the_library_exports_them(L):
    text = open(_lib.HEADER).read()
    assert re.search(r"int\s+vnrAmdNeuralVolumeSetDeterministicTraining\(vnrAmdVolume, int enable\);", text)
    assert re.search(r"int\s+vnrAmdNeuralVolumeGetDeterministicTraining\(vnrAmdVolume, int\* enabled\);", text)
    for n in NAMES:
        assert n in _lib.declared_symbols()
        assert hasattr(L, n)
        assert getattr(L, n).restype is not None and len(getattr(L, n).argtypes) == 2


def test_api_exposes_the_mode():
    assert callable(api.neural_set_deterministic_training) and callable(api.neural_get_deterministic_training)


def test_null_volume_is_an_error_not_a_crash(L):
    import ctypes as C
    e = C.c_int(7)
    assert L.vnrAmdNeuralVolumeSetDeterministicTraining(None, 1) != 0
    assert L.vnrAmdNeuralVolumeGetDeterministicTraining(None, C.byref(e)) != 0


def test_train_tool_lists_deterministic():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vnr_cmd_train.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--deterministic" in out.stdout


def test_integration_section_6_lists_the_variable():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## 6."):]
    sec = sec[:sec.index("\n## ", 4)] if "\n## " in sec[4:] else sec
    assert "`VNR_AMD_DETERMINISTIC`" in sec
