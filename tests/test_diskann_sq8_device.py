"""CPU checks of the device-side medoid / SQ8 entry points (include/hip_diskann_bridge.h): the four names
are declared in the header and exported by the built library, and each refuses a NULL handle with its documented
return value and a message — before it touches a device, so this runs on a machine without one."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HDR = ROOT / "include" / "hip_diskann_bridge.h"
NAMES = ("diskann_hip_medoid", "diskann_hip_quantize_sq8", "diskann_hip_export_sq8",
         "diskann_hip_quantize_phase_seconds")


@pytest.fixture(scope="module")
def L(hipann_mod):
    return hipann_mod.lib()


@pytest.mark.parametrize("name", NAMES)
def test_declared_and_exported(L, name):
    text = re.sub(r"/\*.*?\*/", "", HDR.read_text(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in {HDR.name}"
    assert hasattr(L, name), f"{name} is not exported by libhipann.so"


def test_quantize_refuses_null(L):
    eb = C.create_string_buffer(256)
    h = L.diskann_hip_quantize_sq8(None, eb, 256)
    assert not h
    assert eb.value.strip() != b""
    # no error buffer: still NULL, nothing written
    assert not L.diskann_hip_quantize_sq8(None, None, 0)


def test_medoid_refuses_null(L):
    eb = C.create_string_buffer(256)
    row = C.c_uint32(77)
    assert L.diskann_hip_medoid(None, C.byref(row), eb, 256) == -1
    assert eb.value.strip() != b""
    assert row.value == 77


def test_export_refuses_null(L):
    eb = C.create_string_buffer(256)
    assert L.diskann_hip_export_sq8(None, None, None, None, eb, 256) == -1
    assert eb.value.strip() != b""


def test_phase_seconds_refuses_null(L):
    sec = (C.c_double * 3)(1.0, 2.0, 3.0)
    assert L.diskann_hip_quantize_phase_seconds(None, sec) == -1
    assert list(sec) == [1.0, 2.0, 3.0]
