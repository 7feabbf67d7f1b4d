"""The batched history projection's interface (dtgpu_decode_history, dtgpu_decode_history_result):
declared in dtgpu.h, exported by libdtgpu.so, argument checks that touch no device, and the Python
mirror on DecodeBatch.  (What the projection computes is checked on the GPU, test_gpu_history.py.)"""
import ctypes
import os
import re

import dt_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 67


def test_header_declares_both_functions():
    with open(os.path.join(ROOT, "include", "dtgpu.h")) as f:
        h = f.read()
    assert re.search(r"dtgpu_status\s+dtgpu_decode_history\s*\(\s*const dtgpu_decoded \*base,\s*const uint32_t \*doc,"
                     r"\s*const uint64_t \*versions,\s*const size_t \*version_off,\s*size_t n,\s*float \*ms,"
                     r"\s*dtgpu_decoded \*\*out\)", h)
    assert re.search(r"dtgpu_status\s+dtgpu_decode_history_result\s*\(\s*const dtgpu_decoded \*hist,\s*size_t i,"
                     r"\s*uint64_t \*frontier,\s*size_t cap,\s*size_t \*n_frontier\)", h)


def test_library_exports_both_functions():
    L = dt_amd.lib()
    assert L.dtgpu_decode_history is not None
    assert L.dtgpu_decode_history_result is not None


def test_null_arguments_are_argument_errors():
    L = dt_amd.lib()
    out = ctypes.c_void_p()
    ms = ctypes.c_float()
    assert L.dtgpu_decode_history(None, None, None, None, 0, ctypes.byref(ms), ctypes.byref(out)) == ERR_ARG
    assert L.dtgpu_decode_history(None, None, None, None, 3, None, None) == ERR_ARG
    assert out.value is None
    k = ctypes.c_size_t()
    assert L.dtgpu_decode_history_result(None, 0, None, 0, ctypes.byref(k)) == ERR_ARG


def test_python_mirror_exists():
    for name in ("history", "history_result", "checkout_versions"):
        assert callable(getattr(dt_amd.DecodeBatch, name, None)), name


def test_ffi_crate_declares_both_functions():
    with open(os.path.join(ROOT, "crates", "dtgpu-sys", "src", "lib.rs")) as f:
        rs = f.read()
    assert "pub fn dtgpu_decode_history(" in rs and "pub fn dtgpu_decode_history_result(" in rs
