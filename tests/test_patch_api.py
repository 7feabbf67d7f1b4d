"""The batched patch encoder's interface (dtgpu_decode_encode_from, dtgpu_patches_*): declared in
dtgpu.h, exported by libdtgpu.so, argument checks that touch no device, and the Python mirror
(DecodeBatch.encode_from, PatchBatch).  (What the encoder writes is checked on the GPU,
test_gpu_patch.py.)"""
import ctypes
import os
import re

import dt_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 67
FUNCTIONS = ("dtgpu_decode_encode_from", "dtgpu_patches_size", "dtgpu_patches_result", "dtgpu_patches_get",
             "dtgpu_patches_free", "dtgpu_patches_profile")


def test_header_declares_the_functions():
    with open(os.path.join(ROOT, "include", "dtgpu.h")) as f:
        h = f.read()
    assert re.search(r"typedef struct dtgpu_patches dtgpu_patches;", h)
    assert re.search(r"dtgpu_status\s+dtgpu_decode_encode_from\s*\(\s*const dtgpu_decoded \*base,\s*const uint32_t \*doc,"
                     r"\s*const uint64_t \*versions,\s*const size_t \*version_off,\s*size_t n,\s*uint32_t flags,"
                     r"\s*float \*ms,\s*dtgpu_patches \*\*out\)", h)
    assert re.search(r"size_t\s+dtgpu_patches_size\s*\(\s*const dtgpu_patches \*p\)", h)
    assert re.search(r"dtgpu_status\s+dtgpu_patches_result\s*\(\s*const dtgpu_patches \*p,\s*size_t i,"
                     r"\s*uint64_t \*frontier,\s*size_t cap,\s*size_t \*n_frontier\)", h)
    assert re.search(r"dtgpu_status\s+dtgpu_patches_get\s*\(\s*const dtgpu_patches \*p,\s*size_t i,\s*uint8_t \*out,"
                     r"\s*size_t cap,\s*size_t \*out_len\)", h)
    assert re.search(r"void\s+dtgpu_patches_free\s*\(\s*dtgpu_patches \*p\)", h)
    assert re.search(r"dtgpu_status\s+dtgpu_patches_profile\s*\(\s*const dtgpu_patches \*p,\s*size_t i,\s*uint32_t out\[12\]\)", h)
    assert "encode_oplog.rs:404-747" in h[h.index("dtgpu_patches") - 2500:h.index("dtgpu_patches")]


def test_library_exports_the_functions():
    L = dt_amd.lib()
    for name in FUNCTIONS:
        assert getattr(L, name) is not None, name


def test_null_arguments_are_argument_errors():
    L = dt_amd.lib()
    out = ctypes.c_void_p()
    ms = ctypes.c_float()
    assert L.dtgpu_decode_encode_from(None, None, None, None, 0, 3, ctypes.byref(ms), ctypes.byref(out)) == ERR_ARG
    assert out.value is None
    assert L.dtgpu_decode_encode_from(None, None, None, None, 3, 3, None, None) == ERR_ARG
    assert L.dtgpu_patches_size(None) == 0
    k = ctypes.c_size_t(7)
    assert L.dtgpu_patches_result(None, 0, None, 0, ctypes.byref(k)) == ERR_ARG and k.value == 0
    k = ctypes.c_size_t(7)
    assert L.dtgpu_patches_get(None, 0, None, 0, ctypes.byref(k)) == ERR_ARG and k.value == 0
    prof = (ctypes.c_uint32 * 12)()
    assert L.dtgpu_patches_profile(None, 0, prof) == ERR_ARG
    L.dtgpu_patches_free(None)


def test_python_mirror_exists():
    assert callable(getattr(dt_amd.DecodeBatch, "encode_from", None))
    for name in ("__len__", "status", "frontier", "patch", "profile"):
        assert callable(getattr(dt_amd.PatchBatch, name, None)), name
    p = dt_amd.PatchBatch(None, 0, 1.5)
    assert len(p) == 0 and p.last_ms == 1.5


def test_ffi_crate_declares_the_functions():
    with open(os.path.join(ROOT, "crates", "dtgpu-sys", "src", "lib.rs")) as f:
        rs = f.read()
    assert "pub struct dtgpu_patches" in rs
    for name in FUNCTIONS:
        assert f"pub fn {name}(" in rs, name
