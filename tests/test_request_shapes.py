"""The HIP-free part of the request scaffold (csrc/dt_request_shape.hpp: the request validator, the
LV packer, FrontierSet::read) built with AddressSanitizer + UndefinedBehaviorSanitizer as a
stand-alone program (tests/sanitize/request_shapes.cpp) and run over the shapes the per-request
calls meet: an empty batch, requests of 0, 1, 64 and 65 LVs, LVs past 32 bits, CSRs that do not
start at 0, and reads at every cap.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diamond-types_amd", "csrc")


@pytest.fixture(scope="module")
def shapes_bin(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("san") / "request_shapes")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "sanitize", "request_shapes.cpp"), "-o", out])
    return out


def test_request_shapes(shapes_bin):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([shapes_bin], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.startswith("shapes ok ")
