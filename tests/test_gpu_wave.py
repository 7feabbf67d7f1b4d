"""The wave primitives of csrc/dt_wave.hpp on the device: lib/wave_selftest (source
tests/device/wave_selftest.hip, built by `make`) runs each of them on one full wave and compares
every lane with the sequential definition.  A CPU test checks that the header is the only place
that holds a DPP scan and that no kernel file defines a primitive of its own again."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "diamond-types_amd")
SELFTEST = os.path.join(PKG, "lib", "wave_selftest")

SHARED = ("lane", "lane_id", "rdl", "bcast", "ballot", "popc", "ctz", "first_lane", "lt_mask", "wave_scan", "wave_sum",
          "wave_fence", "utf8_len", "splitmix", "multmodp", "x2nmodp", "scan_incl")


def test_primitives_are_defined_in_the_header_only():
    hip = glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "tools", "*.hip"))
    assert len(hip) >= 9
    define = re.compile(r"^\s*(?:DEV|__device__|static|inline|template)\b[^;=(]*?\b(%s)\s*\([^;]*\)\s*\{" % "|".join(SHARED), re.M)
    for path in hip + glob.glob(os.path.join(ROOT, "tests", "device", "*.hip")):
        src = open(path).read()
        assert "__builtin_amdgcn_update_dpp" not in src, path
        assert not re.search(r"#\s*define\s+DEV\b", src), path
        assert not define.findall(src), (path, define.findall(src))
    hdr = open(os.path.join(PKG, "csrc", "dt_wave.hpp")).read()
    assert "__builtin_amdgcn_update_dpp" in hdr and define.findall(hdr)
    assert "csrc/dt_wave.hpp" in open(os.path.join(PKG, "Makefile")).read()


@pytest.mark.gpu
def test_wave_primitives_match_their_sequential_definitions():
    assert os.access(SELFTEST, os.X_OK), "run `make -C diamond-types_amd` (build() does)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=60)
    mismatches = [line for line in r.stdout.splitlines() if line.startswith("mismatch")]
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert mismatches == []
    assert re.search(r"wave_selftest: \d+ rounds of 64 lanes, 0 mismatches", r.stdout), r.stdout
