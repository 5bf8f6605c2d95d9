"""csrc/er_compact.h, the one statement of the two-pass stable compaction, through the stand-alone program tests/cpp/compact_check.cpp
(er_compact.h + er_common.cpp, nothing else of the library).  Without a HIP device the program checks the host's prefix over block counts (n = 0
and 1, strides 1 to 3, two lists in one object, a total above 2^31, side-tally sums) and what a failed allocation leaves behind, and that run is
repeated under AddressSanitizer and UBSan (host code, a program of its own); with a device its own kernel drives the block helper through both
passes with one and with three tallies at the wave and block edges: a few kilobytes, well under a second."""
import functools
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elasticreconstruction_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@functools.lru_cache(maxsize=None)
def build(*extra):
    out = os.path.join(tempfile.mkdtemp(prefix="er_compact_"), "compact_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
                   + list(extra) + ["-x", "hip", os.path.join(ROOT, "tests", "cpp", "compact_check.cpp"), os.path.join(CSRC, "er_common.cpp"), "-o", out],
                   check=True)
    return out


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "OK" and not any(l.startswith("FAIL") for l in lines), r.stdout + r.stderr
    return r


def test_compact_check_plain_and_sanitized_without_a_device():
    r = run(build())
    if r.stdout.startswith("no device"):
        assert "total above 2^31" in r.stdout and "leaves the object empty" in r.stdout, r.stdout
        s = run(build("-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"))
        assert s.stdout == r.stdout and "runtime error" not in s.stderr and "Sanitizer" not in s.stderr, s.stderr


@pytest.mark.gpu
def test_compact_check_both_passes_on_the_card():
    r = run(build())
    lines = r.stdout.splitlines()
    assert "checking both passes on the card" in lines[0], r.stdout
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 513):
        for tallies in ("1 tally", "3 tallies"):
            for pattern in ("every third kept", "all kept"):
                assert "ok    %s, n = %d, %s" % (tallies, n, pattern) in lines, r.stdout
