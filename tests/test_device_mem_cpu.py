"""csrc/er_mem.h, the one place of the library that allocates and frees device and page-locked host memory, through the stand-alone program
tests/cpp/device_mem_check.cpp (er_mem.h + er_common.cpp, nothing else of the library).  Without a HIP device the program checks what a failed
allocation leaves behind, and that run is repeated under AddressSanitizer and UBSan (host code, a program of its own); with a device it checks
the success path: a few kilobytes, well under a second."""
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
    out = os.path.join(tempfile.mkdtemp(prefix="er_device_mem_"), "device_mem_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
                   + list(extra) + [os.path.join(ROOT, "tests", "cpp", "device_mem_check.cpp"), os.path.join(CSRC, "er_common.cpp"), "-o", out],
                   check=True)
    return out


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "OK" and not any(l.startswith("FAIL") for l in lines), r.stdout + r.stderr
    return r


def test_device_mem_check_plain_and_sanitized_without_a_device():
    r = run(build())
    if r.stdout.startswith("no device"):
        s = run(build("-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"))
        assert s.stdout == r.stdout and "runtime error" not in s.stderr and "Sanitizer" not in s.stderr, s.stderr


@pytest.mark.gpu
def test_device_mem_check_success_path_on_the_card():
    r = run(build())
    assert "checking the success path" in r.stdout.splitlines()[0], r.stdout
