"""The fragment builder without a GPU: the C ABI of er_tsdf_raycast_batch, er_frames_to_models_align and the er_frag_ family,
their defaults and refusals, bin/MakeFragments' command line, and the C++ statement of the kinfu base pose against synth.basepose."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from elasticreconstruction_amd import _ffi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "elasticreconstruction_amd", "bin", "MakeFragments")
NEW = ["er_frag_build", "er_frag_count", "er_frag_create", "er_frag_destroy", "er_frag_lane_bytes", "er_frag_params_default", "er_frag_read",
       "er_frames_to_models_align", "er_tsdf_raycast_batch"]


def last_error():
    return _ffi.lib().er_last_error().decode()


def test_header_binding_and_library_agree_on_the_new_symbols():
    txt = open(os.path.join(ROOT, "include", "er_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    header = set(re.findall(r"\b(er_[a-z0-9_]+)\s*\(", txt))
    L = _ffi.lib()
    for s in NEW:
        assert s in header and s in _ffi.SYMBOLS and hasattr(L, s), s
    assert sorted(s for s in header if s.startswith("er_frag_")) == [s for s in NEW if s.startswith("er_frag_")]
    import elasticreconstruction_amd as pkg
    assert pkg.FragmentBuilder is not None and "FragmentBuilder" in pkg.__all__
    from elasticreconstruction_amd import tsdf
    assert callable(tsdf.raycast_batch)


def test_default_parameters():
    from elasticreconstruction_amd import fragments
    p = fragments.default_params()
    assert p["interval"] == 50 and p["lanes"] == 8 and p["max_units"] == 512 and p["length"] == np.float32(3.0)
    assert p["raycast"] == (np.float32(0.0), np.float32(4.0), np.float32(0.8) * np.float32(0.03))
    assert _ffi.lib().er_frag_params_default(None) != 0 and "NULL" in last_error()


def test_null_arguments_are_refused_with_a_message():
    L = _ffi.lib()
    h = C.c_void_p()
    assert L.er_frag_create(160, 120, None, None, None, 0, None) != 0 and "out is NULL" in last_error()
    assert L.er_frag_build(None, 1, None, 0, None, 1, None, None) != 0 and "NULL handle" in last_error()
    assert L.er_frag_count(None, None) != 0 and "NULL" in last_error()
    assert L.er_frag_read(None, 0, None, None, 0, None) != 0 and "NULL" in last_error()
    assert L.er_frag_lane_bytes(None, None) != 0 and "NULL" in last_error()
    assert L.er_frag_destroy(None) == 0
    assert L.er_tsdf_raycast_batch(1, None, None, None, None, None, None, None, None) != 0 and "NULL argument" in last_error()
    assert L.er_tsdf_raycast_batch(-1, None, None, None, None, None, None, None, None) != 0 and "negative" in last_error()
    assert L.er_tsdf_raycast_batch(65536, None, None, None, None, None, None, None, None) != 0 and "65535" in last_error()
    assert L.er_tsdf_raycast_batch(0, None, None, None, None, None, None, None, None) == 0, "no job: a no-op, with or without a device"
    # parameter refusals come before the device is looked for
    for field, value, word in (("interval", 0, "interval"), ("lanes", 0, "lanes"), ("lanes", 65, "lanes"), ("max_units", 0, "max_units")):
        p = _ffi.ErFragParams()
        L.er_frag_params_default(C.byref(p))
        setattr(p, field, value)
        assert L.er_frag_create(160, 120, None, None, C.byref(p), 0, C.byref(h)) != 0 and word in last_error() and not h.value


def test_constructors_refuse_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from elasticreconstruction_amd import FragmentBuilder
    with pytest.raises(_ffi.ErError, match="no HIP device"):
        FragmentBuilder(160, 120, None, interval=4, lanes=2, max_units=64)
    L = _ffi.lib()
    one = np.zeros(1, np.int32)
    assert L.er_frames_to_models_align(None, 1, None, 1, _ffi.ptr(one), 0, _ffi.ptr(one), None, None, None, None, None, 0) != 0
    assert "no HIP device" in last_error()


def test_program_help_and_command_line_refusals(tmp_path):
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--depth_raw" in r.stdout and "--lanes" in r.stdout and "--seg_log" in r.stdout
    d = str(tmp_path)
    np.zeros((2, 120 * 160), np.uint16).tofile(os.path.join(d, "frames.raw"))
    open(os.path.join(d, "list.txt"), "w").close()
    size = ["--cols", "160", "--rows", "120"]
    both = subprocess.run([EXE, "--depth_raw", "frames.raw", "--depth_list", "list.txt", "--dir", "out"] + size, cwd=d, capture_output=True, text=True, timeout=60)
    assert both.returncode != 0 and "one of --depth_raw and --depth_list" in both.stderr
    neither = subprocess.run([EXE, "--dir", "out"] + size, cwd=d, capture_output=True, text=True, timeout=60)
    assert neither.returncode != 0 and "one of --depth_raw and --depth_list" in neither.stderr
    nodir = subprocess.run([EXE, "--depth_raw", "frames.raw"] + size, cwd=d, capture_output=True, text=True, timeout=60)
    assert nodir.returncode != 0 and "--dir is required" in nodir.stderr
    assert sorted(os.listdir(d)) == ["frames.raw", "list.txt"], "a refused run writes nothing"


def test_program_refuses_without_a_gpu_and_writes_nothing(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    d = str(tmp_path)
    np.zeros((2, 120 * 160), np.uint16).tofile(os.path.join(d, "frames.raw"))
    r = subprocess.run([EXE, "--depth_raw", "frames.raw", "--dir", d, "--cols", "160", "--rows", "120"], cwd=d, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
    assert sorted(os.listdir(d)) == ["frames.raw"]


@pytest.mark.parametrize("length", [3.0, 2.5, 0.7])
def test_cpp_base_pose_equals_synth_basepose_bit_for_bit(length):
    src = os.path.join(ROOT, "tests", "hostcheck", "basepose_check.cpp")
    inc = os.path.join(ROOT, "elasticreconstruction_amd", "csrc")
    out = os.path.join(ROOT, "tests", "hostcheck", "_build", "basepose_check")
    deps = [src, os.path.join(inc, "er_mat4.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + inc, src, "-o", out], check=True)
    r = subprocess.run([out, repr(length)], capture_output=True, text=True, check=True, timeout=60)
    got = np.array([int(x, 16) for x in r.stdout.split()], np.uint64).reshape(4, 4)
    assert np.array_equal(got, synth.basepose(length).view(np.uint64))
