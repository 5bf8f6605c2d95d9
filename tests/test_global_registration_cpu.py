"""bin/GlobalRegistration without a GPU: the host-only header csrc/host/er_globalreg.h compiled with g++ (tests/hostcheck/globalreg_check.cpp)
-- the alignment.config parser against formats.load_alignment_config, the three trajectory constructions of the odometry mode against
numpy, the acceptance rule of align_redux at its edges, the float32 inverse against icp.inverse4f -- the program's usage text and its exit
where there is no device, and the new entry point at the C ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from elasticreconstruction_amd import _ffi, formats
from elasticreconstruction_amd.icp import inverse4f

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elasticreconstruction_amd", "bin", "GlobalRegistration")
BOOLS = ("visualization", "aux_data", "estimate_normal", "smart_swap")
INTS = ("max_iteration", "num_of_samples", "correspondence_randomness", "pcl_verbose", "inlier_number")
FLOATS = ("edge_similarity", "resample_leaf", "max_correspondence_distance", "inlier_fraction", "angle_difference", "normal_radius", "feature_radius")
_cache = {}


def hostlib():
    if "lib" not in _cache:
        src = os.path.join(ROOT, "tests", "hostcheck", "globalreg_check.cpp")
        inc = os.path.join(ROOT, "elasticreconstruction_amd", "csrc", "host")
        out = os.path.join(ROOT, "tests", "hostcheck", "_build", "libglobalreg_check.so")
        deps = [src, os.path.join(inc, "er_globalreg.h"), os.path.join(inc, "er_formats.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I" + inc, src, "-o", out, "-lz"], check=True)
        L = C.CDLL(out)
        L.gr_segment_entries_needed.restype = C.c_long
        _cache["lib"] = L
    return _cache["lib"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def h_config(path):
    b, i, f = np.zeros(4, np.int32), np.zeros(5, np.int32), np.zeros(7, np.float32)
    why = C.create_string_buffer(256)
    rc = hostlib().gr_load_config(str(path).encode(), _p(b), _p(i), _p(f), why, 256)
    cfg = dict(zip(BOOLS, (bool(v) for v in b)))
    cfg.update(zip(INTS, (int(v) for v in i)))
    cfg.update(zip(FLOATS, f))
    return rc, cfg, why.value.decode()


def same_config(cfg, ref):
    for k in BOOLS + INTS:
        assert cfg[k] == ref[k] and type(cfg[k]) is type(ref[k]), k
    for k in FLOATS:
        assert cfg[k] == np.float32(ref[k]), k                                              # the reference's fields are floats


def test_config_parser_equals_load_alignment_config(tmp_path):
    golden = os.path.join(ROOT, "tests", "golden", "alignment.config")
    rc, cfg, _ = h_config(golden)
    assert rc == 0
    same_config(cfg, formats.load_alignment_config(golden))
    same_config(cfg, formats.ALIGNMENT_DEFAULTS)                                            # the shipped file holds the defaults
    odd = tmp_path / "alignment.config"
    odd.write_text("max_iteration=200000\ninlier_fraction = 0.2 \nno equals sign here\n\nunknown_key=17\nsmart_swap=True\nestimate_normal=false\n"
                   "aux_data=true\nvisualization=yes\npcl_verbose=0\nedge_similarity=0.5=\nnum_of_samples=6\r\n")
    rc, cfg, why = h_config(odd)
    assert rc == -1 and "edge_similarity" in why                                            # a number that does not parse: formats raises on it too
    with pytest.raises(ValueError):
        formats.load_alignment_config(str(odd))
    odd.write_text(odd.read_text().replace("edge_similarity=0.5=\n", "edge_similarity=0.5\n"))
    rc, cfg, _ = h_config(odd)
    ref = formats.load_alignment_config(str(odd))
    assert rc == 0
    same_config(cfg, ref)
    assert (cfg["max_iteration"], cfg["num_of_samples"], cfg["pcl_verbose"]) == (200000, 6, 0) and cfg["inlier_fraction"] == np.float32(0.2)
    assert cfg["aux_data"] is True and cfg["estimate_normal"] is False
    assert cfg["smart_swap"] is False and cfg["visualization"] is False                     # only the spelling `true` is true
    assert cfg["inlier_number"] == 30000 and cfg["resample_leaf"] == np.float32(0.05)       # untouched keys keep their defaults
    rc, cfg, _ = h_config(tmp_path / "nothing_here.config")
    assert rc == 1
    same_config(cfg, formats.load_alignment_config(None))


def np_trajectories(seg, fragment, num):
    """GlobalRegistration.cpp:197-225 in numpy: (init, pose, odometry) as lists of (id1, id2, frame, T)."""
    init, base = [], np.eye(4)
    for i, S in enumerate(seg):
        if i % fragment == 0 and i > 0:
            base = init[i - 1][3] @ np.linalg.inv(S)
        init.append((i, i, i + 1, base @ S))
    pose = [(i // fragment, i // fragment, i // fragment + 1, init[i][3] @ np.linalg.inv(seg[0])) for i in range(0, len(init), fragment)]
    odo = [(i - 1, i, num, np.linalg.inv(pose[i - 1][3]) @ pose[i][3]) for i in range(1, num)]
    return init, pose, odo


def poses(n, seed):
    from elasticreconstruction_amd import synth
    g = np.random.default_rng(seed)
    out, T = [], synth.perturbation(seed, 40.0, 1.0)
    for i in range(n):
        out.append(T.copy())
        T = T @ synth.perturbation(int(g.integers(1 << 30)), 5.0, 0.05)
    return np.array(out)


@pytest.mark.parametrize("n_seg,fragment,num", ((4, 1, 4), (15, 5, 3), (11, 5, 3), (17, 7, 3), (11, 5, 2)))
def test_trajectory_constructions_equal_numpy(n_seg, fragment, num):
    """Segment lengths 1 and 5, logs the length divides and logs it does not (11 = 2 * 5 + 1 is the shortest log three fragments of 5 can
    have; 17 poses in fragments of 7 end inside the third), and fewer fragments than the log holds."""
    L = hostlib()
    seg = poses(n_seg, 3 * n_seg + fragment)
    assert L.gr_segment_entries_needed(num, fragment) == (num - 1) * fragment + 1 <= n_seg
    counts = np.zeros(3, np.int32)
    ids = [np.zeros((n_seg, 3), np.int32) for _ in range(3)]
    Ts = [np.zeros((n_seg, 4, 4)) for _ in range(3)]
    L.gr_trajectories(n_seg, _p(np.ascontiguousarray(seg)), fragment, num, _p(counts), _p(ids[0]), _p(Ts[0]), _p(ids[1]), _p(Ts[1]), _p(ids[2]), _p(Ts[2]))
    ref = np_trajectories(seg, fragment, num)
    assert list(counts) == [len(r) for r in ref] == [n_seg, (n_seg + fragment - 1) // fragment, num - 1]
    for which in range(3):
        for row, (a, b, f, T) in enumerate(ref[which]):
            assert tuple(ids[which][row]) == (a, b, f), (which, row)
            assert np.abs(Ts[which][row] - T).max() < 1e-12, (which, row)                   # cofactor against LAPACK inverses of well-conditioned poses
    assert np.abs(Ts[0][0] - seg[0]).max() == 0 and np.abs(Ts[1][0] - np.eye(4)).max() < 1e-12


def test_acceptance_rule_at_its_edges():
    acc = hostlib().gr_redux_accepted
    acc.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int]
    huge = 1 << 30
    for count, n in ((33, 100), (1, 3), (2311, 7003), (1, 1)):
        f = np.float32(count) / np.float32(n)
        assert acc(count, n, f, huge) == 1                                                  # count / n == inlier_fraction exactly
        assert acc(count, n, np.nextafter(f, np.float32(2)), huge) == 0
        assert acc(count - 1, n, f, huge) == 0
    assert acc(30000, 100000, 0.33, 30000) == 0                                             # count == inlier_number: not more than it
    assert acc(30001, 100000, 0.33, 30000) == 1
    assert acc(0, 100, 0.0, -1) == 0                                                        # no inlier: the error is not below FLT_MAX
    assert acc(1, 100, 0.0, huge) == 1


def test_float32_inverse_equals_its_python_restatement():
    L = hostlib()
    from elasticreconstruction_amd import synth
    g = np.random.default_rng(9)
    for t in range(200):
        M = synth.perturbation(t, 180.0, 3.0).astype(np.float32) if t % 2 else g.normal(size=(4, 4)).astype(np.float32)
        out = np.zeros((4, 4), np.float32)
        assert L.gr_inverse4f(_p(np.ascontiguousarray(M)), _p(out)) == 1
        assert np.array_equal(out.view(np.uint32), inverse4f(M).view(np.uint32)), t
        assert np.abs(out.astype(np.float64) @ M - np.eye(4)).max() < (1e-5 if t % 2 else 1e-2)
    out = np.full((4, 4), 7, np.float32)
    assert L.gr_inverse4f(_p(np.zeros((4, 4), np.float32)), _p(out)) == 0 and (out == 7).all()


def test_program_prints_its_usage_without_arguments():
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage" in r.stdout and "<dir> <100-0.log> <segment_length>" in r.stdout


def test_program_refuses_to_run_without_a_device(tmp_path):
    import torch
    if torch.cuda.is_available():
        return                                                                              # (tests/test_global_registration_program_gpu.py runs it there)
    (tmp_path / "frags").mkdir()
    r = subprocess.run([BIN, str(tmp_path / "frags") + "/"], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode != 0 and "no HIP device available" in r.stderr
    assert "0 detected." in r.stdout and "alignment.config not found! Use default parameters." in r.stdout
    assert not (tmp_path / "result.txt").exists()


def test_batch_entry_point_is_declared_bound_and_refuses_without_a_device():
    hdr = open(os.path.join(ROOT, "include", "er_hip.h")).read()
    L = _ffi.lib()
    assert "er_ransac_align_batch(" in hdr and "er_ransac_align_batch" in _ffi.SYMBOLS and hasattr(L, "er_ransac_align_batch")
    p = _ffi.ErRansacParams()
    assert L.er_ransac_params_default(C.byref(p)) == 0
    assert L.er_ransac_align_batch(0, None, None, None, None, C.byref(p), None, 0, None, None, None, None, None, None, None) == 0   # nothing to do
    import torch
    if torch.cuda.is_available():
        return
    assert L.er_ransac_align_batch(1, None, None, None, None, C.byref(p), None, 0, None, None, None, None, None, None, None) != 0
    assert "no HIP device" in L.er_last_error().decode()
