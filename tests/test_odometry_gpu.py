"""Depth odometry on the GPU (csrc/er_odom.hip) against the numpy restatement (tests/odometry_restatement.py): the maps bit for
bit, the sums of one linearisation within the bound of two summation orders, every traced iteration step by step, the independence of a
pair's result from the list, the window and the run, the end-to-end trajectory, the refusals and bin/DepthOdometry.  Sizes: 72 x 52 (levels
36 x 26 and 18 x 13: rows that are no multiple of a wave, a coarsest level smaller than one workgroup) and 160 x 120."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import odometry_restatement as orr
from odometry_cases import same_bits, scene
from elasticreconstruction_amd import _ffi, formats, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(72, 52), (160, 120)]
_cache = {}


def device_odometry(cols, rows, cam, **params):
    from elasticreconstruction_amd import DepthOdometry
    key = (cols, rows, tuple(float(np.float32(k)) for k in cam), tuple(sorted(params.items())))
    if key not in _cache:
        _cache[key] = DepthOdometry(cols, rows, cam, **params)
    return _cache[key]


def restatement(cols, rows, cam, **params):
    """The restatement with the LIBRARY's tables and default parameters (tests/test_odometry_cpu.py pins both)."""
    from elasticreconstruction_amd import odometry
    p = odometry.default_params()
    p.update(params)
    return orr.Odometry(cols, rows, cam, tables_=odometry.tables(), **p)


def rest_maps(cols, rows, n=4):
    key = ("maps", cols, rows, n)
    if key not in _cache:
        d, W, cam = scene(cols, rows, n)
        od = restatement(cols, rows, cam)
        _cache[key] = [od.maps(f) for f in d]
    return _cache[key]


# ---- maps -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,rows", SIZES)
def test_maps_equal_the_restatement(gpu, cols, rows):
    d, W, cam = scene(cols, rows)
    holed = d[0].copy()
    holed[rows // 4:rows // 2, cols // 3:cols // 3 + 11] = 0
    far = (int(d[0][d[0] > 0].min()) + int(d[0].max())) // 2         # cuts the far wall, keeps the sphere
    cases = [(d[0], {}), (holed, {}), (d[0], dict(max_depth_mm=far)), (np.zeros_like(d[0]), {}), (d[1], dict(bilateral=0))]
    for frame, params in cases:
        dev, ref = device_odometry(cols, rows, cam, **params), restatement(cols, rows, cam, **params)
        want = ref.maps(frame)
        for level in range(3):
            dd, V, N = dev.maps(frame, level)
            wd, wV, wN = want[level]
            assert np.array_equal(dd, wd), (params, level)
            assert same_bits(V, wV) and same_bits(N, wN), (params, level)
        if params.get("max_depth_mm"):
            assert want[0][0].max() <= far and (want[0][0] > 0).any() and (want[0][0] == 0).sum() > (d[0] == 0).sum()
    assert np.isnan(dev.maps(np.zeros_like(d[0]), 2)[1]).all()
    # frames that are already on the device give the same maps
    import torch
    t = torch.from_numpy(d[0].astype(np.int16)).to(gpu)
    a, b = device_odometry(cols, rows, cam).maps(t, 1), device_odometry(cols, rows, cam).maps(d[0], 1)
    assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2])


# ---- one linearisation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,rows", SIZES)
def test_linearize_count_is_exact_and_sums_are_within_the_bound_of_two_summation_orders(gpu, cols, rows):
    d, W, cam = scene(cols, rows)
    dev, ref, m = device_odometry(cols, rows, cam), restatement(cols, rows, cam), rest_maps(cols, rows)
    G = np.linalg.inv(W[0]) @ W[1]
    for name, T in (("identity", np.eye(4)), ("ground truth", G), ("perturbed", G @ synth.perturbation(7, 3.0, 0.03))):
        for level in range(3):
            sums, count = dev.linearize(d[0], d[1], level, T)
            want, wcount, wabs = ref.linearize(m[0], m[1], level, T, with_abs=True)
            print("%d x %d %s level %d: count %d, worst |difference| / bound %.3g" % (
                cols, rows, name, level, count, np.max(np.abs(sums - want) / np.maximum(wcount * 2.0 ** -53 * wabs, 1e-300))))
            assert count == wcount and count > 0, (name, level, count, wcount)
            assert np.all(np.abs(sums - want) <= wcount * 2.0 ** -53 * wabs), (name, level)


# ---- every iteration of a traced pair ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,rows", SIZES)
def test_every_traced_iteration_is_one_restatement_step_from_the_device_state(gpu, cols, rows):
    d, W, cam = scene(cols, rows)
    dev, ref, m = device_odometry(cols, rows, cam), restatement(cols, rows, cam), rest_maps(cols, rows)
    T, status, trace, sums = dev.align_pairs(d, [0], [1], trace=True, sums=True)
    assert status[0] == 0 and trace.shape == (1, 19, 17) and ref.schedule() == [2] * 4 + [1] * 5 + [0] * 10
    state = np.eye(4)
    for k, level in enumerate(ref.schedule()):
        s, count = ref.linearize(m[0], m[1], level, state)
        assert count == int(trace[0, k, 16]), (k, count, trace[0, k, 16])
        step, lost = ref.step(s, count, state)
        assert not lost and np.abs(step - trace[0, k, :16].reshape(4, 4)).max() <= 1e-6, k
        state = trace[0, k, :16].reshape(4, 4)
    assert np.array_equal(T[0], state)
    s, count, sabs = ref.linearize(m[0], m[1], 0, trace[0, -2, :16].reshape(4, 4), with_abs=True)      # `sums`: the last iteration's
    assert np.all(np.abs(sums[0] - s) <= count * 2.0 ** -53 * sabs)


# ---- a pair's result does not depend on the list, the order, the window or the run ------------------------------------------------------------
def test_list_independence(gpu):
    cols, rows = 72, 52
    d, W, cam = scene(cols, rows)
    depth = np.concatenate([d, np.zeros((1, rows, cols), np.uint16)])             # frame 4: all zero
    dev = device_odometry(cols, rows, cam)
    guess = np.linalg.inv(W[1]) @ W[2] @ synth.perturbation(5, 1.0, 0.01)
    #        unequal pairs            (i, i)  against the zero frame  repeated  with a guess
    pairs = [(0, 1), (1, 0), (0, 3), (2, 2), (0, 4), (4, 1),         (0, 1),   (1, 2)]
    guesses = np.stack([np.eye(4)] * 7 + [guess])
    mi, fi = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    single = [dev.align_pairs(depth, [a], [b], guess=guesses[k:k + 1], trace=True, sums=True) for k, (a, b) in enumerate(pairs)]
    sT, sS, sTr, sSu = (np.concatenate([s[q] for s in single]) for q in range(4))
    assert list(sS) == [0, 0, 0, 0, 1, 1, 0, 0]
    assert np.isfinite(sT).all() and np.array_equal(sT[4], np.eye(4)) and np.array_equal(sT[5], np.eye(4))      # lost: the last good pose, no NaN
    assert np.array_equal(sT[3], np.eye(4)) and np.array_equal(sT[0], sT[6]) and not np.array_equal(sT[0], sT[2])
    assert orr.pose_error(sT[7], np.linalg.inv(W[1]) @ W[2])[0] < 0.2
    order = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    for window in (2, 3, 5, 0):
        for perm in (np.arange(8), order):
            for run in range(2):
                T, S, Tr, Su = dev.align_pairs(depth, mi[perm], fi[perm], guess=guesses[perm], window=window, trace=True, sums=True)
                what = (window, list(perm), run)
                assert np.array_equal(S, sS[perm]), what
                assert np.array_equal(T.view(np.uint64), sT[perm].view(np.uint64)), what
                assert np.array_equal(Tr.view(np.uint64), sTr[perm].view(np.uint64)), what
                assert np.array_equal(Su.view(np.uint64), sSu[perm].view(np.uint64)), what


@pytest.mark.parametrize("cols,rows", SIZES)
def test_track_is_align_pairs_on_consecutive_frames_from_host_or_device_memory(gpu, cols, rows):
    import torch
    d, W, cam = scene(cols, rows)
    dev = device_odometry(cols, rows, cam)
    T, S = dev.track(d)
    T2, S2 = dev.align_pairs(d, [0, 1, 2], [1, 2, 3])
    assert T.shape == (3, 4, 4) and np.array_equal(T.view(np.uint64), T2.view(np.uint64)) and np.array_equal(S, S2) and not S.any()
    t = torch.from_numpy(d.astype(np.int16)).to(gpu)
    for window in (0, 2):
        T3, S3 = dev.track(t, window=window)
        assert np.array_equal(T.view(np.uint64), T3.view(np.uint64)) and np.array_equal(S, S3)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
def test_eight_frames_stay_closer_to_the_restatement_than_the_restatement_is_to_the_truth(gpu):
    from elasticreconstruction_amd import accumulate
    cols, rows = 160, 120
    d, W, cam = scene(cols, rows, 8)
    dev, ref = device_odometry(cols, rows, cam), restatement(cols, rows, cam)
    T, S = dev.track(d)
    rT, rlost = ref.track(d)
    assert not S.any() and not rlost.any()
    for i in range(7):
        G = np.linalg.inv(W[i]) @ W[i + 1]
        dr, dt = orr.pose_error(T[i], rT[i])
        gr, gt = orr.pose_error(rT[i], G)
        print("pair %d: device - restatement %.3g deg %.3g mm; restatement - truth %.3g deg %.3g mm" % (i, dr, dt * 1e3, gr, gt * 1e3))
        assert dr < gr and dt < gt, i
    A, rA = accumulate(T, W[0]), orr.accumulate(rT, W[0])
    for i in range(1, 8):
        dr, dt = orr.pose_error(A[i], rA[i])
        gr, gt = orr.pose_error(rA[i], W[i])
        assert dr < gr and dt < gt, i


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_or_the_pair(gpu):
    from elasticreconstruction_amd import DepthOdometry
    cols, rows = 72, 52
    d, W, cam = scene(cols, rows)
    with pytest.raises(_ffi.ErError, match="cols = 70"):
        DepthOdometry(70, 52, cam)
    with pytest.raises(_ffi.ErError, match="rows = 50"):
        DepthOdometry(72, 50, cam)
    DepthOdometry(70, 50, cam, levels=2).close()                                  # divisible by 2^(levels-1) = 2
    for levels in (0, 5, -1):
        with pytest.raises(_ffi.ErError, match="levels = %d" % levels):
            DepthOdometry(cols, rows, cam, levels=levels)
    dev = device_odometry(cols, rows, cam)
    with pytest.raises(_ffi.ErError, match="n_frames = 1"):
        dev.track(d[:1])
    with pytest.raises(_ffi.ErError, match=r"pair 1 names frames \(4, 0\)"):
        dev.align_pairs(d, [0, 4], [1, 0])
    with pytest.raises(_ffi.ErError, match=r"pair 2 names frames \(1, -1\)"):
        dev.align_pairs(d, [0, 1, 1], [1, 2, -1])
    for window in (1, -3):
        with pytest.raises(_ffi.ErError, match="window = %d" % window):
            dev.align_pairs(d, [0], [1], window=window)
        with pytest.raises(_ffi.ErError, match="window = %d" % window):
            dev.track(d, window=window)
    L = _ffi.lib()
    flat = np.ascontiguousarray(d).reshape(4, -1)
    mi, fi, T, S = np.array([0], np.int32), np.array([1], np.int32), np.zeros(16), np.zeros(1, np.int32)
    p = _ffi.ptr
    for args, text in (((dev._h, 4, p(flat), 0, 1, p(mi), p(fi), None, None, p(S), None, None, 0), "T_out is NULL"),
                       ((dev._h, 4, p(flat), 0, 1, p(mi), p(fi), None, p(T), None, None, None, 0), "status is NULL"),
                       ((dev._h, 4, None, 0, 1, p(mi), p(fi), None, p(T), p(S), None, None, 0), "depth is NULL"),
                       ((dev._h, 4, p(flat), 0, 1, None, p(fi), None, p(T), p(S), None, None, 0), "model_idx or frame_idx is NULL")):
        assert L.er_odom_align_pairs(*args) != 0 and text in L.er_last_error().decode()
    assert L.er_odom_track(dev._h, 4, p(flat), 0, None, p(np.zeros(3, np.int32)), 0) != 0 and "T_rel is NULL" in L.er_last_error().decode()
    assert L.er_odom_track(dev._h, 4, p(flat), 0, p(np.zeros(48)), None, 0) != 0 and "status is NULL" in L.er_last_error().decode()
    assert L.er_odom_linearize(dev._h, p(flat), 0, 0, p(np.eye(4)), None, C.byref(C.c_int())) != 0 and "sums is NULL" in L.er_last_error().decode()
    assert L.er_odom_linearize(dev._h, p(flat), 0, 0, p(np.eye(4)), p(np.zeros(27)), None) != 0 and "count is NULL" in L.er_last_error().decode()
    cam4 = np.array(cam, np.float32)
    assert L.er_odom_create(cols, rows, cam4.ctypes.data_as(C.POINTER(C.c_float)), None, 0, None) != 0 and "out is NULL" in L.er_last_error().decode()
    # after every refusal the handle still works
    assert dev.align_pairs(d, [0], [1])[1][0] == 0


# ---- the program --------------------------------------------------------------------------------------------------------------------------------
def test_program_writes_the_log_the_python_route_writes(gpu, tmp_path):
    from elasticreconstruction_amd import accumulate
    cols, rows = 160, 120
    d, W, cam = scene(cols, rows, 8)
    d = d[:6]
    tmp = str(tmp_path)
    d.tofile(os.path.join(tmp, "frames.raw"))
    cam32 = np.array(cam, np.float32)
    with open(os.path.join(tmp, "cam.param"), "w") as f:
        f.write("".join("%.9g\n" % float(x) for x in list(cam32) + [2.5, 2.5]))
    dev = device_odometry(cols, rows, tuple(cam32))
    exe = os.path.join(ROOT, "elasticreconstruction_amd", "bin", "DepthOdometry")
    for interval in (0, 3):
        out = os.path.join(tmp, "traj_%d.log" % interval)
        cmd = [exe, "--cols", str(cols), "--rows", str(rows), "--depth_raw", "frames.raw", "--camera", "cam.param", "--traj_log", out]
        if interval:
            cmd += ["--interval", str(interval)]
        r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        T, S = dev.track(d)
        assert not S.any()
        if interval:
            poses = np.concatenate([accumulate(T[s:s + interval - 1]) for s in range(0, 6, interval)])
        else:
            poses = accumulate(T)
        assert poses.shape == (6, 4, 4)
        want = os.path.join(tmp, "want_%d.log" % interval)
        formats.save_log(want, [formats.FramedTransformation(i, i, i + 1, poses[i]) for i in range(6)])
        assert open(out, "rb").read() == open(want, "rb").read(), interval
        got = formats.load_log(out)
        assert len(got) == 6 and np.array_equal(got[0].T, np.eye(4))
        if interval:
            assert np.array_equal(got[3].T, np.eye(4)) and not np.array_equal(got[4].T, np.eye(4))
