"""Frame-to-model alignment on the GPU (er_frame_to_model_align, DepthOdometry.align_model / track_model): the model side of
a pair is the resident volume ray-cast from a pose.  Held to the restatement route -- odometry_restatement.Odometry.align_maps on the maps of
raycast_restatement -- by the bars of tests/test_odometry_gpu.py: per-iteration counts exact, every traced step within 1e-6 per entry of the
restatement's step from the device's previous state, the last iteration's sums within N 2^-53 sum |terms|.

track_model beside track on 6 frames of the scene at 320 x 240, errors against the renderer's ground truth (measured on MI355X; both series
are in profiles/raycast.txt): the bar per frame is twice track's error plus half a voxel (2.93 mm; for the rotation, the angle half a voxel
subtends at 1 m, 0.168 degrees) -- the margin is for the voxel lattice, which frame-to-frame tracking never sees."""
import ctypes as C
import math

import numpy as np
import pytest

import odometry_restatement as orr
import raycast_cases as rcc
import raycast_restatement as rcr
from odometry_cases import same_bits
from elasticreconstruction_amd import _ffi
from elasticreconstruction_amd.tsdf import TSDFVolume, mat4_mul

pytestmark = pytest.mark.gpu
COLS, ROWS = rcc.SCENE_COLS, rcc.SCENE_ROWS
_cache = {}


def device_odometry(cam, **params):
    from elasticreconstruction_amd import DepthOdometry
    key = tuple(sorted(params.items()))
    if key not in _cache:
        _cache[key] = DepthOdometry(COLS, ROWS, cam, **params)
    return _cache[key]


def restatement(cam, **params):
    from elasticreconstruction_amd import odometry
    p = odometry.default_params()
    p.update(params)
    return orr.Odometry(COLS, ROWS, cam, tables_=odometry.tables(), **p)


def model_setup():
    """Three frames integrated at their true poses; the model is the volume seen from the pose of frame 1.  -> (volume, its units for the
    restatement, frames, poses, cam4)."""
    if "setup" not in _cache:
        d, W, cam, cam6 = rcc.scene_inputs(3)
        vol = TSDFVolume(COLS, ROWS, cam6, max_units=1024)
        vol.IntegrateFrames(d.reshape(3, -1), W)
        units = rcr.Volume({int(k): vol.read_unit(int(k)) for k in vol.unit_keys()})
        _cache["setup"] = (vol, units, d, W, cam)
    return _cache["setup"]


def test_align_model_walks_the_restatements_steps(gpu):
    vol, units, d, W, cam = model_setup()
    dev, ref = device_odometry(cam), restatement(cam)
    model = vol.raycast(W[1], COLS, ROWS, cam, levels=3, device=True)
    want_model = rcr.raycast_levels(units, COLS, ROWS, cam, W[1], 3)
    for l in range(3):
        assert same_bits(model[l][1].cpu().numpy(), want_model[l][1]) and same_bits(model[l][2].cpu().numpy(), want_model[l][2]), l
    T, status, trace, sums = dev.align_model(model, d, trace=True, sums=True)
    assert T.shape == (3, 4, 4) and trace.shape == (3, 19, 17) and not status.any()
    for i in range(3):
        cur = ref.maps(d[i])
        state = np.eye(4)
        for k, level in enumerate(ref.schedule()):
            s, count = ref.linearize(want_model, cur, level, state)
            assert count == int(trace[i, k, 16]) and count > 0, (i, k, count, trace[i, k, 16])
            step, lost = ref.step(s, count, state)
            assert not lost and np.abs(step - trace[i, k, :16].reshape(4, 4)).max() <= 1e-6, (i, k)
            state = trace[i, k, :16].reshape(4, 4)
        assert np.array_equal(T[i], state)
        s, count, sabs = ref.linearize(want_model, cur, 0, trace[i, -2, :16].reshape(4, 4), with_abs=True)
        assert np.all(np.abs(sums[i] - s) <= count * 2.0 ** -53 * sabs), i
        G = np.linalg.inv(W[1]) @ W[i]
        print("frame %d against the model at frame 1: %.3g deg, %.3g mm from the truth" % ((i,) + tuple(np.array(orr.pose_error(T[i], G)) * (1, 1e3))))
    # the restatement route end to end, and maps handed over in host memory
    rT, rlost, _ = rcr.align_model(ref, units, W[1], d[2])
    G = np.linalg.inv(W[1]) @ W[2]
    assert not rlost and orr.pose_error(T[2], rT)[0] < orr.pose_error(rT, G)[0] and orr.pose_error(T[2], rT)[1] < orr.pose_error(rT, G)[1], \
        "the device stays closer to the restatement than the restatement is to the truth"
    host_model = vol.raycast(W[1], COLS, ROWS, cam, levels=3)
    T2, S2 = dev.align_model(host_model, d)
    assert np.array_equal(T2.view(np.uint64), T.view(np.uint64)) and np.array_equal(S2, status)


def test_a_frames_result_is_the_same_alone_in_a_list_and_for_any_window(gpu):
    vol, units, d, W, cam = model_setup()
    dev = device_odometry(cam)
    model = vol.raycast(W[1], COLS, ROWS, cam, levels=3, device=True)
    guess = np.stack([np.linalg.inv(W[1]) @ W[i] for i in range(3)])
    T, S, Tr, Su = dev.align_model(model, d, guess=guess, trace=True, sums=True)
    for i in range(3):
        t, s, tr, su = dev.align_model(model, d[i], guess=guess[i:i + 1], trace=True, sums=True)
        assert s[0] == S[i] and np.array_equal(t[0].view(np.uint64), T[i].view(np.uint64))
        assert np.array_equal(tr[0].view(np.uint64), Tr[i].view(np.uint64)) and np.array_equal(su[0].view(np.uint64), Su[i].view(np.uint64))
    for window in (2, 3, 4):                       # window 2: one frame per run, the model's slot stays resident from run to run
        t, s = dev.align_model(model, d, guess=guess, window=window)
        assert np.array_equal(t.view(np.uint64), T.view(np.uint64)) and np.array_equal(s, S), window
    back = dev.align_model(model, d[::-1].copy(), guess=guess[::-1].copy())[0]
    assert np.array_equal(back[::-1].view(np.uint64), T.view(np.uint64))


def test_one_level_and_refusals(gpu):
    vol, units, d, W, cam = model_setup()
    dev1, ref1 = device_odometry(cam, levels=1), restatement(cam, levels=1)
    model = vol.raycast(W[1], COLS, ROWS, cam, levels=1, device=True)
    T, S, Tr = dev1.align_model(model, d[2], trace=True)
    assert not S.any() and Tr.shape == (1, 10, 17)
    rT, rlost, rtrace = rcr.align_model(ref1, units, W[1], d[2])
    G = np.linalg.inv(W[1]) @ W[2]
    assert not rlost and int(Tr[0, 0, 16]) == rtrace[0][1]
    assert orr.pose_error(T[0], rT)[0] < orr.pose_error(rT, G)[0] and orr.pose_error(T[0], rT)[1] < orr.pose_error(rT, G)[1]
    dev3 = device_odometry(cam)
    with pytest.raises(ValueError):
        dev3.align_model(model, d[2])                                   # one level for an odometry of three
    m3 = vol.raycast(W[1], COLS, ROWS, cam, levels=3, device=True)
    L = _ffi.lib()
    frames = np.ascontiguousarray(d[2].reshape(1, -1))
    out, st = np.zeros((1, 16)), np.zeros(1, np.int32)
    recs = (C.c_void_p * 3)(m3[0][1].data_ptr(), None, m3[2][1].data_ptr())
    assert L.er_frame_to_model_align(dev3._h, recs, 1, _ffi.ptr(frames), 0, None, _ffi.ptr(out), _ffi.ptr(st), None, None, 0) != 0
    assert b"level 1" in L.er_last_error()
    assert L.er_frame_to_model_align(dev3._h, None, 1, _ffi.ptr(frames), 0, None, _ffi.ptr(out), _ffi.ptr(st), None, None, 0) != 0
    recs = (C.c_void_p * 3)(*[m[1].data_ptr() for m in m3])
    assert L.er_frame_to_model_align(dev3._h, recs, 1, _ffi.ptr(frames), 0, None, _ffi.ptr(out), None, None, None, 0) != 0
    assert L.er_frame_to_model_align(dev3._h, recs, 1, _ffi.ptr(frames), 0, None, _ffi.ptr(out), _ffi.ptr(st), None, None, 1) != 0
    assert L.er_frame_to_model_align(dev3._h, recs, 0, _ffi.ptr(frames), 0, None, _ffi.ptr(out), _ffi.ptr(st), None, None, 0) != 0
    assert not out.any()


def test_track_model_is_the_chain_of_public_calls_and_stays_near_the_truth(gpu):
    # 320 x 240: at 160 x 120 a pixel at the walls' distance is three voxels wide, and a volume that holds ONE frame is then a staircase of
    # facets that all face the camera of that frame -- the model's normals say nothing about the walls (measured on the restatements: frame 1
    # against the one-frame model ends 1.55 degrees and 10.7 mm off at 160 x 120, 0.03 degrees and 0.10 mm at 320 x 240).
    from elasticreconstruction_amd import DepthOdometry
    import odometry_cases as oc
    n, cols, rows = 6, 320, 240
    d, W, cam = oc.scene(cols, rows, n)
    W = np.asarray(W, np.float64).copy()
    W[:, :3, 3] += rcc.SCENE_SHIFT
    cam6 = np.array(list(cam) + [2.5, 4.0], np.float32)
    dev = DepthOdometry(cols, rows, cam)
    vol = TSDFVolume(cols, rows, cam6, max_units=1024)
    P, S = dev.track_model(vol, d, T0=W[0])
    assert P.shape == (n, 4, 4) and not S.any(), "no frame is lost"
    # the same chain written out by hand
    hand = TSDFVolume(cols, rows, cam6, max_units=1024)
    Q = [np.asarray(W[0], np.float64)]
    hand.Integrate(d[0], Q[0])
    for i in range(1, n):
        model = hand.raycast(Q[-1], cols, rows, cam, levels=3, device=True)
        T, st = dev.align_model(model, d[i])
        assert st[0] == 0
        Q.append(mat4_mul(Q[-1], T[0]))
        hand.Integrate(d[i], Q[-1])
    assert np.array_equal(np.stack(Q).view(np.uint64), P.view(np.uint64))
    assert np.array_equal(hand.unit_keys(), vol.unit_keys())
    vol.close()
    hand.close()
    # beside frame-to-frame tracking, against the ground truth
    from elasticreconstruction_amd import accumulate
    A = accumulate(dev.track(d)[0], W[0])
    half_voxel = 0.5 * rcc.UL
    half_voxel_deg = math.degrees(math.atan(half_voxel / 1.0))
    worst = 0.0
    for i in range(1, n):
        mr, mt = orr.pose_error(P[i], W[i])
        fr, ft = orr.pose_error(A[i], W[i])
        print("frame %d: track_model %.4f deg %.3f mm; track %.4f deg %.3f mm" % (i, mr, mt * 1e3, fr, ft * 1e3))
        worst = max(worst, mt / (2 * ft + half_voxel), mr / (2 * fr + half_voxel_deg))
        assert mt <= 2 * ft + half_voxel and mr <= 2 * fr + half_voxel_deg, i
    print("worst error / bar: %.3f" % worst)
