"""The fragment builder on the GPU (er_frag_*, er_frames_to_models_align; csrc/er_fragments.hip) against the route it replaces:
per fragment DepthOdometry.track_model on a fresh TSDFVolume, then extract_oriented and SaveFragment's cube filter.  Everything is compared
bit for bit -- poses as uint64, statuses, points and normals -- for several lane counts, host and device depth, and a second run.

The scene: 14 frames of odometry_cases.scene(320, 240) moved off the unit lattice by raycast_cases.SCENE_SHIFT, interval 4 (fragments of 4, 4,
4 and 2 frames), every fragment started at the shifted truth pose of its first frame."""
import numpy as np
import pytest

import odometry_cases as oc
import raycast_cases as rcc
from odometry_cases import same_bits
from elasticreconstruction_amd import _ffi
from elasticreconstruction_amd.tsdf import TSDFVolume

pytestmark = pytest.mark.gpu
COLS, ROWS, N, INTERVAL, UNITS = 320, 240, 14, 4, 256
_cache = {}


def scene():
    """(depth uint16 [N, ROWS * COLS], shifted truth poses, cam4, cam6)."""
    if "scene" not in _cache:
        d, W, cam = oc.scene(COLS, ROWS, N)
        W = np.asarray(W, np.float64).copy()
        W[:, :3, 3] += rcc.SCENE_SHIFT
        cam6 = np.array(list(cam) + [2.5, 4.0], np.float32)
        _cache["scene"] = (d.reshape(N, -1).copy(), W, cam, cam6)
    return _cache["scene"]


def reference(depth, T0s, cols=COLS, rows=ROWS, cam=None, cam6=None, interval=INTERVAL, max_units=UNITS, length=3.0):
    """The loop the builder replaces: per fragment track_model on a fresh volume, extract_oriented, the cube filter."""
    from elasticreconstruction_amd import DepthOdometry
    if cam is None:
        _, _, cam, cam6 = scene()
    od = DepthOdometry(cols, rows, cam)
    Ws, Ss, frags = [], [], []
    for k, lo in enumerate(range(0, len(depth), interval)):
        vol = TSDFVolume(cols, rows, cam6, max_units=max_units)
        W, S = od.track_model(vol, depth[lo:lo + interval], T0=T0s[k] if np.ndim(T0s) == 3 else T0s)
        pts, nrm = vol.extract_oriented()
        vol.close()
        x = pts[:, :3]
        inside = ((x >= np.float32(0.0)) & (x < np.float32(length))).all(axis=1)
        Ws.append(W), Ss.append(S), frags.append((np.ascontiguousarray(x[inside]), np.ascontiguousarray(nrm[inside])))
    od.close()
    return np.concatenate(Ws), np.concatenate(Ss), frags


def main_reference():
    if "ref" not in _cache:
        d, W, _, _ = scene()
        _cache["ref"] = reference(d, W[::INTERVAL])
    return _cache["ref"]


def builder(lanes=1, **kw):
    from elasticreconstruction_amd import FragmentBuilder
    _, _, _, cam6 = scene()
    args = dict(interval=INTERVAL, lanes=lanes, max_units=UNITS)
    args.update(kw)
    return FragmentBuilder(COLS, ROWS, cam6, **args)


def same_result(got, want):
    W, S, frags = got
    rW, rS, rfrags = want
    assert W.shape == rW.shape and np.array_equal(W.view(np.uint64), rW.view(np.uint64)), "poses"
    assert np.array_equal(S, rS), "statuses"
    assert len(frags) == len(rfrags)
    for k, ((x, n), (rx, rn)) in enumerate(zip(frags, rfrags)):
        assert x.shape == rx.shape and np.array_equal(x.view(np.uint32), rx.view(np.uint32)), "points of fragment %d" % k
        assert same_bits(n, rn), "normals of fragment %d" % k
    return True


def test_the_reference_meets_the_condition(gpu):
    W, S, frags = main_reference()
    assert W.shape == (N, 4, 4) and not S.any(), "no frame is lost"
    assert [len(x) for x, _ in frags] and min(len(x) for x, _ in frags) >= 1000, [len(x) for x, _ in frags]
    assert len(frags) == 4


@pytest.mark.parametrize("lanes", [1, 2, 3, 5])
def test_every_lane_count_gives_the_reference(gpu, lanes):
    d, W, _, _ = scene()
    b = builder(lanes)
    first = b.build(d, T0=W[::INTERVAL])
    assert same_result(first, main_reference())
    if lanes == 2:
        import torch
        assert same_result(b.build(d, T0=W[::INTERVAL]), first), "the second build on the same handle"
        dev = torch.from_numpy(d.view(np.int16)).to("cuda:0")
        assert same_result(b.build(dev, T0=W[::INTERVAL]), first), "device depth"
        assert b.lane_bytes() > UNITS * (2 << 20)
    b.close()


@pytest.mark.parametrize("lanes", [1, 3])
def test_a_lost_frame_keeps_the_pose_and_nothing_else_changes(gpu, lanes):
    d, W, _, _ = scene()
    d = d.copy()
    d[INTERVAL + 2] = 0                                       # the third frame of fragment 1
    key = "lost"
    if key not in _cache:
        _cache[key] = reference(d, W[::INTERVAL])
    want = _cache[key]
    rW, rS, rfrags = want
    assert rS[INTERVAL + 2] == 1 and rS.sum() == 1 and np.array_equal(rW[INTERVAL + 2], rW[INTERVAL + 1])
    clean = main_reference()
    for k in (0, 2, 3):                                       # the other fragments are the clean run's
        sl = slice(k * INTERVAL, (k + 1) * INTERVAL)
        assert np.array_equal(rW[sl], clean[0][sl]) and np.array_equal(rfrags[k][0], clean[2][k][0])
    b = builder(lanes)
    assert same_result(b.build(d, T0=W[::INTERVAL]), want)
    b.close()


def test_an_all_zero_first_frame_of_a_fragment(gpu):
    d, W, _, _ = scene()
    d = d.copy()
    d[2 * INTERVAL] = 0                                       # fragment 2 starts blind: whatever track_model does is the answer
    want = reference(d, W[::INTERVAL])
    assert want[1][2 * INTERVAL] == 0, "a fragment's first frame is never lost"
    b = builder(3)
    assert same_result(b.build(d, T0=W[::INTERVAL]), want)
    b.close()


def test_one_start_pose_for_all_and_the_base_pose(gpu):
    from elasticreconstruction_amd import synth
    d, W, _, _ = scene()
    d = d[:6]
    b = builder(2)
    one = b.build(d, T0=W[0])
    assert same_result(one, reference(d, W[0]))
    base = b.build(d)
    assert same_result(base, reference(d, synth.basepose(3.0)))
    assert np.array_equal(base[0][0], synth.basepose(3.0)) and np.array_equal(base[0][INTERVAL], synth.basepose(3.0))
    b.close()


def test_full_resolution(gpu):
    from elasticreconstruction_amd import FragmentBuilder
    d, W, cam = oc.scene(640, 480, 6)
    W = np.asarray(W, np.float64).copy()
    W[:, :3, 3] += rcc.SCENE_SHIFT
    d = d.reshape(6, -1).copy()
    cam6 = np.array(list(cam) + [2.5, 4.0], np.float32)
    want = reference(d, W[::3], 640, 480, cam, cam6, interval=3, max_units=256)
    b = FragmentBuilder(640, 480, cam6, interval=3, lanes=2, max_units=256)
    assert same_result(b.build(d, T0=W[::3]), want)
    assert len(want[2]) == 2 and min(len(x) for x, _ in want[2]) > 0
    b.close()


def test_alignment_against_one_model_per_frame(gpu):
    from elasticreconstruction_amd import DepthOdometry
    d, W, cam, cam6 = rcc.scene_inputs(3)
    cols, rows = rcc.SCENE_COLS, rcc.SCENE_ROWS
    vol = TSDFVolume(cols, rows, cam6, max_units=1024)
    vol.IntegrateFrames(d.reshape(3, -1), W)
    od = DepthOdometry(cols, rows, cam)
    models = [vol.raycast(W[k], cols, rows, cam, levels=3, device=True) for k in range(3)]
    # one model: er_frame_to_model_align's bits, trace and sums included
    a = od.align_model(models[1], d, trace=True, sums=True)
    b = od.align_models(models[1:2], d, [0, 0, 0], trace=True, sums=True)
    for x, y in zip(a, b):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    # three models x three frames: every frame's result is the single-model call's
    mof = [0, 1, 2, 1, 2, 0, 2, 0, 1]
    fr = np.stack([d[i // 3] for i in range(9)])
    want_T, want_S = np.zeros((9, 4, 4)), np.zeros(9, np.int32)
    for i in range(9):
        t, s = od.align_model(models[mof[i]], fr[i])
        want_T[i], want_S[i] = t[0], s[0]
    assert not want_S.any() and len({want_T[i].tobytes() for i in range(9)}) == 9
    T, S = od.align_models(models, fr, mof)
    assert np.array_equal(T.view(np.uint64), want_T.view(np.uint64)) and np.array_equal(S, want_S)
    T, S = od.align_models(models, fr[::-1].copy(), mof[::-1])
    assert np.array_equal(T[::-1].view(np.uint64), want_T.view(np.uint64)), "reversed"
    T, S = od.align_models(models, fr, mof, window=2)
    assert np.array_equal(T.view(np.uint64), want_T.view(np.uint64)) and np.array_equal(S, want_S), "window 2: one pair per run"
    with pytest.raises(_ffi.ErError, match="frame 1 names model 3 of 3"):
        od.align_models(models, fr[:2], [0, 3])
    od.close()
    vol.close()


def test_refusals(gpu):
    d, W, _, _ = scene()
    for kw, word in ((dict(interval=0), "interval"), (dict(lanes=0), "lanes"), (dict(lanes=65), "lanes")):
        with pytest.raises(_ffi.ErError, match=word):
            builder(**kw)
    b = builder(1)
    with pytest.raises(_ffi.ErError, match="n_T0 = 2, must be 1 or the fragment count 4"):
        b.build(d, T0=W[:2])
    with pytest.raises(_ffi.ErError, match="n_T0 = 3"):
        b.build(d[:4], T0=W[:3])
    b.close()


def test_edge_counts(gpu):
    d, W, _, _ = scene()
    b = builder(2)
    Wn, S, frags = b.build(d[:0])
    assert Wn.shape == (0, 4, 4) and S.shape == (0,) and frags == []
    got = b.build(d[:1], T0=W[0])
    assert len(got[2]) == 1 and got[0].shape == (1, 4, 4) and np.array_equal(got[0][0], W[0]) and not got[1].any()
    assert same_result(got, reference(d[:1], W[0]))
    b.close()
