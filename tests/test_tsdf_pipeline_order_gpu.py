"""The order of the batch pipeline (er_tsdf.hip: run_batch) under many small batches: the pipeline slots (three), the pre-pass streams
(two) and the ring of per-batch constants (six entries) wrap several times, the warp's scatter of a batch runs before the batch's slot
is free, warp and rigid calls alternate, a zero-write replay sits between ordinary batches, reset / wait_event / synchronize cut in
with batches in flight.  Every volume is compared bit for bit -- unit set and every voxel -- with the CPU oracle fed frame by frame.

Images are 80 x 60 (the room seen through a camera scaled down by 8: a frame still touches 8 and more units), so a case runs in a second
or two.  The oracle's Reproject keeps the reference's literal 640 x 480 bounds (oracle/tsdf_oracle.c: xyz2uvd) while the library clips
to the image, so a warped point that left an 80 x 60 image to the right or below would be undefined on the oracle's side.  The frames
therefore carry an empty 3-pixel border (the grids move a point by less than a pixel), and the oracle re-projects every frame embedded
in the corner of a 640 x 480 image, where such a point would land in plain sight: _reproject asserts that there is none."""
import functools

import numpy as np
import pytest

import helpers
from elasticreconstruction_amd import synth
from elasticreconstruction_amd.tsdf import TSDFVolume, mat4_mul
from oracle.pyoracle import OracleVolume

pytestmark = pytest.mark.gpu

COLS, ROWS, PX = 80, 60, 80 * 60
CAM = np.array([525.0 / 8, 525.0 / 8, 39.5, 29.5, 2.5, 2.5], np.float32)
UNITS = 512


class Snapshot:
    """The units of a volume at one moment (what helpers.assert_volumes_identical reads); never changed afterwards."""

    def __init__(self, vol):
        self.keys = vol.unit_keys().copy()
        self.units = {int(k): vol.read_unit(k) for k in self.keys}

    def unit_keys(self):
        return self.keys

    def read_unit(self, key):
        return self.units[int(key)]


def _render(poses):
    d = synth.to_numpy_u16(synth.render_depth(poses, cols=COLS, rows=ROWS, cam=tuple(float(c) for c in CAM[:4]))).copy().reshape(-1, ROWS, COLS)
    d[:, :3, :] = d[:, -3:, :] = 0
    d[:, :, :3] = d[:, :, -3:] = 0
    return np.ascontiguousarray(d.reshape(-1, PX))


@functools.lru_cache(maxsize=None)
def _big_oracle():
    return OracleVolume(640, 480, CAM)


def _reproject(depth, ctr, resolution, length, seg, madj):
    """The oracle's Reproject of one 80 x 60 frame (module docstring)."""
    e = np.zeros((480, 640), np.uint16)
    e[:ROWS, :COLS] = depth.reshape(ROWS, COLS)
    o = _big_oracle().Reproject(e, ctr, resolution, length, seg, madj).reshape(480, 640)
    assert not o[ROWS:].any() and not o[:, COLS:].any(), "test input: a warped point leaves the %d x %d image" % (COLS, ROWS)
    return np.ascontiguousarray(o[:ROWS, :COLS]).reshape(-1)


def _scenario(n, interval, stride):
    """synth.make_scenario at 80 x 60: n frames of the circle through the room, `interval` frames per fragment / control grid."""
    w = synth.circle_trajectory(3000)[::stride][:n]
    pose, seg = synth.split_trajectory(w, interval)
    traj = np.stack([mat4_mul(pose[f // interval], seg[f]) for f in range(n)])
    sc = dict(depth=_render(w), traj=traj, pose=pose, seg=seg, grids=synth.control_grids(pose, 8, 3.0, 0.005), interval=interval,
              resolution=8, length=3.0, n=n)
    sc["warp"] = synth.warp_arrays(sc)
    w_ = sc["warp"]
    sc["warped"] = np.stack([_reproject(sc["depth"][f], sc["grids"][w_["grid_index"][f]], 8, 3.0, w_["seg"][f], w_["madj"][f]) for f in range(n)])
    return sc


def _oracle(sc, use_warp):
    """Snapshot of the oracle's volume after the frames of sc, frame by frame; use_warp: bool, or one bool per frame."""
    ora = OracleVolume(COLS, ROWS, CAM)
    flags = [use_warp] * sc["n"] if isinstance(use_warp, bool) else use_warp
    for f in range(sc["n"]):
        ora.Integrate(sc["warped"][f] if flags[f] else sc["depth"][f], sc["traj"][f])
    snap = Snapshot(ora)
    ora.close()
    return snap


CALLS = [1, 2, 3] * 5                      # 15 batches as 15 calls: the slots wrap five times, the constants ring two and a half times


@functools.lru_cache(maxsize=None)
def _small():
    """30 frames, 6 fragments; the oracle with the warp on every frame, on none, and on the frames of every other call."""
    sc = _scenario(sum(CALLS), 5, 100)
    alt = []
    for c, k in enumerate(CALLS):
        alt += [c % 2 == 0] * k
    return sc, _oracle(sc, True), _oracle(sc, False), alt, _oracle(sc, alt)


@functools.lru_cache(maxsize=None)
def _long():
    sc = _scenario(130, 10, 23)
    return sc, _oracle(sc, True)


def _slice_warp(w, lo, hi):
    return dict(ctr=w["ctr"], resolution=w["resolution"], length=w["length"], grid_index=w["grid_index"][lo:hi], seg=w["seg"][lo:hi], madj=w["madj"][lo:hi])


def _feed(vol, sc, calls, warp_on, device_depth=None, sync=False):
    """The frames of sc as len(calls) IntegrateFrames calls; warp_on: bool, or a function of the call's index."""
    lo = 0
    for c, k in enumerate(calls):
        on = warp_on if isinstance(warp_on, bool) else warp_on(c)
        w = _slice_warp(sc["warp"], lo, lo + k) if on else None
        if device_depth is not None:
            vol.IntegrateFrames(None, sc["traj"][lo:lo + k], w, device_ptr=device_depth.data_ptr() + lo * PX * 2)
        else:
            vol.IntegrateFrames(sc["depth"][lo:lo + k], sc["traj"][lo:lo + k], w)
        if sync:
            vol.synchronize()
        lo += k
    assert lo == sc["n"]


def _to_device(depth):
    import torch
    t = torch.from_numpy(depth.view(np.int16)).to("cuda:0")
    torch.cuda.synchronize()                # the pre-pass streams do not wait for torch's
    return t


def _three_ways(sc, ref, warp_on, what):
    dev = _to_device(sc["depth"])
    vols = [TSDFVolume(COLS, ROWS, CAM, max_units=UNITS) for _ in range(3)]
    _feed(vols[0], sc, CALLS, warp_on, device_depth=dev)
    _feed(vols[1], sc, CALLS, warp_on)
    _feed(vols[2], sc, CALLS, warp_on, sync=True)
    for v, how in zip(vols, ("device frames", "host frames", "host frames, synchronize() after every call")):
        assert helpers.assert_volumes_identical(v, ref, "%s, %s:" % (what, how)) >= 2
        v.close()
    del dev


def test_many_small_batches_with_warp(gpu):
    sc, ref_warp, _, _, _ = _small()
    _three_ways(sc, ref_warp, True, "15 warp calls of 1, 2, 3 frames")


def test_many_small_batches_without_warp(gpu):
    sc, _, ref_rigid, _, _ = _small()
    _three_ways(sc, ref_rigid, False, "15 rigid calls of 1, 2, 3 frames")


def test_warp_and_rigid_calls_alternate(gpu):
    """Only a warp batch has the part of the chain that runs before its slot is free; its neighbours on both pre-pass streams are rigid."""
    sc, _, _, _, ref_alt = _small()
    _three_ways(sc, ref_alt, lambda c: c % 2 == 0, "warp and rigid calls alternating")


def test_zero_write_replay_between_ordinary_batches(gpu):
    """The construction of test_tsdf_gpu.py::test_reproject_zero_depth_reset_inside_a_batch (a grid that collapses the points onto the
    camera: writes of depth 0, flagged and replayed by k_reproject_fix) in calls 3 and 4 of seven 3-frame calls, one on each pre-pass
    stream, with ordinary warp batches in front of and behind them on the same stream: the scatter that follows a replay batch must meet
    cleared flag words and re-armed replay buffers, although it no longer waits for its slot."""
    res, length = 2, 3.0
    n1 = res + 1
    k, j, i = np.meshgrid(np.arange(n1), np.arange(n1), np.arange(n1), indexing="ij")
    verts = np.stack([i.ravel(), j.ravel(), k.ravel()], 1).astype(np.float64) * (length / res)
    squash = verts.copy()
    squash[:, 2] = -0.3 + 0.0001 + (verts[:, 2] / length) * 0.0013
    squash[:, 0] = 1.5 + (verts[:, 0] - 1.5) * 0.0002               # (a narrower cone than at 640 x 480: the points stay inside 80 x 60)
    squash[:, 1] = 1.5 + (verts[:, 1] - 1.5) * 0.0002
    mild = verts + np.random.RandomState(3).normal(0, 0.004, verts.shape)
    grids = np.stack([mild, squash]).astype(np.float32)
    n, special = 21, (9, 11, 13)
    traj = synth.circle_trajectory(3000)[::140][:n]
    depth = _render(traj)
    depth[np.random.RandomState(6).rand(n, PX) < 0.05] = 0
    seg = np.stack([synth.basepose(length)] * n)
    madj = np.stack([np.linalg.inv(seg[0])] * n)
    warp = dict(ctr=grids, resolution=res, length=np.float32(length), grid_index=np.array([1 if f in special else 0 for f in range(n)], np.int32),
                seg=seg, madj=madj)
    sc = dict(depth=depth, traj=traj, warp=warp, n=n)
    ora = OracleVolume(COLS, ROWS, CAM)
    zero_cells = 0
    for f in range(n):
        d = _reproject(depth[f], grids[warp["grid_index"][f]], res, length, seg[f], madj[f])
        if f in special:
            zero_cells += int((d == 1).sum())
        ora.Integrate(d, traj[f])
    assert zero_cells > 0, "test input does not exercise the 0/1 mm boundary"
    dev = _to_device(depth)
    for how, kw in (("device frames", dict(device_depth=dev)), ("host frames", {})):
        vol = TSDFVolume(COLS, ROWS, CAM, max_units=UNITS)
        _feed(vol, sc, [3] * 7, True, **kw)
        assert helpers.assert_volumes_identical(vol, ora, "zero-write replay between ordinary batches, %s:" % how) >= 2
        vol.close()
    ora.close()


def test_reset_and_wait_event_with_batches_in_flight(gpu):
    """reset() while batches are in flight, then every call's frames arrive in HBM by an asynchronous copy on a stream of the caller's,
    announced with wait_event(): the pre-pass -- its hoisted scatter too -- must wait for the event.  The volume must equal a fresh
    handle's and the oracle's."""
    import torch
    sc, ref_warp, _, _, _ = _small()
    vol = TSDFVolume(COLS, ROWS, CAM, max_units=UNITS)
    _feed(vol, sc, CALLS, lambda c: c % 2 == 1)               # something else first, left in flight
    vol.reset()
    assert vol.unit_count() == 0
    pinned = torch.from_numpy(sc["depth"].view(np.int16)).pin_memory()
    dev = torch.zeros_like(pinned, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    events, lo = [], 0
    for k in CALLS:
        with torch.cuda.stream(side):
            dev[lo:lo + k].copy_(pinned[lo:lo + k], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
        events.append(ev)
        vol.wait_event(ev.cuda_event)
        vol.IntegrateFrames(None, sc["traj"][lo:lo + k], _slice_warp(sc["warp"], lo, lo + k), device_ptr=dev.data_ptr() + lo * PX * 2)
        lo += k
    fresh = TSDFVolume(COLS, ROWS, CAM, max_units=UNITS)
    _feed(fresh, sc, CALLS, True)
    assert helpers.assert_volumes_identical(vol, fresh, "after reset() and wait_event(), against a fresh handle:") >= 2
    helpers.assert_volumes_identical(vol, ref_warp, "after reset() and wait_event():")
    vol.close()
    fresh.close()


def test_callers_stream_is_joined_to_the_voxel_stream(gpu):
    """With a stream of the caller's (set_stream) the voxel passes still run on the handle's own stream.  Nothing may read the volume
    on the caller's stream before the last voxel pass is done: read-outs straight after the calls, without synchronize(), see every
    frame; reset() on the caller's stream stands in front of the next call's voxel passes; profiling counts as before; and a handle
    that goes back to its own stream carries on."""
    import torch
    sc, ref_warp, _, _, _ = _small()
    dev = _to_device(sc["depth"])
    stream = torch.cuda.Stream()
    vol = TSDFVolume(COLS, ROWS, CAM, max_units=UNITS)
    vol.set_stream(stream.cuda_stream)
    _feed(vol, sc, CALLS, lambda c: c % 2 == 1, device_depth=dev)          # something else first
    vol.reset()                                                             # memsets on the caller's stream
    vol.set_profiling(True)
    _feed(vol, sc, CALLS, True, device_depth=dev)
    assert helpers.assert_volumes_identical(vol, ref_warp, "on a caller's stream, read straight after the calls:") >= 2
    prof = vol.get_profile()
    assert prof["launches"] == len(CALLS) and prof["frames"] == sc["n"], prof
    vol.set_profiling(False)
    vol.reset()
    half = len(CALLS) // 2
    lo = sum(CALLS[:half])
    first = dict(sc, depth=sc["depth"][:lo], traj=sc["traj"][:lo], warp=_slice_warp(sc["warp"], 0, lo), n=lo)
    rest = dict(sc, depth=sc["depth"][lo:], traj=sc["traj"][lo:], warp=_slice_warp(sc["warp"], lo, sc["n"]), n=sc["n"] - lo)
    _feed(vol, first, CALLS[:half], True)
    vol.set_stream(None)                                                    # back to the handle's own stream, batches in flight
    _feed(vol, rest, CALLS[half:], True)
    helpers.assert_volumes_identical(vol, ref_warp, "half on a caller's stream, half on the handle's own:")
    vol.close()
    del dev


def test_one_call_of_130_frames_equals_one_frame_per_call(gpu):
    """130 frames in one call are three batches of 44, 44 and 42 frames; one frame per call is 130 batches."""
    sc, ref = _long()
    one, each = TSDFVolume(COLS, ROWS, CAM, max_units=UNITS), TSDFVolume(COLS, ROWS, CAM, max_units=UNITS)
    one.IntegrateFrames(sc["depth"], sc["traj"], sc["warp"])
    _feed(each, sc, [1] * sc["n"], True, device_depth=_to_device(sc["depth"]))
    assert helpers.assert_volumes_identical(one, ref, "130 frames in one call:") >= 2
    helpers.assert_volumes_identical(each, ref, "130 frames, one per call:")
    one.close()
    each.close()


def test_profile_counts_one_launch_per_batch(gpu):
    """With profiling on, k_integrate is still launched once per batch -- 15 small calls and one of 130 frames in three batches -- and
    the frames are all accounted for; the timed pipeline gives the same volume."""
    sc, ref_warp, _, _, _ = _small()
    lg, _ = _long()
    vol = TSDFVolume(COLS, ROWS, CAM, max_units=UNITS)
    vol.set_profiling(True)
    _feed(vol, sc, CALLS, True)
    prof = vol.get_profile()
    assert prof["launches"] == len(CALLS) and prof["frames"] == sc["n"], prof
    helpers.assert_volumes_identical(vol, ref_warp, "with profiling on:")
    vol.IntegrateFrames(lg["depth"], lg["traj"], lg["warp"])
    prof = vol.get_profile()
    assert prof["launches"] == len(CALLS) + 3 and prof["frames"] == sc["n"] + 130, prof
    assert prof["integrate_ms"] > 0.0 and prof["unit_visits"] > 0
    vol.close()
