"""The timeline hook of the batch pipeline (er_tsdf_set_timeline / er_tsdf_get_timeline, er_tsdf.hip: run_batch).

Eight calls of 1, 3, 7, 1, 3, 7, 1, 3 frames are eight batches: the three pipeline slots wrap twice and both pre-pass streams are used four
times; the calls alternate between warp and rigid.  Images are 64 x 48 (the room through a camera scaled down by 10), so every kernel is one
or two workgroups wide and the file runs in a few seconds.  What is asserted about the times is what the events of run_batch guarantee --
order within a stream and across the two event waits -- never an overlap or a rate: at these shapes launch latency decides both.

The oracle and the empty 3-pixel border are those of tests/test_tsdf_pipeline_order_gpu.py (its docstring says why), at this file's image size."""
import functools

import numpy as np
import pytest

import helpers
from elasticreconstruction_amd import synth
from elasticreconstruction_amd.tsdf import TSDFVolume, mat4_mul
from oracle.pyoracle import OracleVolume
from test_tsdf_pipeline_order_gpu import Snapshot, _feed, _slice_warp

pytestmark = pytest.mark.gpu

COLS, ROWS, PX = 64, 48, 64 * 48
CAM = np.array([52.5, 52.5, 31.5, 23.5, 2.5, 2.5], np.float32)
UNITS = 512
CALLS = [1, 3, 7, 1, 3, 7, 1, 3]
WARP_ON = lambda c: c % 2 == 0
X_COLS = ("x_wait", "x_consts", "x_fix", "x_prepare", "x_plan")


@functools.lru_cache(maxsize=None)
def _scene():
    """26 frames in 13 fragments, and the oracle's volume with the warp on the frames of every other call."""
    n, interval = sum(CALLS), 2
    w = synth.circle_trajectory(3000)[::110][:n]
    d = synth.to_numpy_u16(synth.render_depth(w, cols=COLS, rows=ROWS, cam=tuple(float(c) for c in CAM[:4]))).copy().reshape(-1, ROWS, COLS)
    d[:, :3, :] = d[:, -3:, :] = 0
    d[:, :, :3] = d[:, :, -3:] = 0
    pose, seg = synth.split_trajectory(w, interval)
    sc = dict(depth=np.ascontiguousarray(d.reshape(-1, PX)), traj=np.stack([mat4_mul(pose[f // interval], seg[f]) for f in range(n)]), pose=pose,
              seg=seg, grids=synth.control_grids(pose, 8, 3.0, 0.005), interval=interval, resolution=8, length=3.0, n=n)
    sc["warp"] = wa = synth.warp_arrays(sc)
    big, ora = OracleVolume(640, 480, CAM), OracleVolume(COLS, ROWS, CAM)
    f = 0
    for c, k in enumerate(CALLS):
        for _ in range(k):
            frame = sc["depth"][f]
            if WARP_ON(c):
                e = np.zeros((480, 640), np.uint16)
                e[:ROWS, :COLS] = frame.reshape(ROWS, COLS)
                o = big.Reproject(e, sc["grids"][wa["grid_index"][f]], 8, 3.0, wa["seg"][f], wa["madj"][f]).reshape(480, 640)
                assert not o[ROWS:].any() and not o[:, COLS:].any(), "test input: a warped point leaves the %d x %d image" % (COLS, ROWS)
                frame = np.ascontiguousarray(o[:ROWS, :COLS]).reshape(-1)
            ora.Integrate(frame, sc["traj"][f])
            f += 1
    ref = Snapshot(ora)
    ora.close()
    big.close()
    return sc, ref


def _volume():
    return TSDFVolume(COLS, ROWS, CAM, max_units=UNITS)


def test_hook_off_records_nothing(gpu):
    sc, ref = _scene()
    vol = _volume()
    _feed(vol, sc, CALLS, WARP_ON)
    assert vol.get_timeline() == []
    assert helpers.assert_volumes_identical(vol, ref, "hook off:") >= 2
    vol.close()


def test_one_row_per_batch_in_pipeline_order(gpu):
    sc, ref = _scene()
    off, vol = _volume(), _volume()
    _feed(off, sc, CALLS, WARP_ON)
    vol.set_timeline(True)
    _feed(vol, sc, CALLS, WARP_ON)
    rows = vol.get_timeline()
    assert vol.get_timeline() == [], "reading clears the record"
    assert [r["batch"] for r in rows] == list(range(len(CALLS))) and [r["frames"] for r in rows] == CALLS, rows
    for b, r in enumerate(rows):
        assert r["slot"] == b % 3 and r["stream"] == b % 2, r
        assert 0.0 <= r["host_in"] <= r["host_consts"] <= r["host_out"], r
        x = [r[c] for c in X_COLS]
        assert 0.0 <= x[0] and x == sorted(x), "batch %d is not monotone on its pre-pass stream: %r" % (b, r)
        assert r["x_plan"] <= r["v_begin"] <= r["v_end"], "batch %d: k_integrate against its own pre-pass: %r" % (b, r)
    for b in range(len(rows) - 1):
        assert rows[b]["host_out"] <= rows[b + 1]["host_in"]
        assert rows[b]["v_end"] <= rows[b + 1]["v_begin"], "k_integrate of batch %d begins before that of batch %d ends" % (b + 1, b)
    for b in range(len(rows) - 2):
        assert rows[b]["x_plan"] <= rows[b + 2]["x_wait"], "batches %d and %d share a pre-pass stream" % (b, b + 2)
    for b in range(len(rows) - 3):
        assert rows[b]["v_end"] <= rows[b + 3]["x_wait"], "the pre-pass of batch %d begins before k_integrate of batch %d ends (int_done)" % (b + 3, b)
    assert helpers.assert_volumes_identical(vol, off, "hook on against hook off:") >= 2
    helpers.assert_volumes_identical(vol, ref, "hook on:")
    vol.set_timeline(False)
    off.close()
    vol.close()


def test_switching_off_with_batches_in_flight(gpu):
    """The rows recorded until then stay readable, later batches record nothing, and the volume is the oracle's."""
    sc, ref = _scene()
    lo = sum(CALLS[:5])
    first = dict(sc, depth=sc["depth"][:lo], traj=sc["traj"][:lo], warp=_slice_warp(sc["warp"], 0, lo), n=lo)
    rest = dict(sc, depth=sc["depth"][lo:], traj=sc["traj"][lo:], warp=_slice_warp(sc["warp"], lo, sc["n"]), n=sc["n"] - lo)
    vol = _volume()
    vol.set_timeline(True)
    _feed(vol, first, CALLS[:5], WARP_ON)
    vol.set_timeline(False)
    _feed(vol, rest, CALLS[5:], lambda c: WARP_ON(c + 5))
    rows = vol.get_timeline()
    assert [r["batch"] for r in rows] == list(range(5)) and all(r["v_begin"] <= r["v_end"] for r in rows), rows
    assert vol.get_timeline() == []
    vol.set_timeline(True)                                        # a new recording starts from nothing, against a new base
    assert vol.get_timeline() == []
    helpers.assert_volumes_identical(vol, ref, "hook switched off in mid-flight:")
    vol.close()
