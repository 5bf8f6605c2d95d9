"""Holds tests/prepass_restatement.py to the CPU oracle: the scaled depth of a frame bit for bit, and the set of units a frame touches (a
fresh OracleVolume holds exactly the units its one frame touched).  tests/test_prepass_gpu.py then holds k_prepare to the restatement."""
import numpy as np
import pytest

import prepass_restatement as R
from oracle.pyoracle import OracleVolume


def small_cam(cols, rows):
    return np.array([525.0, 525.0, (cols - 1) / 2.0, (rows - 1) / 2.0, 2.5, 2.5], np.float32)


def pose(tx, ty, tz, yaw=0.0):
    T = np.eye(4)
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(yaw), np.sin(yaw), -np.sin(yaw), np.cos(yaw)
    T[:3, 3] = tx, ty, tz
    return T


def frames(cols, rows, n, seed):
    """Depth with holes, steps across unit boundaries (a unit is 0.375 m), values beyond integration_trunc and the largest value."""
    rng = np.random.RandomState(seed)
    d = rng.choice(np.array([0, 1, 400, 1000, 1150, 1200, 2400, 2600, 3000], np.uint16), size=(n, rows * cols))
    d[:, ::7] = rng.randint(300, 2600, d[:, ::7].shape).astype(np.uint16)
    d[:, 5:7] = 65535                                      # (two pixels only: the oracle integrates every unit a frame touches, 64^3 voxels each)
    return d.astype(np.uint16)


@pytest.mark.parametrize("cols,rows", [(36, 33), (30, 21), (64, 32)])
def test_restatement_equals_oracle(cols, rows):
    cam = small_cam(cols, rows)
    d = frames(cols, rows, 3, 11 + cols)
    Ts = [pose(1.5, 1.5, 0.2), pose(1.31, 1.62, 0.05, 0.3), pose(0.9, 2.0, 1.0, -1.1)]
    got = R.products(d, Ts, cam, cols, rows)
    assert got["out_of_range"] == 0
    union = {}
    for f in range(3):
        ora = OracleVolume(cols, rows, cam)
        assert np.array_equal(ora.ScaleDepth(d[f]).view(np.uint32), got["scaled"][f, :cols * rows].view(np.uint32))
        ora.Integrate(d[f], Ts[f])
        keys = np.sort(ora.unit_keys())
        mine = np.unique(R.unit_keys(d[f], Ts[f], cam, cols, rows))
        assert np.array_equal(keys, mine[mine >= 0]), "frame %d" % f
        for k in keys:
            union[int(k)] = union.get(int(k), 0) | (1 << f)
        ora.close()
    assert len(union) > 3
    assert np.array_equal(got["keys"], np.array(sorted(union), np.int32))
    assert np.array_equal(got["masks"], np.array([union[k] for k in sorted(union)], np.uint64))
    assert not got["scaled"][:, cols * rows:].any()


def test_default_camera_full_size_scale_depth():
    d = frames(640, 480, 1, 5)
    ora = OracleVolume()
    assert np.array_equal(ora.ScaleDepth(d[0]).view(np.uint32), R.scale_depth(d, R.DEFAULT_CAM, 640, 480)[0].view(np.uint32))
    ora.close()


def test_extrema_by_hand():
    """The minima count a pixel without usable depth as 0, in its own 16-pixel tile and in its 32-pixel tile only."""
    cols, rows = 64, 32
    cam = small_cam(cols, rows)
    d = np.full((1, rows, cols), 1000, np.uint16)
    d[0, 20, 37] = 0                                       # tile 1; fine tile (1, 2)
    d[0, 3, 3] = 3000                                      # beyond integration_trunc: scaled 0 -> the minimum of tile 0 / fine tile (0, 0) is 0
    got = R.products(d.reshape(1, -1), [pose(1.5, 1.5, 0.2)], cam, cols, rows)
    sc = got["scaled"][0, :cols * rows].reshape(rows, cols)
    assert sc[3, 3] == 0 and sc[20, 37] == 0 and sc[0, 0] > 1.0
    assert got["tile_lo"].shape == (1, 2, 1) and got["tile_lo_fine"].shape == (2, 4, 1) and got["tile_max"].shape == (1, 2, 1)
    assert list(got["tile_lo"][0, :, 0]) == [0.0, 0.0]
    fine = got["tile_lo_fine"][:, :, 0]
    assert fine[0, 0] == 0 and fine[1, 2] == 0
    assert (np.delete(fine.reshape(-1), [0, 6]) >= 1.0).all()
    assert got["tile_max"][0, 0, 0] == sc[:, :32].max() and got["tile_max"][0, 1, 0] == sc[:, 32:].max()
    assert (R.unit_keys(d[0], pose(1.5, 1.5, 0.2), cam, cols, rows).reshape(rows, cols)[3, 3]) >= 0     # ... and its key is still touched
