"""k_prepare against tests/prepass_restatement.py through er_tsdf_prepass_trace: the scaled depth (pad included) and the three extrema arrays
bit for bit, the (unit key, frame mask) set and the out-of-range count equal.  Shapes are the smallest at which the thread layout can go wrong
(a thread owns four adjacent pixels of a row, a wave 8 rows x 32 columns, a 16-pixel sub-tile is one quad wide and two waves high; the wide
instantiation needs cols % 4 == 0 and an 8-byte aligned depth pointer).  tests/test_prepass_cpu.py holds the restatement to the oracle."""
import numpy as np
import pytest

import prepass_restatement as R
from elasticreconstruction_amd import synth
from elasticreconstruction_amd.tsdf import TSDFVolume
from oracle.pyoracle import OracleVolume

pytestmark = pytest.mark.gpu

UNIT_A, UNIT_B = 1000, 1400                            # depths (mm) on either side of a unit boundary for POSE0: z = 1.2 m and 1.6 m, the boundary at 1.5 m - UL / 2


def small_cam(cols, rows):
    return np.array([525.0, 525.0, (cols - 1) / 2.0, (rows - 1) / 2.0, 2.5, 2.5], np.float32)


def pose(tx, ty, tz, yaw=0.0):
    T = np.eye(4)
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(yaw), np.sin(yaw), -np.sin(yaw), np.cos(yaw)
    T[:3, 3] = tx, ty, tz
    return T


POSE0 = pose(1.7, 1.7, 0.2)                           # x and y stay inside one unit (1.497 .. 1.872 m) over these small images


def poses(n):
    return np.stack([pose(1.5 + 0.004 * f, 1.5 - 0.003 * f, 0.2 + 0.002 * f, 0.01 * f) for f in range(n)])


def random_frames(cols, rows, n, seed):
    rng = np.random.RandomState(seed)
    d = rng.choice(np.array([0, 1, 400, UNIT_A, 1150, UNIT_B, 2400, 2600, 3000], np.uint16), size=(n, rows * cols))
    d[:, ::7] = rng.randint(300, 2600, d[:, ::7].shape).astype(np.uint16)
    d[:, 5:7] = 65535
    return np.ascontiguousarray(d, np.uint16)


def check(vol, depth, Ts, cam, cols, rows, warp=None, seen=None, device_ptr=None):
    """seen: what k_prepare reads on the warped path (the re-projected frames)."""
    before = vol.status()[1]
    tr = vol.prepass_trace(depth, Ts, warp, device_ptr=device_ptr)
    exp = R.products(depth if seen is None else seen, Ts, cam, cols, rows)
    assert tr["pad"] == R.PAD
    for name in ("scaled", "tile_max", "tile_lo", "tile_lo_fine"):
        assert tr[name].shape == exp[name].shape, name
        bad = tr[name].view(np.uint32) != exp[name].view(np.uint32)
        assert not bad.any(), "%s: %d of %d differ, first at %s" % (name, bad.sum(), bad.size, np.argwhere(bad)[0])
    assert np.array_equal(tr["keys"], exp["keys"]), "unit keys"
    assert np.array_equal(tr["masks"], exp["masks"]), "frame masks"
    flags, oor = vol.status()
    assert flags == 0 and oor - before == exp["out_of_range"]
    return exp


# ---- shapes and batch sizes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,rows", [(64, 32), (36, 33), (30, 21)])      # exact tiles / wide, partial tiles, a column group cut by the edge / narrow
def test_shapes_and_batch_sizes(gpu, cols, rows):
    cam = small_cam(cols, rows)
    vol = TSDFVolume(cols, rows, cam, max_units=256)
    for n in (1, 2, 64):                                                    # (64: bit 63 of the mask; the slots of the pipeline in turn)
        exp = check(vol, random_frames(cols, rows, n, 100 * cols + n), poses(n), cam, cols, rows)
        assert len(exp["keys"]) > 3 and int(exp["masks"].max()) >> (n - 1) == 1
    vol.close()


def test_workload_size_one_frame(gpu):
    cols, rows = 640, 480
    y, x = np.mgrid[0:rows, 0:cols]
    d = (900 + x + 2 * y + 300 * ((x // 50 + y // 30) % 2)).astype(np.uint16)
    d[np.random.RandomState(2).rand(rows, cols) < 0.0005] = 0
    d[100:140, 200:260] = 0                                                 # whole 16- and 32-pixel tiles without depth
    vol = TSDFVolume(max_units=512)
    exp = check(vol, d.reshape(1, -1), POSE0[None], R.DEFAULT_CAM, cols, rows)
    assert len(exp["keys"]) > 8 and (exp["tile_lo"] > 0).any() and (exp["tile_lo"] == 0).any()
    vol.close()


# ---- where the depth comes from ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,rows,offset", [(64, 32, 0), (36, 33, 0), (64, 32, 1), (64, 32, 3), (30, 21, 0)])
def test_rigid_device_depth(gpu, cols, rows, offset):
    """Device depth at an 8-byte aligned address (wide where cols % 4 == 0) and `offset` pixels behind one (narrow)."""
    import torch
    n, cam = 3, small_cam(cols, rows)
    d = random_frames(cols, rows, n, 7 + offset)
    buf = torch.zeros(n * cols * rows + 8, dtype=torch.int16, device="cuda:0")
    assert buf.data_ptr() % 8 == 0
    buf[offset:offset + d.size] = torch.from_numpy(d.view(np.int16).reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    vol = TSDFVolume(cols, rows, cam, max_units=256)
    check(vol, d, poses(n), cam, cols, rows, device_ptr=buf.data_ptr() + 2 * offset)
    vol.close()


def warp_case(cols, rows, n, special):
    res, length = 2, 3.0
    n1 = res + 1
    k, j, i = np.meshgrid(np.arange(n1), np.arange(n1), np.arange(n1), indexing="ij")
    verts = np.stack([i.ravel(), j.ravel(), k.ravel()], 1).astype(np.float64) * (length / res)
    squash = verts.copy()                                                   # (tests/test_tsdf_gpu.py: everything lands within 1.4 mm of the camera)
    squash[:, 2] = -0.3 + 0.0001 + (verts[:, 2] / length) * 0.0013
    squash[:, 0] = 1.5 + (verts[:, 0] - 1.5) * 0.0005
    squash[:, 1] = 1.5 + (verts[:, 1] - 1.5) * 0.0005
    mild = verts + np.random.RandomState(3).normal(0, 0.004, verts.shape)
    grids = np.stack([mild, squash]).astype(np.float32)
    seg = np.stack([synth.basepose(length)] * n)
    madj = np.stack([np.linalg.inv(seg[0])] * n)
    gi = np.array([1 if f in special else 0 for f in range(n)], np.int32)
    warp = dict(ctr=grids, resolution=res, length=np.float32(length), grid_index=gi, seg=seg, madj=madj)
    rng = np.random.RandomState(9)
    y, x = np.mgrid[0:rows, 0:cols]
    d = (1300 + 3 * (x % 97) + 2 * (y % 61))[None] + rng.randint(0, 200, (n, rows, cols))
    d[rng.rand(n, rows, cols) < 0.1] = 0
    return np.ascontiguousarray(d.reshape(n, -1), np.uint16), warp


def reprojected(vol_or_oracle, d, warp):
    w = warp
    return np.stack([vol_or_oracle.Reproject(d[f], w["ctr"][w["grid_index"][f]], w["resolution"], float(w["length"]), w["seg"][f], w["madj"][f])
                     for f in range(d.shape[0])])


@pytest.mark.parametrize("cols,rows,special", [(640, 480, ()), (640, 480, (1,)), (36, 33, (2,)), (30, 21, (1,))])
def test_warped(gpu, cols, rows, special):
    """The z-buffer as k_prepare's input: plain, and with one frame whose scatter wrote zeros (flagged, replayed: take_z per pixel).  What
    k_prepare must have read is the frame's re-projected depth: the oracle's at 640 x 480 (the reference's Reproject knows no other size);
    at the small sizes the volume's own single-frame Reproject, which consumes the z-buffer in a kernel of its own (k_zbuf_to_depth) and is
    held to the oracle at full size by tests/test_tsdf_gpu.py."""
    full = (cols, rows) == (640, 480)
    n, cam = (2 if full else 4), (np.array(R.DEFAULT_CAM, np.float32) if full else small_cam(cols, rows))
    d, warp = warp_case(cols, rows, n, special)
    vol = TSDFVolume(cols, rows, cam, max_units=512)
    if full:
        ora = OracleVolume()
        seen = reprojected(ora, d, warp)
        ora.close()
    else:
        seen = reprojected(vol, d, warp)
    for f in range(n):
        if f in special:
            assert (seen[f] == 1).any(), "the input does not reach the 0 / 1 mm boundary"
        else:
            assert (seen[f] > 400).sum() > rows * cols // 2
    for rep in range(3):                                                    # both pre-pass streams; the second visit of one meets re-armed buffers
        check(vol, d, poses(n), cam, cols, rows, warp=warp, seen=seen)
    vol.close()


# ---- data edges -------------------------------------------------------------------------------------------------------------------------
def test_extrema_edges(gpu):
    cols, rows = 64, 32
    cam = small_cam(cols, rows)
    d = np.full((3, rows, cols), UNIT_A, np.uint16)
    d[0, 20, 37] = 0                                       # frame 0: no depth in ONE 16-pixel sub-tile (tile 1, fine (1, 2))
    d[1, 9, 12] = 3000                                     # frame 1: beyond integration_trunc -> scaled 0, the key still touched
    d[1, 31, 63] = 65535
    d[2] = 0                                               # frame 2: no valid pixel at all
    vol = TSDFVolume(cols, rows, cam, max_units=64)
    exp = check(vol, d.reshape(3, -1), np.stack([POSE0] * 3), cam, cols, rows)
    fine, lo = exp["tile_lo_fine"], exp["tile_lo"]
    assert fine[1, 2, 0] == 0 and (np.delete(fine[:, :, 0].reshape(-1), 6) >= 1.0).all() and lo[0, 1, 0] == 0 and lo[0, 0, 0] >= 1.0
    assert fine[0, 0, 1] == 0 and fine[1, 3, 1] == 0 and exp["scaled"][1, 9 * cols + 12] == 0
    assert not exp["tile_max"][:, :, 2].any() and not fine[:, :, 2].any()
    assert len(exp["keys"]) >= 3 and all(int(m) & 4 == 0 for m in exp["masks"])       # frame 2 touches nothing; 3000 and 65535 mm touch units of their own
    only1 = [int(m) for m in exp["masks"] if int(m) == 2]
    assert len(only1) >= 2
    vol.close()


ISLANDS = [(4, 5), (3, 5), (7, 5), (0, 1), (0, 8), (0, 16), (16, 3), (31, 31), (32, 7), (60, 15), (28, 23), (1, 0)]


def test_unit_boundaries(gpu):
    """One pixel of unit B in a frame of unit A, at every kind of place a leader can stand: a thread's pixel 0 (its left neighbour is another
    thread's register), its pixels 1-3, column group 0 of an odd row (lane 8 of a DPP row), of a wave's first row, of the second sub-tile
    row, the first pixel of the right half, the tile's last pixel.  Then the boundaries as runs: between a thread's pixel 3 and the next
    thread's pixel 0, between two rows of a wave, at a wave border."""
    cols, rows = 64, 32
    cam = small_cam(cols, rows)
    n = len(ISLANDS) + 3
    d = np.full((n, rows, cols), UNIT_A, np.uint16)
    for f, (x, y) in enumerate(ISLANDS):
        d[f, y, x] = UNIT_B
    d[len(ISLANDS), :, 12:] = UNIT_B                       # columns 0-11 A, 12-63 B: the boundary between pixel 3 of one thread and pixel 0 of the next
    d[len(ISLANDS) + 1, 3:, :] = UNIT_B                    # rows 0-2 A: between two rows of a wave (and inside a DPP row)
    d[len(ISLANDS) + 2, 8:, :] = UNIT_B                    # rows 0-7 A: at a wave border
    vol = TSDFVolume(cols, rows, cam, max_units=64)
    exp = check(vol, d.reshape(n, -1), np.stack([POSE0] * n), cam, cols, rows)
    assert len(exp["keys"]) == 2 and all(int(m) == (1 << n) - 1 for m in exp["masks"])  # both units in every frame
    vol.close()


def test_alternating_units_take_the_direct_path(gpu):
    """Neighbouring pixels alternate between two units: 1024 leaders in a tile, more than the tile's list holds (kTileKeys = 96)."""
    cols, rows = 36, 33
    cam = small_cam(cols, rows)
    y, x = np.mgrid[0:rows, 0:cols]
    d = np.where((x + y) % 2 == 0, UNIT_A, UNIT_B).astype(np.uint16)
    d = np.stack([d, np.where(x % 2 == 0, UNIT_B, UNIT_A).astype(np.uint16)])
    vol = TSDFVolume(cols, rows, cam, max_units=64)
    exp = check(vol, d.reshape(2, -1), np.stack([POSE0] * 2), cam, cols, rows)
    assert len(exp["keys"]) == 2 and all(int(m) == 3 for m in exp["masks"])
    vol.close()


def test_out_of_range_pixels_are_counted(gpu):
    cols, rows = 36, 33
    cam = small_cam(cols, rows)
    d = random_frames(cols, rows, 2, 4)
    Ts = np.stack([pose(1.5, 1.5, 0.2), pose(1.5, 97.0, 0.2)])             # frame 1 beyond +-96 m: skipped and counted, but for the two pixels of 65535 mm
    vol = TSDFVolume(cols, rows, cam, max_units=256)
    exp = check(vol, d, Ts, cam, cols, rows)
    assert exp["out_of_range"] == int((d[1] != 0).sum()) - 2 and sum(1 for m in exp["masks"] if int(m) & 2) == 2
    vol.close()
