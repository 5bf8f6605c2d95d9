"""What a batch does only to hand itself over: the epoch-tagged z-buffer (nobody re-arms it: a cell counts only under the tag of the batch or
frame that reads it) and k_plan as the one that clears the frame masks, the unit list and its length and accounts the unit visits.  Checked
through er_tsdf_prepass_trace against tests/prepass_restatement.py, with tests/test_prepass_gpu.py's harness; what k_prepare must have read on
the warped path is each frame's re-projected depth from a z-buffer that was filled just before (`fresh_reprojected`: er_tsdf_reset refills it),
so the expectation never depends on a tag compare."""
import re

import numpy as np
import pytest

import prepass_restatement as R
import test_prepass_gpu as P
import test_tsdf_gpu
from elasticreconstruction_amd import _ffi, synth
from elasticreconstruction_amd.tsdf import TSDFVolume

pytestmark = pytest.mark.gpu

SHAPES = [(36, 20), (64, 8)]                                  # the narrow instantiation (a partial tile on both axes), the wide one


def warp_of(n, special=()):
    return P.warp_case(8, 8, n, special)[1]                   # (the lattices and matrices do not depend on the image size)


def frames(cols, rows, n, seed, holes):
    """Depths on both sides of a unit boundary and in between, `holes` of the pixels without depth: what one frame leaves in a cell differs
    from what the next one writes there, in both directions, and many cells of a frame stay unwritten."""
    rng = np.random.RandomState(seed)
    d = rng.randint(700, 2300, (n, rows * cols))
    d[rng.rand(n, rows * cols) < holes] = 0
    return np.ascontiguousarray(d, np.uint16)


def fresh_reprojected(ref, d, warp):
    out = []
    for f in range(d.shape[0]):
        ref.reset()                                           # z-buffer filled, counter at 0: no stale cell under this frame
        out.append(ref.Reproject(d[f], warp["ctr"][warp["grid_index"][f]], warp["resolution"], float(warp["length"]), warp["seg"][f], warp["madj"][f]))
    return np.stack(out)


@pytest.mark.parametrize("cols,rows", SHAPES)
def test_shapes_batches_and_reuse(gpu, cols, rows):
    """Batches of 1, 2, 3 and 64 frames, twice, on one handle: each z-buffer is scattered into four times and each pipeline slot two or three
    times, every time under cells that other frames left; then the same slots on the rigid path."""
    cam = P.small_cam(cols, rows)
    vol, ref = TSDFVolume(cols, rows, cam, max_units=256), TSDFVolume(cols, rows, cam, max_units=1)
    visits = 0
    vol.set_profiling(1)
    for call, n in enumerate((1, 2, 3, 64, 1, 2, 3, 64)):
        d, warp = frames(cols, rows, n, 10 * cols + call, (0.05, 0.5, 0.2, 0.8)[call % 4]), warp_of(n)
        seen = fresh_reprojected(ref, d, warp)
        assert (seen > 0).any() and (seen == 0).any()
        exp = P.check(vol, d, P.poses(n), cam, cols, rows, warp=warp, seen=seen)
        assert len(exp["keys"]) > 1
        visits += sum(bin(int(m)).count("1") for m in exp["masks"])
    for call, n in enumerate((3, 1, 64)):
        d = frames(cols, rows, n, 77 + call, 0.3)
        exp = P.check(vol, d, P.poses(n), cam, cols, rows)
        visits += sum(bin(int(m)).count("1") for m in exp["masks"])
    assert vol.get_profile()["unit_visits"] == visits
    vol.close()
    ref.close()


@pytest.mark.parametrize("cols,rows", SHAPES)
def test_stale_cells_read_as_empty(gpu, cols, rows):
    """Batch 0 and batch 2 share a z-buffer.  Batch 0 writes 900 mm into every cell; batch 2 writes 2100 mm into every third pixel and nothing
    elsewhere: where it writes, the stale value is the SMALLER one (a plain atomicMin would keep it), elsewhere the cell must read as empty."""
    cam = P.small_cam(cols, rows)
    vol, ref = TSDFVolume(cols, rows, cam, max_units=64), TSDFVolume(cols, rows, cam, max_units=1)
    n = 3
    warp = warp_of(n)
    dense = np.full((n, rows * cols), 900, np.uint16)
    sparse = np.zeros((n, rows * cols), np.uint16)
    sparse[:, ::3] = 2100
    seen_dense, seen_sparse = fresh_reprojected(ref, dense, warp), fresh_reprojected(ref, sparse, warp)
    assert (seen_dense > 0).mean() > 0.5 and ((seen_sparse == 0) & (seen_dense > 0)).sum() > n * rows * cols // 4
    both = (seen_sparse > 0) & (seen_dense > 0)
    assert both.any() and (seen_sparse[both] > seen_dense[both]).all()
    P.check(vol, dense, P.poses(n), cam, cols, rows, warp=warp, seen=seen_dense)          # z-buffer 0
    P.check(vol, dense, P.poses(n), cam, cols, rows, warp=warp, seen=seen_dense)          # z-buffer 1
    P.check(vol, sparse, P.poses(n), cam, cols, rows, warp=warp, seen=seen_sparse)        # z-buffer 0 again
    P.check(vol, sparse, P.poses(n), cam, cols, rows, warp=warp, seen=seen_sparse)        # z-buffer 1 again
    # the single-frame consumer of z-buffer 0 (k_zbuf_to_depth) over what the batches left, then a batch over what it left
    for d, seen in ((dense, seen_dense), (sparse, seen_sparse)):
        got = vol.Reproject(d[1], warp["ctr"][0], warp["resolution"], float(warp["length"]), warp["seg"][1], warp["madj"][1])
        assert np.array_equal(got, seen[1])
    P.check(vol, sparse, P.poses(n), cam, cols, rows, warp=warp, seen=seen_sparse)
    vol.close()
    ref.close()


@pytest.mark.parametrize("cols,rows", SHAPES)
def test_epoch_wrap(gpu, cols, rows):
    """The counters of both z-buffers start at 65 533: six batches use the epochs 65 534, 65 535 and -- behind the refill -- 1 of each buffer.
    Then the same for the single-frame Reproject (z-buffer 0) and for the colour reprojection's own buffer."""
    cam = P.small_cam(cols, rows)
    vol, ref = TSDFVolume(cols, rows, cam, max_units=256), TSDFVolume(cols, rows, cam, max_units=1)
    n = 3
    warp = warp_of(n)
    vol.set_zbuf_epoch(0, 65533)
    vol.set_zbuf_epoch(1, 65533)
    for call in range(6):
        d = frames(cols, rows, n, 500 + call, (0.1, 0.6)[call // 2 % 2])
        P.check(vol, d, P.poses(n), cam, cols, rows, warp=warp, seen=fresh_reprojected(ref, d, warp))
    args = (warp["ctr"][0], warp["resolution"], float(warp["length"]), warp["seg"][0], warp["madj"][0])
    vol.set_zbuf_epoch(0, 65533)
    vol.set_zbuf_epoch(2, 65533)
    rng = np.random.RandomState(8)
    for call in range(6):
        d = frames(cols, rows, 1, 600 + call, (0.1, 0.6)[call % 2])[0]
        rgb = rng.randint(0, 256, (rows * cols, 3)).astype(np.uint8)
        ref.reset()
        want = ref.Reproject(d, *args)
        assert np.array_equal(vol.Reproject(d, *args), want), "Reproject, call %d" % call
        zc, cc = vol.ReprojectColor(d, rgb, *args)
        zr, cr = ref.ReprojectColor(d, rgb, *args)                         # (a colour call fills its z-buffer first; this one stays far from the wrap)
        assert np.array_equal(zc, want) and np.array_equal(zr, want) and np.array_equal(cc, cr), "ReprojectColor, call %d" % call
    with pytest.raises(_ffi.ErError, match="epoch"):
        vol.set_zbuf_epoch(0, 65536)
    vol.close()
    ref.close()


def test_color_frames_across_the_wrap(gpu):
    """er_tsdf_color_frames warps its frames one after the other through ONE z-buffer, an epoch each: six frames whose holes differ, the counter
    started at 65 533, against the same frames splatted one call each (a call fills the buffer first)."""
    cols, rows = 36, 20
    cam = P.small_cam(cols, rows)
    n = 6
    warp = warp_of(n)
    d = np.concatenate([frames(cols, rows, 1, 700 + f, (0.1, 0.7)[f % 2]) for f in range(n)])
    rgb = np.random.RandomState(3).randint(0, 256, (n, rows * cols, 3)).astype(np.uint8)
    Ts = P.poses(n)
    acc = []
    for one_call in (True, False):
        vol = TSDFVolume(cols, rows, cam, max_units=64)
        vol.IntegrateFrames(d, Ts, warp)
        vol.enable_color()
        vol.set_zbuf_epoch(2, 65533)
        if one_call:
            st = vol.ColorFrames(d, rgb, Ts, warp)
        else:
            st = np.sum([vol.ColorFrames(d[f:f + 1], rgb[f:f + 1], Ts[f:f + 1], dict(warp, grid_index=warp["grid_index"][f:f + 1], seg=warp["seg"][f:f + 1],
                                                                                     madj=warp["madj"][f:f + 1])) for f in range(n)], axis=0)
        acc.append((tuple(int(x) for x in st), [vol.read_unit_color(k) for k in vol.unit_keys()]))
        vol.close()
    assert acc[0][0] == acc[1][0] and acc[0][0][0] > 0
    assert len(acc[0][1]) == len(acc[1][1]) > 0 and all(np.array_equal(a, b) for a, b in zip(acc[0][1], acc[1][1]))


# ---- dd == 0: the existing zero-write fixtures over stale cells ---------------------------------------------------------------------------
class StaleVolume(TSDFVolume):
    """A volume whose two z-buffers hold, in every frame of a 40-frame batch, what dense frames left there -- and nothing else: the frames lie
    500 m away, where every pixel is out of range, so no unit is touched and the volume is still empty."""

    def __init__(self, *a, **kw):
        TSDFVolume.__init__(self, *a, **kw)
        n, px = 40, self.cols_ * self.rows_
        res, length = 2, 3.0
        k, j, i = np.meshgrid(np.arange(res + 1), np.arange(res + 1), np.arange(res + 1), indexing="ij")
        grid = (np.stack([i.ravel(), j.ravel(), k.ravel()], 1) * (length / res)).astype(np.float32)[None]
        seg = np.stack([synth.basepose(length)] * n)
        warp = dict(ctr=grid, resolution=res, length=np.float32(length), grid_index=np.zeros(n, np.int32), seg=seg,
                    madj=np.stack([np.linalg.inv(seg[0])] * n))
        d = np.random.RandomState(12).randint(400, 3000, (n, px)).astype(np.uint16)
        far = np.stack([P.pose(1.5, 500.0, 0.2)] * n)
        for batch in range(2):
            self.IntegrateFrames(d, far, warp)
        self.synchronize()                                                              # (status is a poll)
        flags, out_of_range = self.status()
        assert self.unit_count() == 0 and flags == 0 and out_of_range > n * px         # (most cells of both z-buffers were written)


@pytest.mark.parametrize("fixture", [test_tsdf_gpu.test_reproject_zero_depth_reset_semantics, test_tsdf_gpu.test_reproject_zero_depth_reset_inside_a_batch])
def test_zero_depth_fixtures_over_stale_cells(gpu, monkeypatch, fixture):
    monkeypatch.setattr(test_tsdf_gpu, "TSDFVolume", StaleVolume)
    fixture(gpu)


# ---- counters ------------------------------------------------------------------------------------------------------------------------------
# unit_visits after each call, the units requested and the status flags at the end, of the sequence below on the commit before k_reset was
# folded into k_plan (recorded from a run of that commit's library)
PARENT_COUNTERS = dict(unit_visits=[97, 1088, 1122, 1190, 1325], units_requested=152, flags=1)


def counter_sequence():
    cols, rows = 36, 20
    cam = P.small_cam(cols, rows)
    vol = TSDFVolume(cols, rows, cam, max_units=2)
    vol.set_profiling(1)
    visits, want = [], 0
    for call, n in enumerate((3, 64, 1, 2, 5)):
        d = P.random_frames(cols, rows, n, 40 + call)
        vol.IntegrateFrames(d, P.poses(n))
        visits.append(vol.get_profile()["unit_visits"])
        want += sum(bin(int(m)).count("1") for m in R.products(d, P.poses(n), cam, cols, rows)["masks"])
        assert visits[-1] == want
    with pytest.raises(_ffi.ErError, match="pool exhausted") as e:
        vol.unit_count()
    requested = int(re.search(r"(\d+) units requested", str(e.value)).group(1))
    flags = vol.status()[0]
    vol.close()
    return dict(unit_visits=visits, units_requested=requested, flags=flags)


def test_counters_with_a_pool_too_small(gpu):
    got = counter_sequence()
    print("counters:", got)
    assert got["units_requested"] > 2 and got["flags"] == 1                 # ER_STATUS_POOL_EXHAUSTED, the table not full
    assert got == PARENT_COUNTERS


def test_empty_batch_leaves_plan_and_counters_clean(gpu):
    cols, rows = 36, 20
    cam = P.small_cam(cols, rows)
    vol = TSDFVolume(cols, rows, cam, max_units=64)
    vol.set_profiling(1)
    n = 3
    d = frames(cols, rows, n, 5, 0.2)
    warp = warp_of(n)
    first = P.check(vol, d, P.poses(n), cam, cols, rows)
    visits = vol.get_profile()["unit_visits"]
    assert visits == sum(bin(int(m)).count("1") for m in first["masks"]) > 0
    for w in (None, warp, None):                                            # the three slots, one of them through the z-buffer
        tr = vol.prepass_trace(np.zeros_like(d), P.poses(n), w)
        assert len(tr["keys"]) == 0 and not tr["scaled"].any() and not tr["tile_max"].any()
    assert vol.get_profile()["unit_visits"] == visits and vol.unit_count() == len(first["keys"])
    again = P.check(vol, d, P.poses(n), cam, cols, rows)                    # slot 1 again: the same plan as at first
    assert np.array_equal(again["keys"], first["keys"]) and vol.get_profile()["unit_visits"] == 2 * visits
    assert vol.status()[0] == 0
    vol.close()
