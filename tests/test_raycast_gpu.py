"""The ray caster on the device (csrc/er_tsdf_raycast.hip) against the numpy restatement (tests/raycast_restatement.py), bit for
bit: depth, vertex, normal and the NaN pattern.  The restatement marches every step; the kernel skips through units that do not exist -- the
equality below is what proves the skip.  The volumes are the 4-frame 160 x 120 scene (integrated on the device, read back with read_unit for
the restatement) and the crafted units of tests/raycast_cases.py (er_tsdf_import_raw)."""
import numpy as np
import pytest

import raycast_cases as rcc
import raycast_restatement as rcr
from odometry_cases import same_bits
from elasticreconstruction_amd import _ffi, synth
from elasticreconstruction_amd.tsdf import TSDFVolume

pytestmark = pytest.mark.gpu
F = np.float32
_cache = {}

CRAFTED = dict(rcc.crafted(), plane=rcc.plane(), sphere_default_step=rcc.sphere_default_step())
# cols x rows: the three levels of the odometry, one pixel, less than a wave's 8 x 8 tile, and partial tiles and workgroups (16 x 16) on either axis
SIZES = [(160, 120), (80, 60), (40, 30), (1, 1), (7, 5), (65, 3), (17, 33)]


def same_maps(a, b):
    return np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2])


def volume_from_units(units, max_units=16):
    """A TSDFVolume that holds exactly `units` (er_tsdf_import_raw)."""
    import torch
    vol = TSDFVolume(max_units=max_units)
    if units:
        keys = np.array(sorted(units), np.int32)
        raw = np.stack([np.stack([units[int(k)][0], units[int(k)][1]]) for k in keys]).astype(F)
        buf = torch.from_numpy(raw).to("cuda:0")
        torch.cuda.synchronize()
        vol.import_raw(keys, buf.data_ptr())
        vol.synchronize()
    return vol


def scene_volume():
    """(volume with the four frames integrated, its units read back, poses, cam4): built once, never written again."""
    if "scene" not in _cache:
        d, W, cam, cam6 = rcc.scene_inputs()
        vol = TSDFVolume(rcc.SCENE_COLS, rcc.SCENE_ROWS, cam6, max_units=1024)
        vol.IntegrateFrames(d.reshape(len(d), -1), W)
        units = {int(k): vol.read_unit(int(k)) for k in vol.unit_keys()}
        _cache["scene"] = (vol, rcr.Volume(units), W, cam)
    return _cache["scene"]


def view_cam(cols, rows):
    """The scene's focal length scaled to `cols`, the principal point in the middle of the image."""
    _, _, _, cam = scene_volume()
    f = float(cam[0]) * cols / rcc.SCENE_COLS if cols >= 40 else float(cam[0]) * 40 / rcc.SCENE_COLS
    return (f, f, (cols - 1) / 2.0, (rows - 1) / 2.0)


def one(vol, T, cols, rows, cam, params=None, device=False):
    dep, V, N = vol.raycast(T, cols, rows, cam, levels=1, params=params, device=device)[0]
    if device:
        return synth.to_numpy_u16(dep).reshape(rows, cols), V.cpu().numpy(), N.cpu().numpy()
    return dep, V, N


def empty(maps):
    return not maps[0].any() and np.isnan(maps[1]).all() and np.isnan(maps[2]).all()


# ---- sizes and poses ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", ["integration", "novel"])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_scene_equals_restatement_at_every_size(gpu, size, pose):
    vol, units, W, cam = scene_volume()
    cols, rows = size
    T = W[1] if pose == "integration" else rcc.novel_pose()
    k = view_cam(cols, rows)
    st = {}
    want = rcr.raycast(units, cols, rows, k, T, stats=st)
    assert st["hits"] > 0 and st["samples"] > 20 * cols * rows, "rays meet the surface, after a march through empty space"
    assert same_maps(one(vol, T, cols, rows, k), want)


def test_levels_are_the_odometry_levels(gpu):
    vol, units, W, cam = scene_volume()
    lv = vol.raycast(W[2], rcc.SCENE_COLS, rcc.SCENE_ROWS, cam, levels=3)
    want = rcr.raycast_levels(units, rcc.SCENE_COLS, rcc.SCENE_ROWS, cam, W[2], 3)
    assert len(lv) == 3
    for l in range(3):
        assert lv[l][0].shape == (rcc.SCENE_ROWS >> l, rcc.SCENE_COLS >> l) and same_maps(lv[l], want[l]), l


# ---- crafted units ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_units_equal_restatement(gpu, name):
    c = CRAFTED[name]
    vol = volume_from_units(c["units"])
    want = rcr.raycast(c["units"], c["cols"], c["rows"], c["cam"], c["T"], c["params"])
    got = one(vol, c["T"], c["cols"], c["rows"], c["cam"], c["params"])
    vol.close()
    assert same_maps(got, want)
    if name.endswith("neighbour_absent"):
        assert np.isfinite(got[1]).all() and np.isnan(got[2]).all()
    if name == "back_face_first":
        assert empty(got)


# ---- rays and ranges ------------------------------------------------------------------------------------------------------------------------------
def test_far_nan_and_huge_poses_give_an_empty_image(gpu):
    vol, units, W, cam = scene_volume()
    k = view_cam(17, 13)
    far = W[1].copy()
    far[:3, 3] += [200.0, 0.0, 0.0]                           # off the lattice (+-96 m): every sample is unobserved
    nan = W[1].copy()
    nan[1, 3] = np.nan
    nanr = W[1].copy()
    nanr[0, 0] = np.nan
    huge = W[1].copy()
    huge[:3, 3] = 1e30
    huger = W[1].copy()
    huger[:3, :3] *= 1e30
    for T in (far, nan, nanr, huge, huger):
        got = one(vol, T, 17, 13, k)
        assert empty(got)
        assert same_maps(got, rcr.raycast(units, 17, 13, k, T))


def test_ranges_and_step_counts(gpu):
    c = rcc.exact_zero()                                      # the camera sits inside the unit, 0.2 m in front of the surface
    vol = volume_from_units(c["units"])
    args = (c["T"], c["cols"], c["rows"], c["cam"])
    for params in ((1.0, 1.0, 0.01), (2.0, 1.0, 0.01)):       # t_max <= t_min: no step, an empty image
        assert rcr.count_steps(*params) == 0 and empty(one(vol, *args, params=params))
    one_step = (0.0, 0.02, 0.024)
    assert rcr.count_steps(*one_step) == 1 and empty(one(vol, *args, params=one_step))
    most = (0.0, 1.0, 1.0 / 65536)                            # 65536 steps of 15 um; the rays meet the surface after 13600 of them
    assert rcr.count_steps(*most) == 65536
    got = one(vol, *args, params=most)
    assert np.isfinite(got[1]).all() and same_maps(got, rcr.raycast(c["units"], c["cols"], c["rows"], c["cam"], c["T"], most))
    away = c["T"].copy()
    away[:3, :3] = c["T"][:3, :3] @ np.diag([1.0, -1.0, -1.0])        # facing away from the surface: all 65536 samples, and nothing
    assert empty(one(vol, away, 1, 1, c["cam"], params=most))
    with pytest.raises(_ffi.ErError, match="65536"):
        one(vol, *args, params=(0.0, 1.0, 1.0 / 65537))
    for bad in ((0.0, 1.0, 0.0), (0.0, np.inf, 0.1), (np.nan, 1.0, 0.1)):
        with pytest.raises(_ffi.ErError):
            one(vol, *args, params=bad)
    with pytest.raises(_ffi.ErError):
        one(vol, c["T"], 0, 5, c["cam"])
    vol.close()


# ---- volume states ----------------------------------------------------------------------------------------------------------------------------------
def test_empty_dropped_and_reset_volumes(gpu):
    c = rcc.identity_view()
    args = (c["T"], c["cols"], c["rows"], c["cam"], c["params"])
    fresh = TSDFVolume(max_units=8)
    assert empty(one(fresh, *args))
    fresh.close()
    vol = volume_from_units(c["units"])
    assert not empty(one(vol, *args))
    gone = rcc.key_of(256, 256, 256)
    vol.drop_units([gone])                                    # zeroed, still in the table: unobserved like a unit that does not exist
    want = rcr.raycast({k: u for k, u in c["units"].items() if k != gone}, c["cols"], c["rows"], c["cam"], c["T"], c["params"])
    got = one(vol, *args)
    assert same_maps(got, want) and np.isfinite(got[1]).any() and not np.isfinite(got[1]).all()
    vol.drop_units(sorted(c["units"]))
    assert empty(one(vol, *args))
    vol.close()
    vol = volume_from_units(c["units"])
    vol.reset()
    assert empty(one(vol, *args))
    vol.close()


# ---- ordering and reproducibility ---------------------------------------------------------------------------------------------------------------------
def test_order_behind_integration_streams_and_outputs(gpu):
    import torch
    d, W, cam, cam6 = rcc.scene_inputs()
    ref_vol, units, _, _ = scene_volume()
    args = (W[3], rcc.SCENE_COLS, rcc.SCENE_ROWS, cam)
    want = one(ref_vol, *args)
    assert same_maps(want, rcr.raycast(units, rcc.SCENE_COLS, rcc.SCENE_ROWS, cam, W[3]))
    assert same_maps(one(ref_vol, *args), want), "two runs, the same bits"
    assert same_maps(one(ref_vol, *args, device=True), want), "device outputs equal host outputs"
    vol = TSDFVolume(rcc.SCENE_COLS, rcc.SCENE_ROWS, cam6, max_units=1024)
    vol.IntegrateFrames(d.reshape(len(d), -1), W)
    first = one(vol, *args)                                   # straight after the call, no synchronize(): every frame is in
    vol.synchronize()
    assert same_maps(first, want) and same_maps(one(vol, *args), want)
    vol.close()
    stream = torch.cuda.Stream()
    vol = TSDFVolume(rcc.SCENE_COLS, rcc.SCENE_ROWS, cam6, max_units=1024)
    vol.set_stream(stream.cuda_stream)
    vol.IntegrateFrames(d.reshape(len(d), -1), W)
    assert same_maps(one(vol, *args), want), "on a caller's stream"
    assert same_maps(one(vol, *args, device=True), want)
    vol.set_stream(None)
    vol.close()
