"""er_tsdf_raycast_batch / k_raycast_batch (csrc/er_tsdf_raycast.hip): a list of ray-casts in one launch.  Every job of every
call below is compared bit for bit -- records and depth -- with er_tsdf_raycast of the same job, and at least one job per test with the numpy
restatement (tests/raycast_restatement.py).  The volumes are the 4-frame 160 x 120 scene and the crafted units of tests/raycast_cases.py."""
import ctypes as C

import numpy as np
import pytest

import raycast_cases as rcc
import raycast_restatement as rcr
from odometry_cases import same_bits
from elasticreconstruction_amd import _ffi, synth
from elasticreconstruction_amd.tsdf import TSDFVolume, raycast_batch

pytestmark = pytest.mark.gpu
F = np.float32
_cache = {}
# the three levels of the odometry, then partial tiles: one pixel, less than a wave's 8 x 8 tile, partial workgroups (16 x 16) on either axis
SIZES = [(160, 120), (80, 60), (40, 30), (1, 1), (7, 5), (65, 3), (17, 33)]


def same_maps(a, b):
    return np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2])


def host(maps):
    dep, V, N = maps
    return synth.to_numpy_u16(dep).reshape(V.shape[:2]), V.cpu().numpy(), N.cpu().numpy()


def empty(maps):
    return not maps[0].any() and np.isnan(maps[1]).all() and np.isnan(maps[2]).all()


def volume_from_units(units, max_units=16):
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
    """(volume with the four frames integrated, its units for the restatement, poses, cam4): built once, never written again."""
    if "scene" not in _cache:
        d, W, cam, cam6 = rcc.scene_inputs()
        vol = TSDFVolume(rcc.SCENE_COLS, rcc.SCENE_ROWS, cam6, max_units=1024)
        vol.IntegrateFrames(d.reshape(len(d), -1), W)
        units = {int(k): vol.read_unit(int(k)) for k in vol.unit_keys()}
        _cache["scene"] = (vol, rcr.Volume(units), W, cam)
    return _cache["scene"]


def crafted_volume():
    if "crafted" not in _cache:
        c = rcc.identity_view()
        _cache["crafted"] = (volume_from_units(c["units"]), c)
    return _cache["crafted"]


def view_cam(cols, rows):
    _, _, _, cam = scene_volume()
    f = float(cam[0]) * max(cols, 40) / rcc.SCENE_COLS
    return (f, f, (cols - 1) / 2.0, (rows - 1) / 2.0)


def job(vol, T, cols, rows, cam, params=None):
    return dict(volume=vol, T=T, cols=cols, rows=rows, cam=cam, params=params)


def single(j):
    """The same job through er_tsdf_raycast, device outputs."""
    return host(j["volume"].raycast(j["T"], j["cols"], j["rows"], j["cam"], levels=1, params=j["params"], device=True)[0])


def run_and_compare(jobs):
    """One batch call; every job against the single call.  -> the batch's outputs on the host."""
    got = [host(m) for m in raycast_batch(jobs)]
    for q, j in enumerate(jobs):
        assert same_maps(got[q], single(j)), "job %d" % q
    return got


def restated(units, j):
    return rcr.raycast(units, j["cols"], j["rows"], j["cam"], j["T"], j["params"])


def test_levels_and_partial_tiles_in_one_call(gpu):
    vol, units, W, cam = scene_volume()
    jobs = [job(vol, W[1], c, r, tuple(np.asarray(cam, F) / F(rcc.SCENE_COLS // c)) if (c, r) in SIZES[:3] else view_cam(c, r)) for c, r in SIZES]
    got = run_and_compare(jobs)
    for q in (0, 2, 4, 6):
        assert same_maps(got[q], restated(units, jobs[q])), q
    assert np.isfinite(got[0][1]).any() and not empty(got[2])


def test_one_volume_twice_a_second_volume_and_empty_ones(gpu):
    vol, units, W, cam = scene_volume()
    cvol, c = crafted_volume()
    fresh = TSDFVolume(max_units=8)
    was = volume_from_units(c["units"])
    was.reset()
    k = view_cam(40, 30)
    jobs = [job(vol, W[1], 40, 30, k), job(cvol, c["T"], c["cols"], c["rows"], c["cam"], c["params"]), job(vol, rcc.novel_pose(), 40, 30, k),
            job(fresh, c["T"], c["cols"], c["rows"], c["cam"], c["params"]), job(was, c["T"], c["cols"], c["rows"], c["cam"], c["params"])]
    got = run_and_compare(jobs)
    assert same_maps(got[1], restated(c["units"], jobs[1])) and same_maps(got[2], restated(units, jobs[2]))
    assert not empty(got[0]) and not empty(got[1]) and not same_maps(got[0], got[2])
    assert empty(got[3]) and empty(got[4])
    fresh.close()
    was.close()


def test_bad_poses_leave_their_neighbours_alone(gpu):
    vol, units, W, cam = scene_volume()
    k = view_cam(17, 13)
    nan, far = W[1].copy(), W[1].copy()
    nan[1, 3] = np.nan
    far[:3, 3] += [200.0, 0.0, 0.0]
    good = [job(vol, W[1], 17, 13, k), job(vol, W[2], 17, 13, k)]
    alone = run_and_compare(good)
    got = run_and_compare([good[0], job(vol, nan, 17, 13, k), job(vol, far, 17, 13, k), good[1]])
    assert same_maps(got[0], alone[0]) and same_maps(got[3], alone[1]) and not empty(got[0])
    assert empty(got[1]) and empty(got[2])
    assert same_maps(got[0], restated(units, good[0]))


def test_jobs_with_their_own_ranges_and_a_call_of_one_job(gpu):
    cvol, c = crafted_volume()
    args = (cvol, c["T"], c["cols"], c["rows"], c["cam"])
    one_step = (0.0, 0.02, 0.024)
    assert rcr.count_steps(*one_step) == 1
    jobs = [job(*args, params=c["params"]), job(*args, params=one_step), job(*args, params=(0.0, 4.0, rcc.UL)), job(*args, params=(1.0, 1.0, 0.01)),
            job(*args)]
    got = run_and_compare(jobs)
    assert same_maps(got[2], restated(c["units"], jobs[2])) and not empty(got[0]) and empty(got[1]) and empty(got[3])
    assert same_maps(got[4], got[0]), "no params: the defaults, which are this case's"
    alone = run_and_compare(jobs[2:3])
    assert same_maps(alone[0], got[2]) and same_maps(alone[0], restated(c["units"], jobs[2]))
    assert same_maps(run_and_compare(jobs)[2], got[2]), "two runs, the same bits"


def test_no_job_is_a_no_op_and_depth_is_optional(gpu):
    import torch
    cvol, c = crafted_volume()
    assert raycast_batch([]) == []
    L = _ffi.lib()
    rec = torch.full((c["rows"], c["cols"], 2, 4), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    vols, rp = (C.c_void_p * 1)(cvol._h.value), (C.c_void_p * 1)(rec.data_ptr())
    one = np.array([c["cols"]], np.int32)
    assert L.er_tsdf_raycast_batch(0, vols, _ffi.ptr(one), _ffi.ptr(one), None, None, None, rp, None) == 0
    assert bool((rec == 7.0).all()), "untouched"
    j = job(cvol, c["T"], c["cols"], c["rows"], c["cam"], c["params"])
    dep, V, N = raycast_batch([j], depth=False)[0]
    want = restated(c["units"], j)
    assert dep is None and same_bits(V.cpu().numpy(), want[1]) and same_bits(N.cpu().numpy(), want[2])


def test_order_behind_integration_and_on_a_callers_stream(gpu):
    import torch
    d, W, cam, cam6 = rcc.scene_inputs()
    ref_vol, units, _, _ = scene_volume()
    j = job(ref_vol, W[3], rcc.SCENE_COLS, rcc.SCENE_ROWS, cam)
    want = run_and_compare([j])[0]
    assert same_maps(want, restated(units, j))
    vol = TSDFVolume(rcc.SCENE_COLS, rcc.SCENE_ROWS, cam6, max_units=1024)
    vol.IntegrateFrames(d.reshape(len(d), -1), W)
    first = host(raycast_batch([dict(j, volume=vol)])[0])               # straight after the call, no synchronize(): every frame is in
    assert same_maps(first, want)
    vol.close()
    stream = torch.cuda.Stream()
    vol = TSDFVolume(rcc.SCENE_COLS, rcc.SCENE_ROWS, cam6, max_units=1024)
    vol.set_stream(stream.cuda_stream)
    vol.IntegrateFrames(d.reshape(len(d), -1), W)
    both = [host(m) for m in raycast_batch([dict(j, volume=vol), j])]
    assert same_maps(both[0], want) and same_maps(both[1], want), "on a caller's stream, beside a volume on its own"
    vol.set_stream(None)
    vol.close()


def test_refusals_name_the_job(gpu):
    import torch
    cvol, c = crafted_volume()
    args = (cvol, c["T"], c["cols"], c["rows"], c["cam"])
    with pytest.raises(_ffi.ErError, match="job 1: more than 65536 steps"):
        raycast_batch([job(*args), job(*args, params=(0.0, 1.0, 1.0 / 65537))])
    with pytest.raises(_ffi.ErError, match="job 2: t_min"):
        raycast_batch([job(*args), job(*args), job(*args, params=(0.0, np.inf, 0.1))])
    with pytest.raises(_ffi.ErError, match="job 0: an image of 0 x 5"):
        raycast_batch([job(cvol, c["T"], 0, 5, c["cam"])])
    L = _ffi.lib()
    n = 2
    rec = torch.full((n, c["rows"], c["cols"], 2, 4), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    vols = (C.c_void_p * n)(*[cvol._h.value] * n)
    cols, rows = np.full(n, c["cols"], np.int32), np.full(n, c["rows"], np.int32)
    cam = np.ascontiguousarray(np.tile(np.asarray(c["cam"], F), (n, 1)))
    T = np.ascontiguousarray(np.tile(c["T"].reshape(1, 16), (n, 1)))
    rp = (C.c_void_p * n)(rec[0].data_ptr(), None)
    call = lambda count, v, r, dp: L.er_tsdf_raycast_batch(count, v, _ffi.ptr(cols), _ffi.ptr(rows), _ffi.ptr(cam), _ffi.ptr(T), None, r, dp)   # noqa: E731
    assert call(n, vols, rp, None) != 0 and b"job 1: both outputs are NULL" in L.er_last_error()
    assert call(n, (C.c_void_p * n)(cvol._h.value, None), rp, None) != 0 and b"job 1: NULL handle" in L.er_last_error()
    assert call(65536, vols, rp, None) != 0 and b"at most 65535" in L.er_last_error()
    assert bool((rec == 7.0).all()), "a refused call launches nothing"


def test_volumes_of_two_devices_are_refused(gpu):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    cvol, c = crafted_volume()
    other = TSDFVolume(max_units=8, device=1)
    with pytest.raises(_ffi.ErError, match="job 1: its volume is on device 1"):
        raycast_batch([job(cvol, c["T"], c["cols"], c["rows"], c["cam"]), job(other, c["T"], c["cols"], c["rows"], c["cam"])])
    other.close()
