"""Colour on the device against its numpy restatement (tests/color_restatement.py): the accumulators of every unit bit for bit,
their independence of batch split, order and run, the warped colour image, the sampler on crafted accumulators, the coloured mesh, and the
lifecycle.  64 x 48 and 37 x 29 images (37 * 29 = 1073 pixels: no multiple of 64, more than one workgroup), pools of at most 64 units."""
import ctypes as C
import os

import numpy as np
import pytest

import color_cases as cc
import color_restatement as cr
from elasticreconstruction_amd import _ffi
from helpers import assert_volumes_identical

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UL = cr.UL
KEY0 = cc.KEY0


def volume(sc, frames=None, color=True, max_units=64):
    from elasticreconstruction_amd.tsdf import TSDFVolume
    vol = TSDFVolume(sc["cols"], sc["rows"], sc["cam"], max_units=max_units)
    f = slice(None) if frames is None else frames
    vol.IntegrateFrames(sc["depth"][f], sc["poses"][f])
    if color:
        vol.enable_color()
    return vol


def read_all(vol):
    return {int(k): vol.read_unit_color(int(k)) for k in vol.unit_keys()}


def assert_same(got, want, what=""):
    assert sorted(got) == sorted(want), what
    for k in want:
        bad = int((got[k] != want[k]).any(axis=1).sum())
        assert bad == 0, "%s unit %d: %d voxels differ" % (what, k, bad)


def expected(sc, keys, frames=None):
    units = cr.empty_units(keys)
    idx = range(len(sc["poses"])) if frames is None else frames
    st = np.zeros(3, np.int64)
    for f in idx:
        st += cr.splat(units, sc["depth"][f], sc["rgb"][f], sc["poses"][f], sc["cam"], sc["cols"], sc["rows"])
    return units, tuple(int(x) for x in st)


@pytest.fixture(scope="module")
def room(gpu):
    """The room with the sphere at 64 x 48, its restatement computed once."""
    sc = cc.room_with_sphere(64, 48)
    vol = volume(sc)
    keys = [int(k) for k in vol.unit_keys()]
    vol.close()
    want, st = expected(sc, keys)
    return sc, keys, want, st


# ---- the accumulators, bit for bit -------------------------------------------------------------------------------------------------------

SCENES = {"room 64x48": lambda: cc.room_with_sphere(64, 48), "room 37x29": lambda: cc.room_with_sphere(37, 29),
          "negative corner 64x48": lambda: cc.negative_corner(64, 48), "negative corner 37x29": lambda: cc.negative_corner(37, 29)}


@pytest.mark.parametrize("name", list(SCENES))
def test_accumulators_of_every_unit_equal_the_restatement(gpu, name):
    sc = SCENES[name]()
    vol = volume(sc)
    keys = [int(k) for k in vol.unit_keys()]
    assert 4 <= len(keys) <= 64
    st = vol.ColorFrames(sc["depth"], sc["rgb"], sc["poses"])
    want, wst = expected(sc, keys)
    assert st == wst and st[0] > 0 and st[1] == 0 and st[2] == 0, (st, wst)
    got = read_all(vol)
    assert_same(got, want, name)
    assert sum(int(u[:, 3].sum()) for u in got.values()) == st[0]
    assert sum(1 for u in got.values() if u[:, 3].any()) >= 4                      # the surface spans several units
    vol.close()


def test_a_one_pixel_image(gpu):
    from elasticreconstruction_amd.tsdf import TSDFVolume
    cam = np.array([100.0, 100.0, 0.0, 0.0, 2.5, 2.5], np.float32)
    T = np.eye(4)
    T[:3, 3] = [-1 * UL, 20 * UL, 63 * UL - 1.0]
    depth, rgb = np.array([[1000]], np.uint16), np.array([[[10, 20, 255]]], np.uint8)
    vol = TSDFVolume(1, 1, cam, max_units=16)
    vol.IntegrateFrames(depth, T[None])
    vol.enable_color()
    keys = [int(k) for k in vol.unit_keys()]
    key = KEY0 - (1 << 18)
    assert key in keys
    assert vol.ColorFrames(depth, rgb, T[None]) == (1, 0, 0)
    want = cr.empty_units(keys)
    assert cr.splat(want, depth[0], rgb[0], T, cam, 1, 1) == (1, 0, 0)
    assert want[key][(63 * 64 + 20) * 64 + 63].tolist() == [10, 20, 255, 1]
    assert_same(read_all(vol), want)
    vol.close()


@pytest.mark.parametrize("shape", [(64, 48), (37, 29)], ids=["64x48", "37x29"])
def test_contention_every_pixel_of_a_frame_in_one_voxel(gpu, shape):
    """Colour 255 255 255 from every pixel into one voxel, three times over: the sums are exact and nothing carries between the packed fields."""
    from elasticreconstruction_amd.tsdf import TSDFVolume
    cols, rows = shape
    cam, T, depth, rgb, key, vox = cc.contention_frame(cols, rows)
    vol = TSDFVolume(cols, rows, cam, max_units=16)
    vol.IntegrateFrames(depth[None], T[None])
    vol.enable_color()
    n = cols * rows
    st = vol.ColorFrames(np.stack([depth] * 3), np.stack([rgb] * 3), np.stack([T] * 3))
    assert st == (3 * n, 0, 0)
    got = read_all(vol)
    assert got[key][vox].tolist() == [255 * 3 * n, 255 * 3 * n, 255 * 3 * n, 3 * n]
    assert sum(int(u.astype(np.uint64).sum()) for u in got.values()) == (3 * 255 + 1) * 3 * n          # and nothing anywhere else
    vol.close()


# ---- independence ------------------------------------------------------------------------------------------------------------------------

def test_one_call_equals_one_call_per_frame_equals_the_reversed_order_equals_a_second_run(gpu, room):
    sc, keys, want, wst = room
    runs = []
    for mode in ("one call", "per frame", "reversed", "one call again"):
        vol = volume(sc)
        if mode == "per frame":
            st = np.sum([vol.ColorFrames(sc["depth"][f:f + 1], sc["rgb"][f:f + 1], sc["poses"][f:f + 1]) for f in range(4)], axis=0)
        elif mode == "reversed":
            st = vol.ColorFrames(sc["depth"][::-1], sc["rgb"][::-1], sc["poses"][::-1])
        else:
            st = vol.ColorFrames(sc["depth"], sc["rgb"], sc["poses"])
        assert tuple(int(x) for x in st) == wst, mode
        got = read_all(vol)
        assert_same(got, want, mode)
        runs.append(b"".join(got[k].tobytes() for k in sorted(got)))
        vol.close()
    assert all(r == runs[0] for r in runs)


def test_host_and_device_inputs_no_frames_and_two_calls_accumulate(gpu, room):
    import torch
    sc, keys, want, wst = room
    vol = volume(sc)
    assert vol.ColorFrames(sc["depth"][:0], sc["rgb"][:0], sc["poses"][:0]) == (0, 0, 0)
    assert not any(u.any() for u in read_all(vol).values())
    d = torch.from_numpy(sc["depth"].view(np.int16)).cuda()
    c = torch.from_numpy(sc["rgb"]).cuda()
    torch.cuda.synchronize()
    assert vol.ColorFrames(None, None, sc["poses"], device_ptrs=(d.data_ptr(), c.data_ptr())) == wst
    assert_same(read_all(vol), want, "device inputs")
    assert vol.ColorFrames(sc["depth"], sc["rgb"], sc["poses"]) == wst                # a second call adds to the first
    assert_same(read_all(vol), {k: 2 * u for k, u in want.items()}, "two calls")
    vol.close()


def test_stats_count_pixels_without_a_unit_and_pixels_off_the_lattice(gpu, room):
    sc, keys, want, wst = room
    vol = volume(sc, frames=slice(0, 2))                                              # the wall views were never integrated
    some = [int(k) for k in vol.unit_keys()]
    st = vol.ColorFrames(sc["depth"], sc["rgb"], sc["poses"])
    w2, wst2 = expected(sc, some)
    assert st == wst2 and st[1] > 100 and st[2] == 0, (st, wst2)
    assert_same(read_all(vol), w2, "no_unit")
    far = sc["poses"].copy()
    far[:, 0, 3] += 100.0                                                             # 100 m out: past the lattice's 96 m
    st = vol.ColorFrames(sc["depth"], sc["rgb"], far)
    assert st == (0, 0, wst[0] + wst[1]) and st[2] > 1000
    assert_same(read_all(vol), w2, "out_of_range")                                    # ... and nothing was added
    vol.close()


# ---- the warped colour image -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(64, 48), (37, 29)], ids=["64x48", "37x29"])
def test_the_warped_colour_image_and_the_warped_splat(gpu, tmp_path, shape):
    from elasticreconstruction_amd.tsdf import TSDFVolume
    cols, rows = shape
    sc = cc.warp_case(cols, rows)
    w = sc["warp"]
    chk = cr.build_color_check(ROOT)
    vol = TSDFVolume(cols, rows, sc["cam"], max_units=64)
    vol.IntegrateFrames(sc["depth"], sc["traj"], w)
    vol.enable_color()
    keys = [int(k) for k in vol.unit_keys()]
    Zs, Cs = [], []
    for f in range(len(sc["traj"])):
        ctr = w["ctr"][w["grid_index"][f]]
        args = (ctr, w["resolution"], w["length"], w["seg"][f], w["madj"][f])
        Z, Cw = vol.ReprojectColor(sc["depth"][f], sc["rgb"][f], *args)
        assert np.array_equal(Z, vol.Reproject(sc["depth"][f], *args))               # the depth is er_tsdf_reproject's
        cell, dd = cr.reproject_cells(chk, tmp_path, sc["depth"][f], sc["cam"], cols, rows, *args)
        wZ, wC, win = cr.warp_images(cell, dd, sc["rgb"][f])
        assert np.array_equal(Z, wZ) and np.array_equal(Cw, wC), "frame %d" % f
        assert (Z != 0).sum() > 0.4 * cols * rows
        Zs.append(Z)
        Cs.append(Cw)
    want = cr.empty_units(keys)
    wst = cr.splat_frames(want, Zs, Cs, sc["traj"], sc["cam"], cols, rows)
    st = vol.ColorFrames(sc["depth"], sc["rgb"], sc["traj"], warp=w)
    assert st == wst and st[0] > 0.4 * cols * rows * len(Zs), (st, wst)
    assert_same(read_all(vol), want, "warped splat")
    rigid = TSDFVolume(cols, rows, sc["cam"], max_units=64)                           # ... which is the rigid splat of the hook's output
    rigid.IntegrateFrames(sc["depth"], sc["traj"], w)
    rigid.enable_color()
    assert rigid.ColorFrames(np.stack(Zs), np.stack(Cs), sc["traj"]) == st
    assert_same(read_all(rigid), want, "splat of the hook's output")
    rigid.close()
    vol.close()


# ---- the sampler on crafted accumulators --------------------------------------------------------------------------------------------------

def local(i, j, k):
    return (i * 64 + j) * 64 + k


def test_the_sampler_on_crafted_accumulators(gpu):
    from elasticreconstruction_amd.tsdf import TSDFVolume
    vol = TSDFVolume(64, 48, cc.small_cam(64, 48), max_units=8)
    ks = [KEY0, KEY0 + 1, KEY0 + 512, KEY0 + (1 << 18)]                               # the origin's unit and its +z, +y, +x neighbours
    world = np.array([[0, 0, 0, 0.5], [0, 0, 64, 0.5], [0, 64, 0, 0.5], [64, 0, 0, 0.5]], np.float32)
    assert vol.LoadWorld(world) == 4 and [int(k) for k in vol.unit_keys()] == sorted(ks)
    vol.enable_color()
    units = cr.empty_units(ks)
    units[KEY0][local(5, 5, 5)] = [1, 3, 5, 2]                                       # level 0, exact halves
    units[KEY0][local(9, 9, 9)] = [3 * 255, 0, 299, 3]
    units[KEY0][local(9, 9, 10)] = [7, 7, 7, 1]                                      # (a neighbour with samples does not count at level 0)
    units[KEY0 + 1][local(20, 20, 0)] = [20, 21, 23, 1]                              # the only sample near (20, 20, 63): across the z border
    units[KEY0 + 512][local(30, 0, 30)] = [40, 50, 60, 2]                            # ... near (30, 63, 30): across the y border
    units[KEY0 + (1 << 18)][local(0, 40, 40)] = [200, 100, 1, 4]                     # ... near (63, 40, 40): across the x border
    units[KEY0][local(0, 10, 10)] = [9, 9, 9, 1]                                     # next to the unit at -x, which does not exist
    units[KEY0][local(1 << 4, 1 << 4, 1 << 4)] = [2 ** 31, 2 ** 31 + 6, 12, 2 ** 24]  # sums past 32 bits in 2 s + n
    for k in ks:
        vol.write_unit_color(k, units[k])
        assert np.array_equal(vol.read_unit_color(k), units[k])
    pts = np.array([[5, 5, 5], [9, 9, 9], [20, 20, 63], [30, 63, 30], [63, 40, 40], [-1, 10, 10], [0, 10, 11], [40, 40, 40], [-2, 10, 10],
                    [16, 16, 16], [16, 16, 17], [2.5, 3.5, 0], [20, 20, 64]], np.float64) * UL
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, -np.inf, 0], [0, 0, 97.0], [0, -96.5, 0], [3.0e38, 0, 0]], np.float64)
    p = np.concatenate([pts, bad]).astype(np.float32)
    rgba, counts = vol.sample_colors(p, counts=True)
    want, level = cr.sample(units, p)
    assert np.array_equal(rgba, want), (rgba.tolist(), want.tolist())
    assert counts == (int((level == 0).sum()), int((level == 1).sum()))
    assert level.tolist() == [0, 0, 1, 1, 1, 1, 1, -1, -1, 0, 1, -1, 0] + [-1] * 6
    assert rgba[:7].tolist() == [[1, 2, 3, 255], [255, 0, 100, 255], [20, 21, 23, 255], [20, 25, 30, 255], [50, 25, 0, 255], [9, 9, 9, 255],
                                 [9, 9, 9, 255]]
    assert rgba[9].tolist() == [128, 128, 0, 255] and not rgba[13:].any()
    assert np.array_equal(vol.sample_colors(p[:, :3].copy()), rgba)                   # [n, 3] points; a fourth column is ignored
    q = np.concatenate([p[:, :3], np.full((len(p), 1), np.nan, np.float32)], axis=1)
    assert np.array_equal(vol.sample_colors(q), rgba)
    assert vol.sample_colors(np.zeros((0, 4), np.float32), counts=True)[1] == (0, 0)
    vol.close()


def test_the_coloured_mesh_is_the_sampler_on_its_vertices_is_the_restatement(gpu, room):
    sc, keys, want, wst = room
    vol = volume(sc)
    vol.ColorFrames(sc["depth"], sc["rgb"], sc["poses"])
    verts, nrm, tris, rgba = vol.extract_indexed_mesh(colors=True)
    v2, n2, t2 = vol.extract_indexed_mesh()
    assert np.array_equal(verts.view(np.uint32), v2.view(np.uint32)) and np.array_equal(tris, t2) and len(verts) > 5000
    got, counts = vol.sample_colors(verts, counts=True)
    assert rgba.dtype == np.uint8 and rgba.shape == (len(verts), 4) and np.array_equal(rgba, got)
    wrgba, level = cr.sample(want, verts)
    assert np.array_equal(rgba, wrgba)
    assert counts == (int((level == 0).sum()), int((level == 1).sum())) and counts[0] > 500 and counts[1] > 500
    print("%d vertices: %d at level 0, %d at level 1, %d uncoloured" % (len(verts), counts[0], counts[1], len(verts) - sum(counts)))
    vol.close()


def test_save_mesh_writes_colours_iff_colour_is_enabled(gpu, room, tmp_path):
    from elasticreconstruction_amd import formats
    sc, keys, want, wst = room
    vol = volume(sc, color=False)
    a, b, c = (str(tmp_path / n) for n in ("plain.ply", "colour.ply", "suppressed.ply"))
    vol.SaveMesh(a)
    assert formats.load_ply_colors(a)[3] is None
    vol.enable_color()
    vol.ColorFrames(sc["depth"], sc["rgb"], sc["poses"])
    nv, nt = vol.SaveMesh(b)
    v, t, n, col = formats.load_ply_colors(b)
    assert col.shape == (nv, 4) and np.array_equal(col, vol.extract_indexed_mesh(colors=True)[3]) and (col[:, 3] == 255).mean() > 0.9
    vol.SaveMesh(c, colors=False)
    assert open(c, "rb").read() == open(a, "rb").read()
    vol.close()


# ---- lifecycle, refusals, non-interference --------------------------------------------------------------------------------------------------

def test_reset_and_drop_zero_the_accumulators_and_enable_is_idempotent(gpu, room):
    sc, keys, want, wst = room
    vol = volume(sc)
    vol.enable_color()                                                                # twice
    vol.ColorFrames(sc["depth"], sc["rgb"], sc["poses"])
    assert_same(read_all(vol), want)
    vol.enable_color()                                                                # ... and a third time: nothing is lost
    assert_same(read_all(vol), want)
    full = [k for k in keys if want[k][:, 3].any()]
    vol.drop_units(np.array(full[:2], np.int32))
    with pytest.raises(_ffi.ErError, match="handed to its owner"):
        vol.read_unit_color(full[0])
    vol.IntegrateFrames(sc["depth"][:1], sc["poses"][:1])                             # brings the dropped units back
    got = read_all(vol)
    assert not got[full[0]].any() and not got[full[1]].any()
    assert_same({k: u for k, u in got.items() if k not in full[:2]}, {k: u for k, u in want.items() if k not in full[:2]}, "after drop")
    vol.reset()
    assert vol.unit_count() == 0
    vol.IntegrateFrames(sc["depth"], sc["poses"])
    got = read_all(vol)
    assert sorted(got) == sorted(keys) and not any(u.any() for u in got.values())
    assert vol.ColorFrames(sc["depth"], sc["rgb"], sc["poses"]) == wst                # ... and colour goes on working
    assert_same(read_all(vol), want, "after reset")
    vol.close()


def test_refusals(gpu, room):
    from elasticreconstruction_amd.tsdf import TSDFVolume
    sc, keys, want, wst = room
    L = _ffi.lib()
    vol = volume(sc, color=False)
    T = np.ascontiguousarray(sc["poses"], np.float64)
    pts = np.zeros((1, 4), np.float32)
    for call, name in ((lambda: vol.ColorFrames(sc["depth"], sc["rgb"], sc["poses"]), "er_tsdf_color_frames"),
                       (lambda: vol.read_unit_color(keys[0]), "er_tsdf_read_unit_color"),
                       (lambda: vol.write_unit_color(keys[0], want[keys[0]]), "er_tsdf_write_unit_color"),
                       (lambda: vol.sample_colors(pts), "er_tsdf_sample_colors")):
        with pytest.raises(_ffi.ErError, match=name + ".*not enabled"):               # colour calls before enable
            call()
    vol.enable_color()
    missing = KEY0 + 5 * (1 << 18)
    assert missing not in keys
    with pytest.raises(_ffi.ErError, match="no unit with key"):
        vol.read_unit_color(missing)
    with pytest.raises(_ffi.ErError, match="no unit with key"):
        vol.write_unit_color(missing, want[keys[0]])
    st = (C.c_long * 3)(0, 0, 0)
    d = np.ascontiguousarray(sc["depth"])
    assert L.er_tsdf_color_frames(vol._h, 4, _ffi.ptr(d), None, 0, _ffi.ptr(T), None, st) != 0      # a NULL rgb
    assert "NULL" in L.er_last_error().decode()
    assert L.er_tsdf_color_frames(vol._h, -1, _ffi.ptr(d), _ffi.ptr(sc["rgb"]), 0, _ffi.ptr(T), None, st) != 0
    assert not any(u.any() for u in read_all(vol).values())
    vol.close()
    shard = TSDFVolume(64, 48, sc["cam"], max_units=64)
    shard.set_unit_shard(0, 2)
    with pytest.raises(_ffi.ErError, match="across GPUs"):
        shard.enable_color()
    shard.close()
    late = TSDFVolume(64, 48, sc["cam"], max_units=64)
    late.enable_color()
    late.set_unit_shard(1, 2)                                                         # shard mode after enable: every colour call is refused
    for call in (lambda: late.ColorFrames(sc["depth"], sc["rgb"], sc["poses"]), lambda: late.sample_colors(pts),
                 lambda: late.read_unit_color(keys[0])):
        with pytest.raises(_ffi.ErError, match="across GPUs"):
            call()
    late.close()


def test_colour_does_not_touch_the_volume(gpu, room):
    sc, keys, want, wst = room
    plain = volume(sc, color=False)
    col = volume(sc)
    col.ColorFrames(sc["depth"], sc["rgb"], sc["poses"])
    col.sample_colors(np.zeros((10, 4), np.float32))
    assert assert_volumes_identical(col, plain, "colour enabled and splatted") == len(keys)
    assert np.array_equal(col.extract_indexed_mesh()[0].view(np.uint32), plain.extract_indexed_mesh()[0].view(np.uint32))
    col.IntegrateFrames(sc["depth"][:2], sc["poses"][:2])                             # and the volume goes on integrating as before
    plain.IntegrateFrames(sc["depth"][:2], sc["poses"][:2])
    assert_volumes_identical(col, plain, "integrating on")
    plain.close()
    col.close()
