"""Colour, the part that needs no GPU: the numpy restatement (tests/color_restatement.py) on hand-made answers, the conditions
the fixtures are there for, the restatement's colours against the texture the frames were rendered from (ground truth), the coloured PLY of
formats.py and csrc/host/er_formats.h, and the new symbols."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import color_cases as cc
import color_restatement as cr
from elasticreconstruction_amd import _ffi, formats, synth
from mesh_restatement import indexed_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UL = cr.UL
KEY0 = cc.KEY0
ONE_PX = np.array([100.0, 100.0, 0.0, 0.0, 2.5, 2.5], np.float32)        # a 1 x 1 image whose only pixel looks along the optical axis


def pose(x, y, z):
    T = np.eye(4)
    T[:3, 3] = [x, y, z]
    return T


def one_pixel(T, d=1000, rgb=(10, 20, 30), keys=None, cam=ONE_PX):
    """The pixel of a 1 x 1 image at depth d millimetres: its world point is exactly T's translation plus (0, 0, d / 1000)."""
    units = cr.empty_units(keys if keys is not None else [KEY0])
    st = cr.splat(units, np.array([d], np.uint16), np.array([rgb], np.uint8), T, cam, 1, 1)
    return units, st


def local(i, j, k):
    return (i * 64 + j) * 64 + k


# ---- the restatement on hand-made answers ----------------------------------------------------------------------------------------------

def test_one_pixel_at_a_known_pose_lands_in_a_known_voxel():
    units, st = one_pixel(pose(10 * UL, 20 * UL, 30 * UL - 1.0 + 0.001))            # z: 30 ul + 1 mm
    assert st == (1, 0, 0)
    u = units[KEY0]
    assert u[local(10, 20, 30)].tolist() == [10, 20, 30, 1] and int(u.sum()) == 61
    cr.splat(units, np.array([1000], np.uint16), np.array([[255, 0, 1]], np.uint8), pose(10 * UL, 20 * UL, 30 * UL - 1.0), ONE_PX, 1, 1)
    assert u[local(10, 20, 30)].tolist() == [265, 20, 31, 2]


def test_points_with_negative_coordinates_and_local_indices_0_and_63_across_a_unit_border():
    below = KEY0 - (1 << 18) - (1 << 9) - 1                                         # the unit that ends at the origin on every axis
    keys = [KEY0, below, KEY0 - (1 << 18)]
    units, st = one_pixel(pose(-1 * UL, -1 * UL, -1 * UL - 1.0), keys=keys)
    assert st == (1, 0, 0) and units[below][local(63, 63, 63)].tolist() == [10, 20, 30, 1] and int(units[KEY0].sum()) == 0
    units, st = one_pixel(pose(0.0, 0.0, -1.0), keys=keys)
    assert st == (1, 0, 0) and units[KEY0][local(0, 0, 0)].tolist() == [10, 20, 30, 1] and int(units[below].sum()) == 0
    units, st = one_pixel(pose(-1 * UL, 0.0, 63 * UL - 1.0), keys=keys)            # index 63 of one unit in x, 0 and 63 of its neighbour in y, z
    assert st == (1, 0, 0) and units[KEY0 - (1 << 18)][local(63, 0, 63)].tolist() == [10, 20, 30, 1]
    units, st = one_pixel(pose(-40.4 * UL, -100.2 * UL, -1.0 - 7.6 * UL), keys=[KEY0 - (1 << 18) - (2 << 9) - 1])
    assert st == (1, 0, 0) and units[KEY0 - (1 << 18) - (2 << 9) - 1][local(64 - 40, 128 - 100, 64 - 8)].tolist() == [10, 20, 30, 1]


def test_a_point_half_way_between_voxels_goes_up_in_the_splat_and_to_the_even_voxel_in_the_sampler():
    # 2.5 ul and 3.5 ul are exact binary fractions (15 / 1024, 21 / 1024), and the x, y of the only pixel's world point are T's translation
    units, st = one_pixel(pose(2.5 * UL, 3.5 * UL, -1.0))
    assert st == (1, 0, 0) and units[KEY0][local(3, 4, 0), 3] == 1                 # floor(x + 0.5): both halves go up
    units, st = one_pixel(pose(-2.5 * UL, -3.5 * UL, -1.0), keys=[KEY0 - (1 << 18) - (1 << 9)])
    assert st == (1, 0, 0) and units[KEY0 - (1 << 18) - (1 << 9)][local(64 - 2, 64 - 3, 0), 3] == 1     # ... also below zero
    v = cr.nearest_voxel(np.array([[2.5 * UL, 3.5 * UL, -2.5 * UL], [0.5 * UL, 1.5 * UL, -0.5 * UL]], np.float32))
    assert v.tolist() == [[2.0, 4.0, -2.0], [0.0, 2.0, -0.0]]                       # rint: half to even
    units = cr.empty_units([KEY0])
    units[KEY0][local(2, 4, 0)] = [7, 8, 9, 1]
    units[KEY0][local(3, 4, 0)] = [200, 200, 200, 1]
    rgba, level = cr.sample(units, np.array([[2.5 * UL, 3.5 * UL, 0.0]], np.float32))
    assert rgba.tolist() == [[7, 8, 9, 255]] and level.tolist() == [0]


def test_pixels_that_contribute_nothing_zero_depth_beyond_the_truncation_no_unit_off_the_lattice():
    T = pose(10 * UL, 20 * UL, 30 * UL - 1.0)
    units, st = one_pixel(T, d=0)
    assert st == (0, 0, 0) and int(units[KEY0].sum()) == 0
    cam = ONE_PX.copy()
    cam[5] = 0.9995                                                                 # integration_trunc below the pixel's 1 m
    units, st = one_pixel(T, cam=cam)
    assert st == (0, 0, 0) and int(units[KEY0].sum()) == 0
    cam[5] = 1.0                                                                    # "res > trunc" is what drops a pixel: 1.0 stays
    assert one_pixel(T, cam=cam)[1] == (1, 0, 0)
    assert one_pixel(T, keys=[KEY0 + 5])[1] == (0, 1, 0)                            # the unit does not exist
    assert one_pixel(pose(100.0, 0.0, 0.0))[1] == (0, 0, 1)                         # 100 m out: past the lattice's 96 m
    assert one_pixel(pose(0.0, 16384 * UL, -1.0))[1] == (0, 0, 1)                   # the first index off the lattice ...
    assert one_pixel(pose(0.0, -16384 * UL, -1.0), keys=[256 << 18 | 0 << 9 | 256])[1] == (1, 0, 0)      # ... and the last one on it
    assert one_pixel(pose(np.nan, 0.0, 0.0))[1] == (0, 0, 1)


def test_channel_rounding_at_exact_halves_and_the_two_levels():
    units = cr.empty_units([KEY0, KEY0 + 1])
    units[KEY0][local(5, 5, 5)] = [1, 3, 5, 2]                                     # 0.5, 1.5, 2.5: half up
    units[KEY0][local(9, 9, 9)] = [3 * 255, 0, 299, 3]                             # 255, 0, 99.67
    units[KEY0][local(20, 20, 62)] = [10, 10, 10, 1]
    units[KEY0 + 1][local(20, 21, 0)] = [20, 21, 23, 1]                            # across the unit border in z
    pts = np.array([[5, 5, 5], [9, 9, 9], [20, 20, 63], [40, 40, 40], [5, 5, 6]], np.float64) * UL
    rgba, level = cr.sample(units, pts.astype(np.float32))
    assert rgba.tolist() == [[1, 2, 3, 255], [255, 0, 100, 255], [15, 16, 17, 255], [0, 0, 0, 0], [1, 2, 3, 255]]
    assert level.tolist() == [0, 0, 1, -1, 1]
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 97.0], [0, -96.5, 0]], np.float32)
    rgba, level = cr.sample(units, bad)
    assert not rgba.any() and (level == -1).all()


# ---- the fixtures' conditions ------------------------------------------------------------------------------------------------------------

def test_the_contention_fixture_puts_every_pixel_into_one_voxel():
    for cols, rows in ((64, 48), (37, 29)):
        cam, T, depth, rgb, key, vox = cc.contention_frame(cols, rows)
        units = cr.empty_units([key])
        assert cr.splat(units, depth, rgb, T, cam, cols, rows) == (cols * rows, 0, 0)
        assert units[key][vox].tolist() == [255 * cols * rows] * 3 + [cols * rows]
        assert int(units[key][:, 3].sum()) == cols * rows


def test_the_gpu_scenes_fit_their_pools_cross_unit_borders_and_reject_pixels():
    from oracle import pyoracle
    for make, neg in ((cc.room_with_sphere, False), (cc.negative_corner, True)):
        for cols, rows in ((64, 48), (37, 29)):
            sc = make(cols, rows)
            ora = pyoracle.OracleVolume(cols, rows, sc["cam"])
            for f in range(len(sc["poses"])):
                ora.Integrate(sc["depth"][f], sc["poses"][f])
            keys = [int(k) for k in ora.unit_keys()]
            assert 4 <= len(keys) <= 64
            units = cr.empty_units(keys)
            added, no_unit, oor = cr.splat_frames(units, sc["depth"], sc["rgb"], sc["poses"], sc["cam"], cols, rows)
            assert no_unit == 0 and oor == 0 and added > 0.4 * sc["depth"].size
            assert sum(1 for u in units.values() if u[:, 3].any()) >= 4          # the coloured surface spans several units
            if neg:
                assert all((k >> 18) < 256 and ((k >> 9) & 511) < 256 and (k & 511) < 256 for k in keys if units[k][:, 3].any())
            else:
                assert added < int((sc["depth"] != 0).sum())                      # pixels beyond integration_trunc


@pytest.mark.parametrize("shape", [(64, 48), (37, 29)], ids=["64x48", "37x29"])
def test_the_warp_fixture_has_equal_depth_contenders_and_occluded_pixels(tmp_path, color_check, shape):
    cols, rows = shape
    sc = cc.warp_case(cols, rows)
    w = sc["warp"]
    ties = occluded = 0
    for f in range(len(sc["traj"])):
        ctr = w["ctr"][w["grid_index"][f]]
        cell, dd = cr.reproject_cells(color_check, tmp_path, sc["depth"][f], sc["cam"], cols, rows, ctr, w["resolution"], w["length"], w["seg"][f], w["madj"][f])
        Z, C, win = cr.warp_images(cell, dd, sc["rgb"][f])
        # (Z is not compared with the oracle's Reproject here: like the reference it clips to the literal 640 x 480 and writes past a smaller
        #  image; the GPU tests compare er_tsdf_reproject_color's depth with er_tsdf_reproject's)
        on = cell >= 0
        assert on.sum() > 0.5 * cols * rows and (Z != 0).sum() > 0.4 * cols * rows
        contenders = np.bincount(cell[on & (dd == Z[np.maximum(cell, 0)])], minlength=cols * rows)
        ties += int((contenders >= 2).sum())
        occluded += int((on & (dd > Z[np.maximum(cell, 0)])).sum())
        assert ((win >= 0) == (Z != 0)).all() and not C[Z == 0].any()
    print("%d x %d: %d cells with two or more equal-depth contenders, %d occluded source pixels" % (cols, rows, ties, occluded))
    assert ties >= 1 and occluded >= 1


# ---- ground truth ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def coloured_room():
    """The textured room with the sphere: volume from the CPU oracle, vertices from the mesh restatement, colours from the colour restatement."""
    from oracle import pyoracle
    sc = cc.ground_truth_scene()
    ora = pyoracle.OracleVolume(sc["cols"], sc["rows"], sc["cam"])
    for f in range(len(sc["poses"])):
        ora.Integrate(sc["depth"][f], sc["poses"][f])
    keys = [int(k) for k in ora.unit_keys()]
    verts, tris, _ = indexed_mesh({k: ora.read_unit(k) for k in keys})
    units = cr.empty_units(keys)
    st = cr.splat_frames(units, sc["depth"], sc["rgb"], sc["poses"], sc["cam"], sc["cols"], sc["rows"])
    rgba, level = cr.sample(units, verts)
    return sc, verts, tris, rgba, level, st


def test_render_rgbd_gives_render_depths_image_and_the_texture_at_the_hit_point():
    sc = cc.room_with_sphere(37, 29)
    d = synth.to_numpy_u16(synth.render_depth(sc["poses"], 37, 29, tuple(float(x) for x in sc["cam"][:4])))
    assert np.array_equal(d, sc["depth"]) and (d != 0).all()
    assert sc["rgb"].dtype == np.uint8 and sc["rgb"].shape == (4, 37 * 29, 3)
    assert sc["rgb"].min() >= 30 and sc["rgb"].max() <= 228 and len(np.unique(sc["rgb"])) > 100
    # the texture is Lipschitz with TEXTURE_G: random pairs
    rng = np.random.default_rng(3)
    a = rng.uniform(-2, 5, (20000, 3))
    b = a + rng.normal(size=(20000, 3)) * 0.01
    slope = np.abs(synth.texture(a) - synth.texture(b)).max(axis=1) / np.linalg.norm(a - b, axis=1)
    assert slope.max() <= synth.TEXTURE_G and slope.max() > 0.8 * synth.TEXTURE_G


def test_every_coloured_vertex_carries_the_texture_of_its_own_position(coloured_room):
    """|colour - texture(vertex)| <= G r + 1 levels, r = sqrt(3) voxels + 1 mm at level 0 (the vertex and every sample of its nearest voxel lie in
    that voxel's cell; a sample's point is off its true hit point by the millimetre rounding of the depth) and 2 sqrt(3) voxels + 1 mm at
    level 1 (a sample may lie in a neighbouring cell); + 1 for the rounding of the rendered byte and of the mean."""
    sc, verts, tris, rgba, level, st = coloured_room
    assert len(verts) > 50000 and st[1] == 0 and st[2] == 0
    tex = synth.texture(verts[:, :3].astype(np.float64))
    err = np.abs(rgba[:, :3].astype(np.float64) - tex).max(axis=1)
    for lv, r in ((0, math.sqrt(3) * UL + 0.001), (1, 2 * math.sqrt(3) * UL + 0.001)):
        m = level == lv
        bound = synth.TEXTURE_G * r + 1
        print("level %d: %d vertices, max error %.2f levels, bound %.2f" % (lv, m.sum(), err[m].max(), bound))
        assert m.sum() > 10000 and err[m].max() <= bound
    assert (rgba[level >= 0, 3] == 255).all() and not rgba[level < 0].any()


def test_at_most_two_percent_of_the_vertices_stay_uncoloured(coloured_room):
    sc, verts, tris, rgba, level, st = coloured_room
    share = float((level < 0).mean())
    print("uncoloured: %.3f %% of %d vertices; level 0: %.1f %%" % (100 * share, len(verts), 100 * float((level == 0).mean())))
    assert share <= 0.02


# ---- PLY with colours --------------------------------------------------------------------------------------------------------------------

def small_mesh():
    rng = np.random.default_rng(7)
    verts = np.concatenate([rng.normal(size=(9, 3)), rng.integers(0, 3, (9, 1))], 1).astype(np.float32)
    nrm = rng.normal(size=(9, 3)).astype(np.float32)
    nrm[2] = np.nan
    tris = rng.integers(0, 9, (5, 3)).astype(np.int32)
    col = rng.integers(0, 256, (9, 4)).astype(np.uint8)
    col[0], col[1] = [0, 0, 0, 0], [255, 255, 255, 255]
    return verts, nrm, tris, col


def ply_header(n, m, normals, binary):
    lines = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "element vertex %d" % n,
             "property float x", "property float y", "property float z"]
    if normals:
        lines += ["property float nx", "property float ny", "property float nz"]
    lines += ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
    lines += ["element face %d" % m, "property list uchar int vertex_indices", "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


@pytest.fixture(scope="module")
def color_check():
    return cr.build_color_check(ROOT)


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "ascii"])
@pytest.mark.parametrize("with_normals", [True, False], ids=["normals", "no normals"])
def test_coloured_ply_header_round_trip_and_the_host_writers_bytes(tmp_path, color_check, binary, with_normals):
    verts, nrm, tris, col = small_mesh()
    path = str(tmp_path / "m.ply")
    formats.save_ply(path, verts, tris, nrm if with_normals else None, binary=binary, colors=col)
    raw = open(path, "rb").read()
    hdr = ply_header(9, 5, with_normals, binary)
    assert raw[:len(hdr)] == hdr, raw[:len(hdr) + 20]
    if binary:
        assert len(raw) == len(hdr) + 9 * (4 * (6 if with_normals else 3) + 4) + 5 * 13
        assert raw[len(hdr) + 4 * (6 if with_normals else 3):][:4] == bytes(col[0])       # packed: the bytes follow the row's floats
    else:
        assert raw[len(hdr):].split(b"\n")[1].split()[-4:] == [b"255"] * 4                # integers
    v, t, n, c = formats.load_ply_colors(path)
    assert np.array_equal(v.view(np.uint32), verts[:, :3].view(np.uint32)) and np.array_equal(t, tris)
    assert c.dtype == np.uint8 and np.array_equal(c, col)
    assert (n is None) == (not with_normals)
    three = formats.load_ply(path)                                                        # the 3-tuple, unchanged, on a coloured file
    assert len(three) == 3 and np.array_equal(three[0], v) and np.array_equal(three[1], t)
    if with_normals:
        assert np.array_equal(three[2], n) and not np.isnan(n).any()
    # the same arrays through er_formats.h
    arrays = str(tmp_path / "arrays.bin")
    with open(arrays, "wb") as f:
        f.write(np.array([9, 5], np.int64).tobytes())
        f.write(verts.tobytes())
        f.write(np.concatenate([nrm, np.zeros((9, 1), np.float32)], 1).tobytes())
        f.write(tris.tobytes())
        f.write(col.tobytes())
    other = str(tmp_path / "host.ply")
    subprocess.run([color_check, "ply", arrays, other, "1" if binary else "0", "1" if with_normals else "0"], check=True, timeout=60)
    assert open(other, "rb").read() == raw


def test_a_file_without_colours_is_what_it_was_and_loads_with_none(tmp_path):
    verts, nrm, tris, col = small_mesh()
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    formats.save_ply(a, verts, tris, nrm)
    formats.save_ply(b, verts, tris, nrm, True, None)
    assert open(a, "rb").read() == open(b, "rb").read() and b"red" not in open(a, "rb").read()
    assert formats.load_ply_colors(a)[3] is None
    with pytest.raises(ValueError):
        formats.save_ply(a, verts, tris, nrm, colors=col[:5])


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------

COLOR_SYMBOLS = ("er_tsdf_color_enable", "er_tsdf_read_unit_color", "er_tsdf_write_unit_color", "er_tsdf_color_frames", "er_tsdf_sample_colors",
                 "er_tsdf_reproject_color")


def test_the_colour_entry_points_are_declared_bound_exported_and_refuse_a_null_handle():
    header = open(os.path.join(ROOT, "include", "er_hip.h")).read()
    L = _ffi.lib()
    for name in COLOR_SYMBOLS:
        assert "int %s(" % name in header and name in _ffi.SYMBOLS and hasattr(L, name), name
    buf = np.zeros(16, np.uint32)
    calls = {"er_tsdf_color_enable": lambda: L.er_tsdf_color_enable(None),
             "er_tsdf_read_unit_color": lambda: L.er_tsdf_read_unit_color(None, KEY0, _ffi.ptr(buf)),
             "er_tsdf_write_unit_color": lambda: L.er_tsdf_write_unit_color(None, KEY0, _ffi.ptr(buf)),
             "er_tsdf_color_frames": lambda: L.er_tsdf_color_frames(None, 0, None, None, 0, None, None, None),
             "er_tsdf_sample_colors": lambda: L.er_tsdf_sample_colors(None, None, 0, None, None),
             "er_tsdf_reproject_color": lambda: L.er_tsdf_reproject_color(None, None, None, None, 8, C.c_float(3.0), None, None)}
    for name in COLOR_SYMBOLS:
        assert calls[name]() != 0 and name in L.er_last_error().decode(), name


def test_no_colour_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from elasticreconstruction_amd.tsdf import TSDFVolume
    with pytest.raises(_ffi.ErError):
        TSDFVolume(64, 48, cc.small_cam(64, 48), max_units=4).enable_color()


# ---- load_png_rgb8 against Pillow --------------------------------------------------------------------------------------------------------

def png_bytes(img, ctype, depth=8, interlace=0, filters=None):
    """A PNG of img uint8[h, w, channels] written here: filter type filters[y] (default y % 5: all five occur) on row y, one IDAT chunk."""
    import struct
    import zlib
    h, w, ch = img.shape
    raw = bytearray()
    prev = np.zeros(w * ch, np.int64)
    for y in range(h):
        cur = img[y].reshape(-1).astype(np.int64)
        ft = (y % 5) if filters is None else filters[y]
        a = np.concatenate([np.zeros(ch, np.int64), cur[:-ch]])
        c = np.concatenate([np.zeros(ch, np.int64), prev[:-ch]])
        if ft == 0:
            pred = np.zeros_like(cur)
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = prev
        elif ft == 3:
            pred = (a + prev) // 2
        else:
            p = a + prev - c
            pa, pb, pc = np.abs(p - a), np.abs(p - prev), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
        raw += bytes([ft]) + ((cur - pred) % 256).astype(np.uint8).tobytes()
        prev = cur

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h // (depth // 8) if depth == 16 else h, depth, ctype, 0, 0, interlace))
            + chunk(b"IDAT", zlib.compress(bytes(raw))) + chunk(b"IEND", b""))


def filters_of(path, bpp):
    """The filter types that occur in a non-interlaced 8-bit PNG file."""
    import struct
    import zlib
    raw = open(path, "rb").read()
    pos, idat, w = 8, b"", 0
    while pos < len(raw):
        n, kind = struct.unpack(">I4s", raw[pos:pos + 8])
        if kind == b"IHDR":
            w = struct.unpack(">I", raw[pos + 8:pos + 12])[0]
        if kind == b"IDAT":
            idat += raw[pos + 8:pos + 8 + n]
        pos += 12 + n
    return set(zlib.decompress(idat)[::w * bpp + 1])


def sample_images(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    noise = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    hramp = np.stack([(x * 3) % 256, (x * 5 + 7) % 256, (255 - x) % 256], -1).astype(np.uint8)
    vramp = np.stack([(y * 3) % 256, (y * 7 + 1) % 256, (255 - 2 * y) % 256], -1).astype(np.uint8)
    smooth = np.stack([127 + 120 * np.sin(x / 9.0 + y / 7.0), 127 + 120 * np.cos(x / 5.0) * np.sin(y / 11.0), (x * y) % 256], -1).astype(np.uint8)
    return dict(noise=noise, hramp=hramp, vramp=vramp, smooth=smooth)


def host_png(color_check, path, out):
    r = subprocess.run([color_check, "png", path, out], timeout=60)
    if r.returncode != 0:
        assert not os.path.exists(out)
        return None
    a = np.fromfile(out, np.uint8)
    w, h = np.frombuffer(a[:8].tobytes(), np.int32)
    return a[8:].reshape(h, w, 3)


@pytest.mark.parametrize("shape", [(64, 48), (37, 29), (1, 1), (3, 101)], ids=lambda s: "%dx%d" % s)
def test_load_png_rgb8_against_pillow(tmp_path, color_check, shape):
    from PIL import Image
    w, h = shape
    seen = set()
    for name, img in sample_images(w, h).items():
        p = str(tmp_path / (name + ".png"))
        Image.fromarray(img, "RGB").save(p)                                          # Pillow's own choice of filters
        seen |= filters_of(p, 3)
        assert np.array_equal(host_png(color_check, p, str(tmp_path / "o.bin")), img), name
        p5 = str(tmp_path / (name + "_5.png"))                                       # every filter type, row y with type y % 5
        open(p5, "wb").write(png_bytes(img, 2))
        assert np.array_equal(np.asarray(Image.open(p5).convert("RGB")), img)        # (Pillow reads the hand-written file as meant)
        assert np.array_equal(host_png(color_check, p5, str(tmp_path / "o5.bin")), img), name
        rgba = np.concatenate([img, (img[..., :1] // 2 + 3).astype(np.uint8)], -1)
        pa, pa5 = str(tmp_path / (name + "_a.png")), str(tmp_path / (name + "_a5.png"))
        Image.fromarray(rgba, "RGBA").save(pa)
        open(pa5, "wb").write(png_bytes(rgba, 6))
        assert np.array_equal(host_png(color_check, pa, str(tmp_path / "oa.bin")), img), name      # RGBA: the alpha is dropped
        assert np.array_equal(host_png(color_check, pa5, str(tmp_path / "oa5.bin")), img), name
    print("%d x %d: Pillow used the filter types %s" % (w, h, sorted(seen)))
    if h >= 5:
        assert filters_of(str(tmp_path / "noise_5.png"), 3) == {0, 1, 2, 3, 4}


def test_load_png_rgb8_refuses_what_it_does_not_read(tmp_path, color_check):
    from PIL import Image
    img = sample_images(37, 29)["smooth"]
    out = str(tmp_path / "o.bin")
    files = {}
    Image.fromarray(img[..., 0], "L").save(str(tmp_path / "grey.png"))
    Image.fromarray(img[..., 0].astype(np.uint16) * 257).save(str(tmp_path / "grey16.png"))
    Image.fromarray(img, "RGB").quantize(16).save(str(tmp_path / "palette.png"))
    good = png_bytes(img, 2)
    files["rgb16.png"] = png_bytes(img.reshape(29, 37, 3), 2, depth=16)               # bit depth 16 in the header
    files["interlaced.png"] = png_bytes(img, 2, interlace=1)
    files["truncated.png"] = good[:len(good) // 2]
    files["no_iend.png"] = good[:-12]
    files["filter5.png"] = png_bytes(img, 2, filters=[5] * 29)
    files["short_data.png"] = png_bytes(img[:20], 2).replace(b"\x00\x00\x00\x14", b"\x00\x00\x00\x1d", 1)   # 29 rows declared, 20 present
    files["not_a_png.png"] = b"P6 37 29 255\n" + img.tobytes()
    files["empty.png"] = b""
    for name, data in files.items():
        open(str(tmp_path / name), "wb").write(data)
    open(str(tmp_path / "good.png"), "wb").write(good)
    assert np.array_equal(host_png(color_check, str(tmp_path / "good.png"), out), img)
    os.remove(out)
    for name in ["grey.png", "grey16.png", "palette.png"] + list(files) + ["missing.png"]:
        assert host_png(color_check, str(tmp_path / name), out) is None, name


# ---- bin/Integrate's refusals ------------------------------------------------------------------------------------------------------------

def test_integrate_refuses_colour_it_cannot_use(tmp_path):
    from PIL import Image
    d = str(tmp_path)
    exe = os.path.join(ROOT, "elasticreconstruction_amd", "bin", "Integrate")
    eye = np.eye(4)
    formats.save_log(os.path.join(d, "traj.log"), [formats.FramedTransformation(i, i, i + 1, eye) for i in range(3)])
    np.zeros((2, 480 * 640), np.uint16).tofile(os.path.join(d, "frames.raw"))
    np.zeros((2, 480 * 640, 3), np.uint8).tofile(os.path.join(d, "colour.raw"))
    np.zeros((3, 480 * 640, 3), np.uint8).tofile(os.path.join(d, "three.raw"))
    np.zeros((2, 320 * 240, 3), np.uint8).tofile(os.path.join(d, "qvga.raw"))
    Image.fromarray(np.zeros((240, 320, 3), np.uint8), "RGB").save(os.path.join(d, "small.png"))
    Image.fromarray(np.zeros((480, 640, 3), np.uint8), "RGB").save(os.path.join(d, "vga.png"))
    open(os.path.join(d, "small.txt"), "w").write("small.png\nsmall.png\n")
    open(os.path.join(d, "one.txt"), "w").write("vga.png\n")
    base = ["--ref_traj", "traj.log", "-oni", "frames.raw", "--save_to", "w.pcd"]
    cases = [(["--color_raw", "colour.raw"], ["--save_mesh"]),                                         # no --save_mesh
             (["--color_raw", "colour.raw", "--save_mesh", "m.ply", "--gpus", "2", "--same_device"], ["--gpus 2", "colour"]),
             (["--color_raw", "three.raw", "--save_mesh", "m.ply"], ["3 frames", "2"]),                # another frame count
             (["--color_raw", "qvga.raw", "--save_mesh", "m.ply"], ["640x480x3"]),                     # another image size
             (["--color_raw", "nowhere.raw", "--save_mesh", "m.ply"], ["nowhere.raw"]),
             (["--color_list", "small.txt", "--save_mesh", "m.ply"], ["small.png", "640x480"]),
             (["--color_list", "one.txt", "--save_mesh", "m.ply"], ["1 frames", "2"]),
             (["--color_raw", "colour.raw", "--color_list", "one.txt", "--save_mesh", "m.ply"], ["not both"])]
    for extra, words in cases:
        r = subprocess.run([exe] + base + extra, cwd=d, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and all(w in r.stderr for w in words), (extra, r.returncode, r.stderr)
        assert not os.path.exists(os.path.join(d, "w.pcd")) and not os.path.exists(os.path.join(d, "m.ply")), extra
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert "--color_raw" in r.stdout and "--color_list" in r.stdout
