"""er_mesh_simplify and er_tsdf_extract_mesh_simplified on the GPU against tests/mesh_simplify_restatement.py, bit for bit:
index lists at the block, wave and table-size edges of the kernels, the crafted meshes of tests/mesh_simplify_cases.py, the refusals, the
nullable outputs and capacities, and the simplified extraction of volumes -- the analytic sphere with planted voxels, the box room, a coloured
volume -- against the restatement applied to the unsimplified mesh of the same volume."""
import ctypes as C

import numpy as np
import pytest

import helpers
import mesh_simplify_cases as cases
import mesh_simplify_restatement as rs
from elasticreconstruction_amd import _ffi, mesh, synth
from elasticreconstruction_amd.tsdf import TSDFVolume
from test_mesh_components_gpu import planted_sphere_planes, volume_of
from test_mesh_indexed_gpu import sphere_planes
from test_mesh_simplify_cpu import bits, same

pytestmark = pytest.mark.gpu
UL = 3.0 / 512.0
SIZES = cases.sizes()
CRAFTED = cases.crafted()


def as_bytes(r):
    return b"".join(r[k].tobytes() for k in sorted(r) if isinstance(r[k], np.ndarray)) + repr(r["stats"]).encode()


def check(m, what):
    """mesh.simplify against the restatement, three times with the same bytes.  Returns the result."""
    want = rs.simplify(**m)
    got = mesh.simplify(probes=True, **m)
    probes = got.pop("probes")
    print("%s: %d vertices, %d triangles -> %d, %d; stats %s; longest probe sequences %s" % (what, len(m["verts"]), len(m["tris"]), len(got["verts"]),
                                                                                       len(got["tris"]), got["stats"], probes))
    same(got, want, what)
    assert got["verts"].dtype == np.float32 and got["tris"].dtype == np.int32 and got["cluster"].shape == (len(m["verts"]),)
    assert not got["verts"][:, 3].any()
    first = as_bytes(got)
    for _ in range(2):
        assert as_bytes(mesh.simplify(**m)) == first, what + ": another call gave other bytes"
    assert probes[0] <= 2 * max(len(m["verts"]), 1) and probes[1] <= 2 * max(len(m["tris"]), 1)
    return got


@pytest.mark.parametrize("name", list(SIZES))
def test_sizes_at_the_block_wave_and_table_edges(gpu, name):
    check(SIZES[name], name)


@pytest.mark.parametrize("name", list(CRAFTED))
def test_crafted_meshes_match_the_restatement(gpu, name):
    check(CRAFTED[name], name)


def test_two_million_vertices_in_one_far_cell(gpu):
    """|S_x| > 2^53: the sum has left the range in which every integer is a float64.  It still converts exactly -- next to 4096 m a float32 is a
    multiple of 2^-12 m, so every q and their sum is a multiple of 2^8, and float64 holds those up to 2^61, which takes 2^29 members.  A sum whose
    conversion rounds is therefore out of reach of any mesh that fits a device; the host check of er_mesh_simplify_math.h converts such sums."""
    m = cases.far_cell()
    got = check(m, "2^21 + 1 vertices in the last cell below x = 4096 m")
    S = rs.quantise(m["verts"][:-2, 0]).sum()
    assert abs(int(S)) > 2 ** 53 and int(S) % 256 == 0
    assert got["members"].tolist() == [2 ** 21 + 1, 1, 1] and rs.cells(m["verts"][:1, :3], m["cell"])[0, 0] == 2 ** 20 - 1


def test_absent_arrays_and_three_column_inputs(gpu):
    m = cases.random_mesh(4097, 9000, 31)
    for drop in (("normals",), ("colors",), ("normals", "colors")):
        check(dict(m, **{k: None for k in drop}), "without " + " and ".join(drop))
    a = mesh.simplify(m["verts"][:, :3], m["tris"], m["cell"], m["normals"][:, :3], m["colors"])
    same(a, rs.simplify(**m), "three columns")


def test_refusals_name_the_first_offender_and_write_nothing(gpu):
    L = _ffi.lib()
    m = cases.random_mesh(1000, 2000, 41)
    nv, nt = C.c_long(-7), C.c_long(-7)
    st = (C.c_long * 4)(-7, -7, -7, -7)
    p = lambda a: None if a is None else _ffi.ptr(a)

    def refused(verts, tris, cell, words):
        vo, to, cl = np.full((1000, 4), -7, np.float32), np.full((2000, 3), -7, np.int32), np.full(len(verts), -7, np.int32)
        nv.value = nt.value = -7
        rc = L.er_mesh_simplify(p(verts), None, None, len(verts), p(tris), len(tris), C.c_float(cell), 0, p(vo), None, None, None, 1000, p(to), None, 2000, p(cl),
                                C.byref(nv), C.byref(nt), st, None)
        msg = L.er_last_error().decode()
        assert rc != 0 and msg.startswith("er_mesh_simplify: " + words), msg
        assert (vo == -7).all() and (to == -7).all() and (cl == -7).all() and (nv.value, nt.value) == (-7, -7) and tuple(st) == (-7,) * 4
        with pytest.raises(ValueError, match=words.split(" (")[0].replace("[", r"\[").replace(")", r"\)")):
            rs.simplify(verts, tris, cell)

    big = np.float32(4096.0)
    for value, at in ((big, 700), (-big, 3), (np.nan, 999), (np.inf, 64), (-np.inf, 0)):
        v = m["verts"].copy()
        v[at, 1] = value
        v[999, 2] = np.nan                                                      # a later offender is not the one named
        refused(v, m["tris"], m["cell"], "vertex %d (" % at)
        assert "not finite or not below 4096 m" in L.er_last_error().decode()
    # one cell beyond the last, either side; a coordinate offender ahead of it is named instead
    c = np.float32(2.0 ** -9)
    for value, at in ((np.float32(2048.0), 500), (np.nextafter(np.float32(-2048.0), np.float32(-4096.0)), 256)):
        v = m["verts"].copy()
        v[at, 0] = value
        v[800, 0] = value
        refused(v, m["tris"], c, "vertex %d (" % at)
        assert "outside [-2^20, 2^20)" in L.er_last_error().decode()
        v[at - 1, 2] = np.inf
        refused(v, m["tris"], c, "vertex %d (" % (at - 1))
        assert "not finite" in L.er_last_error().decode()
    # the first out-of-range index
    for bad, at in ((1000, 3), (-1, 1), (2 ** 31 - 1, 1999), (1000, 0)):
        t = m["tris"].copy()
        t[at, 1] = bad
        t[1999, 2] = 1005
        refused(m["verts"], t, m["cell"], "triangle %d names vertex %d, outside [0, 1000)" % (at, bad))
    v = m["verts"].copy()                                                       # vertices are looked at before triangles
    v[10, 0] = np.nan
    t = m["tris"].copy()
    t[0, 0] = -5
    refused(v, t, m["cell"], "vertex 10 (")
    with pytest.raises(_ffi.ErError, match="device 99"):
        mesh.simplify(m["verts"], m["tris"], m["cell"], device=99)
    with pytest.raises(_ffi.ErError, match="finite and above 0"):
        mesh.simplify(m["verts"], m["tris"], 0.0)


def test_counts_only_each_output_alone_and_small_capacities(gpu):
    L = _ffi.lib()
    m = cases.random_mesh(4097, 9000, 51, per_cell=3.0)
    w = rs.simplify(**m)
    n, k = len(w["verts"]), len(w["tris"])
    assert 0 < n < 4097 and 0 < k < 9000
    wn = np.concatenate([w["normals"], np.zeros((n, 1), np.float32)], 1)
    nv, nt = C.c_long(-1), C.c_long(-1)
    st = (C.c_long * 4)(-1, -1, -1, -1)
    p = lambda a: None if a is None else _ffi.ptr(a)

    def call(vo=None, no=None, co=None, mo=None, cv=0, to=None, io=None, ct=0, cl=None, s=st):
        return L.er_mesh_simplify(p(m["verts"]), p(m["normals"]), p(m["colors"]), 4097, p(m["tris"]), 9000, C.c_float(m["cell"]), 0, p(vo), p(no), p(co), p(mo), cv,
                                  p(to), p(io), ct, p(cl), C.byref(nv), C.byref(nt), s, None)

    def fresh():
        return dict(vo=np.zeros((n, 4), np.float32), no=np.zeros((n, 4), np.float32), co=np.zeros((n, 4), np.uint8), mo=np.zeros(n, np.int32),
                    to=np.zeros((k, 3), np.int32), io=np.zeros(k, np.int32), cl=np.zeros(4097, np.int32))

    assert call() == 0 and (nv.value, nt.value) == (n, k) and tuple(st) == w["stats"]                      # counts only
    assert call(s=None) == 0 and (nv.value, nt.value) == (n, k)                                            # stats are nullable
    f = fresh()
    assert call(vo=f["vo"], cv=n) == 0 and np.array_equal(bits(f["vo"]), bits(w["verts"]))
    assert call(no=f["no"], cv=n) == 0 and np.array_equal(np.isnan(f["no"]), np.isnan(wn)) and np.array_equal(bits(f["no"])[~np.isnan(wn)], bits(wn)[~np.isnan(wn)])
    assert call(co=f["co"], cv=n) == 0 and np.array_equal(f["co"], w["colors"])
    assert call(mo=f["mo"], cv=n) == 0 and np.array_equal(f["mo"], w["members"])
    assert call(to=f["to"], ct=k) == 0 and np.array_equal(f["to"], w["tris"])
    assert call(io=f["io"], ct=k) == 0 and np.array_equal(f["io"], w["tri_index"])
    assert call(cl=f["cl"]) == 0 and np.array_equal(f["cl"], w["cluster"])
    # a capacity one short: refused with the need in the message, counts and stats set, nothing written
    for rows in ("vo", "no", "co", "mo"):
        f = fresh()
        nv.value = nt.value = -1
        assert call(cv=n - 1, ct=k, to=f["to"], io=f["io"], cl=f["cl"], **{rows: f[rows]}) != 0
        assert L.er_last_error().decode() == "er_mesh_simplify: capacity %d < %d vertices" % (n - 1, n)
        assert (nv.value, nt.value) == (n, k) and tuple(st) == w["stats"] and not any(a.any() for a in f.values())
    for tri in ("to", "io"):
        f = fresh()
        assert call(vo=f["vo"], cv=n, ct=k - 1, cl=f["cl"], **{tri: f[tri]}) != 0
        assert L.er_last_error().decode() == "er_mesh_simplify: capacity %d < %d triangles" % (k - 1, k)
        assert (nv.value, nt.value) == (n, k) and not any(a.any() for a in f.values())


# ---- volumes ----------------------------------------------------------------------------------------------------------------------------

CELLS = [1.0, 2.0, 4.0, 7.5]                                                    # in voxels: k * 3/512 m


def check_volume(vol, source, cell, what, **kw):
    """extract_simplified_mesh against the restatement of `source` = (verts, normals, tris[, rgba]) of the same volume."""
    want = rs.simplify(source[0], source[2], cell, source[1], source[3] if len(source) > 3 else None)
    got = vol.extract_simplified_mesh(cell, stats=True, colors=len(source) > 3, **kw)
    gv, gn, gt, gs = got[0], got[1], got[2], got[-1]
    print("%s, cell %g voxels: %d vertices, %d triangles -> %d, %d; stats %s" % (what, cell / UL, gs[4], gs[5], len(gv), len(gt), gs[:4]))
    assert gv.dtype == np.float32 and gn.dtype == np.float32 and gt.dtype == np.int32 and gv.shape == want["verts"].shape and gt.shape == want["tris"].shape, what
    assert np.array_equal(bits(gv), bits(want["verts"])), what + ": vertices differ"
    assert np.array_equal(np.isnan(gn), np.isnan(want["normals"])) and np.array_equal(bits(gn)[~np.isnan(gn)], bits(want["normals"])[~np.isnan(gn)]), what
    assert np.array_equal(gt, want["tris"]), what + ": triangles differ"
    assert gs[:4] == want["stats"] and gs[4:] == (len(source[0]), len(source[2])), (what, gs, want["stats"])
    if len(source) > 3:
        assert got[3].dtype == np.uint8 and np.array_equal(got[3], want["colors"]), what + ": colours differ"
    again = vol.extract_simplified_mesh(cell, colors=len(source) > 3, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:-1], again)), what + ": another call gave other bytes"
    return got, want


@pytest.fixture(scope="module")
def planted(gpu):
    vol = volume_of(*planted_sphere_planes())
    yield dict(vol=vol, full=vol.extract_indexed_mesh())
    vol.close()


def test_the_analytic_sphere_gives_the_counts_the_definitions_give_on_the_host(gpu):
    vol = volume_of(*sphere_planes())
    full = vol.extract_indexed_mesh()
    assert (len(full[0]), len(full[2])) == (34324, 68644)
    for cell, counts in ((2.0, (7472, 14942)), (4.0, (2000, 3998)), (7.5, (587, 1172))):
        got, want = check_volume(vol, full, np.float32(cell * UL), "sphere")
        assert (len(got[0]), len(got[2])) == counts, (cell, len(got[0]), len(got[2]))
        assert got[-1][2] == 0 and got[-1][3] == 0                                # no duplicate, no orphan: the crafted lists reach those paths
        t = want["tris"]
        opposite = len(np.unique(rs.canonical(np.concatenate([t, t[:, ::-1]])), axis=0))
        pairs = (2 * len(t) - opposite) // 2                                     # (a triangle and its reverse both appear twice among the 2 n rows)
        print("sphere, cell %g voxels: %d opposite-winding pairs" % (cell, pairs))
        assert 1 <= pairs <= 3, "opposite-winding pairs"
    vol.close()


@pytest.mark.parametrize("cell", CELLS)
def test_simplified_mesh_of_the_planted_sphere(planted, cell):
    check_volume(planted["vol"], planted["full"], np.float32(cell * UL), "planted sphere")


@pytest.mark.parametrize("min_triangles,largest_only", [(9, False), (0, True), (2, False), (17, True)])
def test_simplified_mesh_of_the_cleaned_planted_sphere(planted, min_triangles, largest_only):
    vol = planted["vol"]
    cv, cn, ct, _ = vol.extract_clean_mesh(min_triangles, largest_only)
    assert len(cv) < len(planted["full"][0])
    for cell in (2.0, 7.5):
        check_volume(vol, (cv, cn, ct), np.float32(cell * UL), "planted sphere cleaned (%d, %s)" % (min_triangles, largest_only), min_triangles=min_triangles,
                     largest_only=largest_only)
    # 0 and 1 clean nothing; a cleaning that keeps nothing gives the empty mesh
    check_volume(vol, planted["full"], np.float32(4 * UL), "planted sphere, min_triangles 1", min_triangles=1)
    got = vol.extract_simplified_mesh(4 * UL, min_triangles=10 ** 6, stats=True)
    assert got[0].shape == (0, 4) and got[1].shape == (0, 3) and got[2].shape == (0, 3) and got[3] == (0, 0, 0, 0, 0, 0)
    with pytest.raises(_ffi.ErError, match="min_triangles = -1"):
        vol.extract_simplified_mesh(UL, min_triangles=-1)
    with pytest.raises(_ffi.ErError, match="finite and above 0"):
        vol.extract_simplified_mesh(0.0)


def test_simplified_mesh_of_the_box_room(gpu):
    poses, _ = helpers.golden_rigid()
    wall = 447.5 * 3.0 / 512.0
    depth = synth.to_numpy_u16(synth.render_depth(poses, hi=wall, sphere=True))
    vol = TSDFVolume(max_units=256)
    vol.IntegrateFrames(depth, poses)
    full = vol.extract_indexed_mesh()
    for cell in CELLS:
        check_volume(vol, full, np.float32(cell * UL), "box room")              # (prints the stats: whether the room reaches duplicates and orphans)
    cv, cn, ct, _ = vol.extract_clean_mesh(largest_only=True)
    check_volume(vol, (cv, cn, ct), np.float32(2 * UL), "box room, largest only", largest_only=True)
    vol.close()


def test_simplified_colours_are_the_cluster_means_of_the_unsimplified_colours(gpu):
    keys, planes = planted_sphere_planes()
    vol = volume_of(keys, planes, color=True)
    rng = np.random.default_rng(11)
    for q, k in enumerate(keys):
        n = rng.integers(0, 4, (64 ** 3, 1)).astype(np.uint32)                   # a quarter of the voxels without a sample: level 1 occurs,
        n *= q != 0                                                              # and one unit without any: its vertices stay without colour
        vol.write_unit_color(int(k), np.concatenate([rng.integers(0, 256, (64 ** 3, 3)).astype(np.uint32) * n, n], 1))
    full = vol.extract_indexed_mesh(colors=True)
    print("coloured sphere: %.1f %% of the unsimplified vertices without colour" % (100.0 * (full[3][:, 3] == 0).mean()))
    assert (full[3][:, 3] == 0).any() and (full[3][:, 3] == 255).any()
    for cell in (1.0, 2.0, 7.5):
        got, want = check_volume(vol, full, np.float32(cell * UL), "coloured sphere")
        mixed = np.bincount(want["cluster"][want["cluster"] >= 0], full[3][want["cluster"] >= 0, 3] == 0, len(got[0]))
        assert ((mixed > 0) & (mixed < want["members"])).any(), "no cluster has both coloured and uncoloured members"
        assert (got[3][:, 3] == 0).any()
    assert len(np.unique(got[3], axis=0)) > 100
    cv, cn, ct, _, cc = vol.extract_clean_mesh(9, colors=True)
    check_volume(vol, (cv, cn, ct, cc), np.float32(2 * UL), "coloured sphere cleaned", min_triangles=9)
    vol.close()


def test_an_empty_volume_and_colour_not_enabled(planted):
    e = TSDFVolume(max_units=4)
    got = e.extract_simplified_mesh(2 * UL, stats=True)
    assert got[0].shape == (0, 4) and got[1].shape == (0, 3) and got[2].shape == (0, 3) and got[3] == (0, 0, 0, 0, 0, 0)
    assert e.extract_simplified_mesh(2 * UL, largest_only=True)[2].shape == (0, 3)
    with pytest.raises(_ffi.ErError, match="er_tsdf_extract_mesh_simplified: colour is not enabled"):
        e.extract_simplified_mesh(2 * UL, colors=True)
    e.close()
    with pytest.raises(_ffi.ErError, match="colour is not enabled"):
        planted["vol"].extract_simplified_mesh(2 * UL, colors=True)
    # counts only and a capacity one short, through the C entry
    L = _ffi.lib()
    vol = planted["vol"]
    v, n, t = vol.extract_simplified_mesh(4 * UL)
    nv, nt = C.c_long(-1), C.c_long(-1)
    call = lambda vo, cv, to, ct: L.er_tsdf_extract_mesh_simplified(vol._h, C.c_float(4 * UL), 0, 0, 0, None if vo is None else _ffi.ptr(vo), None, None, None, cv,
                                                                    None if to is None else _ffi.ptr(to), ct, C.byref(nv), C.byref(nt), None, None, None)
    assert call(None, 0, None, 0) == 0 and (nv.value, nt.value) == (len(v), len(t))
    vo, to = np.zeros_like(v), np.zeros_like(t)
    assert call(vo, len(v) - 1, to, len(t)) != 0 and "capacity %d < %d vertices" % (len(v) - 1, len(v)) in L.er_last_error().decode()
    assert call(vo, len(v), to, len(t) - 1) != 0 and "capacity %d < %d triangles" % (len(t) - 1, len(t)) in L.er_last_error().decode()
    assert not vo.any() and not to.any() and (nv.value, nt.value) == (len(v), len(t))
    assert call(vo, len(v), None, 0) == 0 and np.array_equal(bits(vo), bits(v))
    assert call(None, 0, to, len(t)) == 0 and np.array_equal(to, t)
