"""er_mesh_smooth and er_tsdf_extract_mesh_smoothed on the GPU against tests/mesh_smooth_restatement.py, bit for bit and with
the same bytes on three calls: index lists at the block and wave edges of the kernels, the crafted meshes of tests/mesh_smooth_cases.py, the
range guard, the refusals, the nullable outputs, and the smoothed extraction of volumes -- the analytic sphere with planted voxels, the box
room, a coloured volume -- against the restatement applied to the unsmoothed mesh of the same volume."""
import ctypes as C
import re

import numpy as np
import pytest

import helpers
import mesh_simplify_restatement as simplify_rs
import mesh_smooth_cases as cases
import mesh_smooth_restatement as rs
from elasticreconstruction_amd import _ffi, mesh, synth
from elasticreconstruction_amd.tsdf import TSDFVolume
from test_mesh_components_gpu import planted_sphere_planes, volume_of
from test_mesh_smooth_cpu import bits, same

pytestmark = pytest.mark.gpu
UL = 3.0 / 512.0
SIZES = cases.sizes()
CRAFTED = cases.crafted()
GUARDS = cases.guards()


def as_bytes(r):
    return b"".join(r[k].tobytes() for k in sorted(r) if isinstance(r[k], np.ndarray)) + repr(r["stats"]).encode()


def check(m, what):
    """mesh.smooth against the restatement, three times with the same bytes.  Returns the result."""
    want = rs.smooth(**m)
    got = mesh.smooth(probes=True, **m)
    probes = got.pop("probes")
    print("%s: %d vertices, %d triangles, %d iterations; stats %s; longest probe sequence %d" % (what, len(m["verts"]), len(m["tris"]), m["iterations"], got["stats"],
                                                                                            probes))
    same(got, want, what)
    nv = len(m["verts"])
    assert got["verts"].dtype == np.float32 and got["verts"].shape == (nv, 4) and got["normals"].shape == (nv, 3) and not got["verts"][:, 3].any()
    assert got["degree"].dtype == np.int32 and got["boundary"].dtype == np.uint8 and got["degree"].shape == got["boundary"].shape == (nv,)
    first = as_bytes(got)
    for _ in range(2):
        assert as_bytes(mesh.smooth(**m)) == first, what + ": another call gave other bytes"
    assert 0 <= probes <= 6 * max(len(m["tris"]), 1)
    return got


@pytest.mark.parametrize("name", list(SIZES))
def test_sizes_at_the_block_and_wave_edges(gpu, name):
    check(SIZES[name], name)


@pytest.mark.parametrize("name", list(CRAFTED))
def test_crafted_meshes_match_the_restatement(gpu, name):
    check(CRAFTED[name], name)


def test_three_column_vertices_and_the_defaults(gpu):
    m = SIZES["nv 4097, nt 8194, 10 iterations"]
    a = mesh.smooth(m["verts"][:, :3], m["tris"])
    same(a, rs.smooth(m["verts"], m["tris"]), "three columns, defaults")
    same(mesh.smooth(m["verts"], m["tris"], 0), rs.smooth(m["verts"], m["tris"], 0), "the normals of the mesh as it is")


@pytest.mark.parametrize("name", list(GUARDS))
def test_a_pass_that_leaves_the_range_is_refused_by_pass_and_vertex(gpu, name):
    L = _ffi.lib()
    m = GUARDS[name][0]
    with pytest.raises(ValueError) as e:
        rs.smooth(**m)
    number, vertex = (int(x) for x in re.search(r"pass (\d+) moves vertex (\d+) ", str(e.value)).groups())
    nv = len(m["verts"])
    vo, no = np.full((nv, 4), -7, np.float32), np.full((nv, 4), -7, np.float32)
    deg, bnd = np.full(nv, -7, np.int32), np.full(nv, 7, np.uint8)
    st, pr = (C.c_long * 4)(-7, -7, -7, -7), (C.c_long * 1)(-7)
    for _ in range(3):
        rc = L.er_mesh_smooth(_ffi.ptr(m["verts"]), nv, _ffi.ptr(m["tris"]), len(m["tris"]), m["iterations"], C.c_float(m["lam"]), C.c_float(m["mu"]),
                              int(m["fix_boundary"]), 0, _ffi.ptr(vo), _ffi.ptr(no), _ffi.ptr(deg), _ffi.ptr(bnd), st, pr)
        msg = L.er_last_error().decode()
        assert rc != 0 and msg.startswith("er_mesh_smooth: pass %d (iteration %d, %s) moves vertex %d to a coordinate" % (number, number // 2, ("lambda", "mu")[number & 1], vertex)), msg
        assert (vo == -7).all() and (no == -7).all() and (deg == -7).all() and (bnd == 7).all() and tuple(st) == (-7,) * 4 and pr[0] == -7
    # the same mesh one pass short of the offence is smoothed
    if number == 1 or (number > 0 and number % 2 == 0):
        short = dict(m, iterations=number // 2) if number % 2 == 0 else dict(m, iterations=1, mu=np.float32(0))
        same(mesh.smooth(**short), rs.smooth(**short), name + ", one pass short")


def test_refusals_name_the_first_offender_and_write_nothing(gpu):
    L = _ffi.lib()
    m = SIZES["nv 4097, nt 8194, 2 iterations"]
    nv, nt = 4097, 8194
    p = lambda a: None if a is None else _ffi.ptr(a)
    st = (C.c_long * 4)(-7, -7, -7, -7)

    def refused(verts, tris, words, **kw):
        vo, no = np.full((nv, 4), -7, np.float32), np.full((nv, 4), -7, np.float32)
        deg, bnd = np.full(nv, -7, np.int32), np.full(nv, 7, np.uint8)
        a = dict(it=2, lam=0.5, mu=-0.53, device=0)
        a.update(kw)
        rc = L.er_mesh_smooth(p(verts), len(verts), p(tris), len(tris), a["it"], C.c_float(a["lam"]), C.c_float(a["mu"]), 0, a["device"], p(vo), p(no), p(deg), p(bnd), st, None)
        msg = L.er_last_error().decode()
        assert rc != 0 and msg.startswith("er_mesh_smooth: " + words), msg
        assert (vo == -7).all() and (no == -7).all() and (deg == -7).all() and (bnd == 7).all() and tuple(st) == (-7,) * 4
        return msg

    big = np.float32(4096.0)
    for value, at in ((big, 700), (-big, 3), (np.nan, 4096), (np.inf, 64), (-np.inf, 0)):
        v = m["verts"].copy()
        v[at, 1] = value
        v[4096, 2] = np.nan                                                     # a later offender is not the one named
        assert "not finite or not below 4096 m" in refused(v, m["tris"], "vertex %d (" % at)
        with pytest.raises(ValueError, match="vertex %d has" % at):
            rs.smooth(v, m["tris"])
    for bad, at in ((4097, 3), (-1, 1), (2 ** 31 - 1, 8193), (4097, 0)):
        t = m["tris"].copy()
        t[at, 1] = bad
        t[8193, 2] = 5000
        refused(m["verts"], t, "triangle %d names vertex %d, outside [0, 4097)" % (at, bad))
        with pytest.raises(ValueError, match=r"triangle %d names vertex %d, outside \[0, 4097\)" % (at, bad)):
            rs.smooth(m["verts"], t)
    v = m["verts"].copy()                                                       # vertices are looked at before triangles
    v[10, 0] = np.nan
    t = m["tris"].copy()
    t[0, 0] = -5
    refused(v, t, "vertex 10 (")
    refused(m["verts"], m["tris"], "device 99", device=99)
    refused(m["verts"], m["tris"], "iterations = 1025", it=1025)
    refused(m["verts"], m["tris"], "iterations = -1", it=-1)
    refused(m["verts"], m["tris"], "lambda = 1.5", lam=1.5)
    refused(m["verts"], m["tris"], "mu = nan", mu=float("nan"))
    refused(m["verts"], m["tris"], "mu = -inf", mu=float("-inf"))
    with pytest.raises(_ffi.ErError, match="lambda = -2"):
        mesh.smooth(m["verts"], m["tris"], lam=-2.0)


def test_each_output_alone_and_all_null(gpu):
    L = _ffi.lib()
    m = SIZES["nv 4097, nt 8194, 2 iterations"]
    w = rs.smooth(**m)
    nv = 4097
    p = lambda a: None if a is None else _ffi.ptr(a)
    st, pr = (C.c_long * 4)(-1, -1, -1, -1), (C.c_long * 1)(-1)

    def call(vo=None, no=None, deg=None, bnd=None, s=st, q=None):
        return L.er_mesh_smooth(p(m["verts"]), nv, p(m["tris"]), len(m["tris"]), 2, C.c_float(m["lam"]), C.c_float(m["mu"]), int(m["fix_boundary"]), 0, p(vo), p(no),
                                p(deg), p(bnd), s, q)

    assert call() == 0 and tuple(st) == w["stats"]                             # all NULL: the stats alone
    assert call(s=None) == 0                                                   # and they are nullable too
    assert call(q=pr) == 0 and pr[0] >= 1
    vo, no, deg, bnd = np.zeros((nv, 4), np.float32), np.zeros((nv, 4), np.float32), np.zeros(nv, np.int32), np.zeros(nv, np.uint8)
    assert call(vo=vo) == 0 and np.array_equal(bits(vo), bits(w["verts"]))
    assert call(no=no) == 0 and not no[:, 3].any()
    nn = np.isnan(w["normals"])
    assert np.array_equal(np.isnan(no[:, :3]), nn) and np.array_equal(bits(no[:, :3])[~nn], bits(w["normals"])[~nn])
    assert call(deg=deg) == 0 and np.array_equal(deg, w["degree"])
    assert call(bnd=bnd) == 0 and np.array_equal(bnd, w["boundary"])
    # no vertex: nothing is written, whatever the triangles say
    assert L.er_mesh_smooth(None, 0, p(m["tris"]), 5, 2, C.c_float(0.5), C.c_float(-0.53), 0, 0, p(vo), None, None, None, st, None) == 0 and tuple(st) == (0, 0, 0, 0)
    assert np.array_equal(bits(vo), bits(w["verts"]))


# ---- volumes ----------------------------------------------------------------------------------------------------------------------------

def smoothed(source, iterations, cell=0.0, **kw):
    """The restatement of the route: source = (verts, normals, tris[, rgba]) of the unsmoothed mesh -> (verts, normals, tris, rgba | None,
    smoothing stats, clustering stats)"""
    w = rs.smooth(source[0], source[2], iterations, **kw)
    rgba = source[3] if len(source) > 3 else None
    if cell == 0:
        return w["verts"], w["normals"], source[2], rgba, w["stats"], (0, 0, 0, 0)
    s = simplify_rs.simplify(w["verts"], source[2], cell, w["normals"], rgba)
    return s["verts"], s["normals"], s["tris"], s["colors"], w["stats"], s["stats"]


def check_volume(vol, source, iterations, what, cell=0.0, lam=0.5, mu=-0.53, fix_boundary=False, **kw):
    want = smoothed(source, iterations, cell, lam=lam, mu=mu, fix_boundary=fix_boundary)
    colors = len(source) > 3
    got = vol.extract_smoothed_mesh(iterations, lam, mu, fix_boundary, cell, stats=True, colors=colors, **kw)
    gv, gn, gt, gs = got[0], got[1], got[2], got[-1]
    print("%s, %d iterations, cell %g voxels: %d vertices, %d triangles -> %d, %d; stats %s" % (what, iterations, cell / UL, gs[8], gs[9], len(gv), len(gt), gs[:8]))
    assert gv.dtype == np.float32 and gn.dtype == np.float32 and gt.dtype == np.int32 and gv.shape == want[0].shape and gt.shape == want[2].shape, what
    assert np.array_equal(bits(gv), bits(want[0])), what + ": vertices differ"
    assert np.array_equal(np.isnan(gn), np.isnan(want[1])) and np.array_equal(bits(gn)[~np.isnan(gn)], bits(want[1])[~np.isnan(gn)]), what + ": normals differ"
    assert np.array_equal(gt, want[2]), what + ": triangles differ"
    assert gs[:4] == want[4] and gs[4:8] == want[5] and gs[8:] == (len(source[0]), len(source[2])), (what, gs, want[4], want[5])
    if colors:
        assert got[3].dtype == np.uint8 and np.array_equal(got[3], want[3]), what + ": colours differ"
    again = vol.extract_smoothed_mesh(iterations, lam, mu, fix_boundary, cell, colors=colors, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:-1], again)), what + ": another call gave other bytes"
    return got


@pytest.fixture(scope="module")
def planted(gpu):
    vol = volume_of(*planted_sphere_planes())
    yield dict(vol=vol, full=vol.extract_indexed_mesh())
    vol.close()


@pytest.mark.parametrize("iterations,cell,kw", [(1, 0.0, {}), (10, 0.0, {}), (3, 2.0, {}), (2, 0.0, dict(fix_boundary=True)), (2, 2.0, dict(lam=0.7, mu=0.0))],
                         ids=["1", "10", "3, cell 2", "2, boundary fixed", "2 Laplacian, cell 2"])
def test_smoothed_mesh_of_the_planted_sphere(planted, iterations, cell, kw):
    got = check_volume(planted["vol"], planted["full"], iterations, "planted sphere", np.float32(cell * UL), **kw)
    if cell == 0:
        assert not np.array_equal(bits(got[0][:, :3]), bits(planted["full"][0][:, :3])) and not got[0][:, 3].any()


@pytest.mark.parametrize("min_triangles,largest_only", [(9, False), (0, True)])
def test_smoothed_mesh_of_the_cleaned_planted_sphere(planted, min_triangles, largest_only):
    vol = planted["vol"]
    cv, cn, ct, _ = vol.extract_clean_mesh(min_triangles, largest_only)
    assert len(cv) < len(planted["full"][0])
    for cell in (0.0, 2.0):
        check_volume(vol, (cv, cn, ct), 4, "planted sphere cleaned (%d, %s)" % (min_triangles, largest_only), np.float32(cell * UL), min_triangles=min_triangles,
                     largest_only=largest_only)
    got = vol.extract_smoothed_mesh(3, min_triangles=10 ** 6, stats=True)        # a cleaning that keeps nothing
    assert got[0].shape == (0, 4) and got[1].shape == (0, 3) and got[2].shape == (0, 3) and got[3] == (0,) * 10


def test_no_iterations_give_the_bytes_of_the_existing_routes(planted):
    vol, full = planted["vol"], planted["full"]
    got = vol.extract_smoothed_mesh(0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, full)) and len(got[0]) > 1000
    assert got[0][:, 3].any(), "the 4th column is extract_indexed_mesh's axis, not the smoothing's 0"
    clean = vol.extract_clean_mesh(9)
    got = vol.extract_smoothed_mesh(0, min_triangles=9)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, clean[:3]))
    cell = np.float32(2 * UL)
    for kw in ({}, dict(largest_only=True)):
        want = vol.extract_simplified_mesh(cell, stats=True, **kw)
        got = vol.extract_smoothed_mesh(0, cell=cell, stats=True, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:3], want[:3]))
        assert got[3] == (0, 0, 0, 0) + want[3]
    # a factor of 0 and 0 runs no pass either, but the stage is not skipped: positions x y z 0 and the normals of the triangles
    got = vol.extract_smoothed_mesh(5, lam=0.0, mu=0.0)
    assert np.array_equal(bits(got[0][:, :3]), bits(full[0][:, :3])) and not got[0][:, 3].any()
    want = rs.smooth(full[0], full[2], 0)["normals"]
    assert np.array_equal(np.isnan(got[1]), np.isnan(want)) and np.array_equal(bits(got[1])[~np.isnan(want)], bits(want)[~np.isnan(want)])


def test_smoothed_mesh_of_the_box_room(gpu):
    poses, _ = helpers.golden_rigid()
    wall = 447.5 * 3.0 / 512.0
    depth = synth.to_numpy_u16(synth.render_depth(poses, hi=wall, sphere=True))
    vol = TSDFVolume(max_units=256)
    vol.IntegrateFrames(depth, poses)
    full = vol.extract_indexed_mesh()
    check_volume(vol, full, 10, "box room")
    check_volume(vol, full, 2, "box room", np.float32(2 * UL), fix_boundary=True)
    cv, cn, ct, _ = vol.extract_clean_mesh(largest_only=True)
    check_volume(vol, (cv, cn, ct), 3, "box room, largest only", np.float32(2 * UL), largest_only=True)
    vol.close()


def test_colours_are_those_of_the_unsmoothed_vertices(gpu):
    keys, planes = planted_sphere_planes()
    vol = volume_of(keys, planes, color=True)
    rng = np.random.default_rng(11)
    for q, k in enumerate(keys):
        n = rng.integers(0, 4, (64 ** 3, 1)).astype(np.uint32)
        n *= q != 0
        vol.write_unit_color(int(k), np.concatenate([rng.integers(0, 256, (64 ** 3, 3)).astype(np.uint32) * n, n], 1))
    full = vol.extract_indexed_mesh(colors=True)
    assert (full[3][:, 3] == 0).any() and (full[3][:, 3] == 255).any()
    got = check_volume(vol, full, 10, "coloured sphere")
    after = vol.sample_colors(got[0])
    print("coloured sphere: %.1f %% of the vertices would be coloured otherwise at their smoothed positions" % (100.0 * (after != full[3]).any(axis=1).mean()))
    assert (after != full[3]).any(axis=1).mean() > 0.05, "sampling after the smoothing would pass"
    check_volume(vol, full, 3, "coloured sphere", np.float32(2 * UL))
    cv, cn, ct, _, cc = vol.extract_clean_mesh(9, colors=True)
    check_volume(vol, (cv, cn, ct, cc), 2, "coloured sphere cleaned", np.float32(2 * UL), min_triangles=9)
    check_volume(vol, (cv, cn, ct, cc), 2, "coloured sphere cleaned", min_triangles=9)
    vol.close()


def test_an_empty_volume_colour_not_enabled_and_capacities(planted):
    e = TSDFVolume(max_units=4)
    for cell in (0.0, 2 * UL):
        got = e.extract_smoothed_mesh(3, cell=cell, stats=True)
        assert got[0].shape == (0, 4) and got[1].shape == (0, 3) and got[2].shape == (0, 3) and got[3] == (0,) * 10
    assert e.extract_smoothed_mesh(3, largest_only=True)[2].shape == (0, 3)
    with pytest.raises(_ffi.ErError, match="er_tsdf_extract_mesh_smoothed: colour is not enabled"):
        e.extract_smoothed_mesh(3, colors=True)
    e.close()
    vol = planted["vol"]
    with pytest.raises(_ffi.ErError, match="colour is not enabled"):
        vol.extract_smoothed_mesh(3, colors=True)
    with pytest.raises(_ffi.ErError, match="min_triangles = -1"):
        vol.extract_smoothed_mesh(3, min_triangles=-1)
    with pytest.raises(_ffi.ErError, match="finite and not below 0"):
        vol.extract_smoothed_mesh(3, cell=-1.0)
    with pytest.raises(_ffi.ErError, match="iterations = 2000"):
        vol.extract_smoothed_mesh(2000)
    # counts only and capacities one short, through the C entry, without and with the clustering
    L = _ffi.lib()
    for cell in (0.0, 4 * UL):
        v, n, t = vol.extract_smoothed_mesh(2, cell=cell)
        nv, nt = C.c_long(-1), C.c_long(-1)
        call = lambda vo, cv, to, ct: L.er_tsdf_extract_mesh_smoothed(vol._h, 2, C.c_float(0.5), C.c_float(-0.53), 0, C.c_float(cell), 0, 0, 0, None if vo is None else _ffi.ptr(vo),
                                                                      None, None, cv, None if to is None else _ffi.ptr(to), ct, C.byref(nv), C.byref(nt), None, None, None)
        assert call(None, 0, None, 0) == 0 and (nv.value, nt.value) == (len(v), len(t))
        vo, to = np.zeros_like(v), np.zeros_like(t)
        nv.value = nt.value = -1
        assert call(vo, len(v) - 1, to, len(t)) != 0 and "capacity %d < %d vertices" % (len(v) - 1, len(v)) in L.er_last_error().decode()
        assert (nv.value, nt.value) == (len(v), len(t))
        assert call(vo, len(v), to, len(t) - 1) != 0 and "capacity %d < %d triangles" % (len(t) - 1, len(t)) in L.er_last_error().decode()
        assert not vo.any() and not to.any() and (nv.value, nt.value) == (len(v), len(t))
        assert call(vo, len(v), None, 0) == 0 and np.array_equal(bits(vo), bits(v))
        assert call(None, 0, to, len(t)) == 0 and np.array_equal(to, t)
