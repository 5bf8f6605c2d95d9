"""er_tsdf_extract_mesh_indexed and er_tsdf_import_world on the GPU: the indexed mesh against the numpy restatement of
tests/mesh_restatement.py bit for bit -- vertices, indices, counts --, against the triangle soup of er_tsdf_extract_mesh, its normals against
the restatement of the oriented extraction, the topology of an analytic sphere straight from the indices, the empty cases and refusals; and
SaveWorld's inverse: a voxel list loaded back, its units, its mesh, its refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers
from elasticreconstruction_amd import _ffi, synth
from elasticreconstruction_amd.tsdf import TSDFVolume
from mesh_restatement import UL, indexed_mesh
from test_oriented_cpu import oriented_oracle
from test_oriented_gpu import hand_made_units, volume_from_units

pytestmark = pytest.mark.gpu
KEY = 256 << 18 | 256 << 9 | 256


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_normals(got, want, what):
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), "%s: NaN positions differ on %d rows" % (what, int((nan_g != nan_w).any(axis=1).sum()))
    fin = ~nan_w.any(axis=1)
    assert np.array_equal(bits(got[fin]), bits(want[fin])), "%s: finite normals differ in their bits" % what
    return float((~fin).mean())


def check_indexed(vol, units, what, want=None):
    """extract_indexed_mesh against the restatement on `units`, the soup, and the oriented restatement.  Returns (verts, normals, tris)."""
    wv, wt, _ = indexed_mesh(units) if want is None else want
    verts, nrm, tris = vol.extract_indexed_mesh()
    assert verts.dtype == np.float32 and nrm.dtype == np.float32 and tris.dtype == np.int32
    assert verts.shape == wv.shape and tris.shape == wt.shape and nrm.shape == (wv.shape[0], 3), (what, verts.shape, wv.shape, tris.shape, wt.shape)
    assert np.array_equal(bits(verts), bits(wv)), "%s: %d vertices differ" % (what, int((bits(verts) != bits(wv)).any(1).sum()))
    assert np.array_equal(tris, wt), "%s: %d triangles differ" % (what, int((tris != wt).any(1).sum()))
    if len(tris):
        assert tris.min() >= 0 and tris.max() < len(verts)
    assert np.array_equal(np.unique(tris), np.arange(len(verts))), what + ": a vertex no triangle uses"
    soup = vol.extract_mesh()
    assert np.array_equal(bits(verts[tris][..., :3]), bits(soup)), what + ": verts[tris] is not er_tsdf_extract_mesh's soup"
    share = same_normals(nrm, oriented_oracle(units, verts), what) if len(verts) else 0.0
    print("%s: %d vertices, %d triangles, %.1f %% NaN normals" % (what, len(verts), len(tris), 100 * share))
    return verts, nrm, tris


def closed_genus_0(verts, tris, what):
    """Straight from the indices, nothing welded and no sliver dropped: every undirected edge lies in exactly two triangles that traverse it
    in opposite directions, and V - E + F = 2."""
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]).astype(np.int64)
    assert (e[:, 0] != e[:, 1]).all()
    nv = len(verts)
    und = np.sort(e, 1)
    _, cnt = np.unique(und[:, 0] * nv + und[:, 1], return_counts=True)
    assert (cnt == 2).all(), "%s: %d edges are not shared by exactly two triangles" % (what, int((cnt != 2).sum()))
    assert len(np.unique(e[:, 0] * nv + e[:, 1])) == len(e), what + ": a directed edge appears twice"
    assert nv - len(cnt) + len(tris) == 2, "%s: Euler characteristic %d" % (what, nv - len(cnt) + len(tris))


# ---- the volumes the tests share ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def room(gpu):
    """The box room of the soup test: golden poses, walls at 447.5 voxels (between two units), the sphere."""
    poses, _ = helpers.golden_rigid()
    wall = 447.5 * 3.0 / 512.0
    depth = synth.to_numpy_u16(synth.render_depth(poses, hi=wall, sphere=True))
    vol = TSDFVolume(max_units=256)
    vol.IntegrateFrames(depth, poses)
    units = {int(k): vol.read_unit(k) for k in vol.unit_keys()}
    yield dict(vol=vol, units=units, want=indexed_mesh(units))
    vol.close()


def sphere_planes():
    """The analytic sphere of test_marching_cubes_of_an_analytic_sphere...: keys, [key][sdf * weight | weight] planes, weight 1."""
    c, r = np.array([0.371, 0.383, 0.377]), 0.25
    keys, planes = [], []
    ax = np.arange(64, dtype=np.float64)
    for xi in (256, 257):
        for yi in (256, 257):
            for zi in (256, 257):
                keys.append(xi * 512 * 512 + yi * 512 + zi)
                gx = (np.float32((xi - 256) * 64 * UL) + ax * UL).astype(np.float32)
                gy = (np.float32((yi - 256) * 64 * UL) + ax * UL).astype(np.float32)
                gz = (np.float32((zi - 256) * 64 * UL) + ax * UL).astype(np.float32)
                d = np.sqrt((gx[:, None, None] - c[0]) ** 2 + (gy[None, :, None] - c[1]) ** 2 + (gz[None, None, :] - c[2]) ** 2) - r
                sdf = np.clip(d / 0.03, -1.0, 1.0).astype(np.float32).reshape(-1)
                planes.append(np.stack([sdf, np.ones_like(sdf)]))
    order = np.argsort(keys)
    return np.array(keys, np.int32)[order], np.stack(planes)[order]


@pytest.fixture(scope="module")
def sphere(gpu):
    keys, planes = sphere_planes()
    buf = torch.from_numpy(planes).to("cuda:0")
    vol = TSDFVolume(max_units=16)
    vol.import_weighted(keys, buf.data_ptr())
    vol.synchronize()
    yield dict(vol=vol, mesh=vol.extract_indexed_mesh())
    vol.close()


# ---- the indexed mesh -----------------------------------------------------------------------------------------------------------------

def test_indexed_mesh_of_the_box_room_matches_the_restatement_the_soup_and_the_oriented_normals(room):
    vol, units = room["vol"], room["units"]
    verts, nrm, tris = check_indexed(vol, units, "box room", room["want"])
    assert len(tris) > 40000 and len(verts) > 20000
    # where a vertex is also one of er_tsdf_extract_oriented's points (same position bits, same axis), the two calls give the same normal
    pts, pn = vol.extract_oriented()
    where = {row.tobytes(): q for q, row in enumerate(bits(pts))}
    hit = np.array([where.get(row.tobytes(), -1) for row in bits(verts)])
    assert (hit >= 0).mean() > 0.9, (hit >= 0).mean()
    a, b = nrm[hit >= 0], pn[hit[hit >= 0]]
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a[~np.isnan(a).any(1)]), bits(b[~np.isnan(b).any(1)]))
    # the same bytes on every call
    again = vol.extract_indexed_mesh()
    for x, y in zip((verts, nrm, tris), again):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("name,base", [("middle", (256, 255, 300)), ("far corner", (510, 510, 510)), ("near corner", (0, 0, 0))])
def test_indexed_mesh_of_hand_made_volumes_matches_the_restatement(gpu, name, base):
    """Random signs, a fifth of the voxels unobserved, one unit of eight absent, in the middle of the lattice and against unit index 511 and
    0: the owner voxel in a neighbour unit, in a unit that does not exist, at both ends of the lattice."""
    units = hand_made_units(1234 + base[0], base, holes=0.2)
    vol = volume_from_units(units)
    check_indexed(vol, units, "hand-made volume, " + name)
    if name == "middle":
        gone = sorted(units)[2]
        vol.drop_units([gone])
        check_indexed(vol, {k: u for k, u in units.items() if k != gone}, "hand-made volume, one unit dropped")
    vol.close()


@pytest.mark.parametrize("neighbour", [None, 512 * 512, 1], ids=["alone", "with its +x neighbour", "with its +z neighbour"])
def test_indexed_mesh_of_alternating_signs_the_densest_rows(gpu, neighbour):
    """sdf = +-0.5 by the parity of i + j + k, every voxel observed: every lattice edge inside a complete cell is crossed.  A row (i, j) of
    a unit carries 64 x-edges, 64 y-edges and the 63 z-edges that stay in the unit; the 64th reaches into the +z unit, so only with that
    neighbour does a row carry 3 x 64 vertices, the densest the rank arithmetic can meet."""
    i, j, k = np.meshgrid(np.arange(64), np.arange(64), np.arange(64), indexing="ij")
    sdf = np.where((i + j + k) & 1, np.float32(-0.5), np.float32(0.5)).astype(np.float32).reshape(-1)
    units = {KEY: (sdf, np.ones_like(sdf))}
    if neighbour:
        units[KEY + neighbour] = (sdf.copy(), np.ones_like(sdf))
    vol = volume_from_units(units)
    verts, _, tris = check_indexed(vol, units, "alternating signs")
    # the vertices of row (i, j): an edge's lower voxel is floor(position / voxel size), every crossing here sits at the middle of its edge
    low = np.floor(verts[:, :3].astype(np.float64) / UL + 1e-3).astype(np.int64)
    per_row = np.bincount((low[:, 0] * 64 + low[:, 1]) * 2 + (low[:, 2] >> 6))          # (rows of the +z unit counted on their own)
    assert per_row.max() == (192 if neighbour == 1 else 191), per_row.max()
    vol.close()


def test_indexed_mesh_of_an_analytic_sphere_is_closed_and_of_genus_0(sphere):
    verts, nrm, tris = sphere["mesh"]
    assert len(tris) > 20000
    closed_genus_0(verts, tris, "analytic sphere")
    assert not np.isnan(nrm).any()
    c = np.array([0.371, 0.383, 0.377])
    out = verts[:, :3].astype(np.float64) - c
    assert (np.einsum("ij,ij->i", nrm.astype(np.float64), out) > 0).all()             # towards positive sdf = away from the centre


def test_indexed_mesh_keeps_edges_apart_that_meet_in_a_zero_voxel(gpu):
    rng = np.random.default_rng(5)
    sdf = rng.uniform(-1.0, 1.0, (64, 64, 64)).astype(np.float32)
    sdf[20:24, 20:24, 20:24] = -0.25
    sdf[21, 21, 21] = 0.0                                                             # outside; its six edges all end in it
    sdf[40:44, 40:44, 40:44] = -0.25
    sdf[41, 41, 41] = -0.0                                                            # -0.0 < 0 is false: outside as well
    units = {KEY: (sdf.reshape(-1), np.ones(64 ** 3, np.float32))}
    vol = volume_from_units(units)
    verts, _, _ = check_indexed(vol, units, "crafted zeros")
    distinct = len(np.unique(bits(verts[:, :3]), axis=0))
    assert len(verts) >= distinct + 10, (len(verts), distinct)                        # 2 x (6 edges -> 1 position)
    for g in (21, 41):
        at = (verts[:, :3] == (np.array([g, g, g], np.float64) * UL).astype(np.float32)).all(1)
        assert at.sum() == 6, at.sum()
    vol.close()


def test_indexed_mesh_empty_cases_queries_and_refusals(sphere):
    L = _ffi.lib()
    vol = TSDFVolume(max_units=4)
    for what in ("empty", "reset"):
        verts, nrm, tris = vol.extract_indexed_mesh()
        assert verts.shape == (0, 4) and nrm.shape == (0, 3) and tris.shape == (0, 3), what
        vol.reset()
    free = torch.ones((1, 2, 64 ** 3), dtype=torch.float32, device="cuda:0")         # sdf = 1, weight = 1: observed free space
    vol.import_raw(np.array([KEY], np.int32), free.data_ptr())
    nv, nt = C.c_long(-1), C.c_long(-1)
    assert L.er_tsdf_extract_mesh_indexed(vol._h, None, None, 0, None, 0, C.byref(nv), C.byref(nt)) == 0 and (nv.value, nt.value) == (0, 0)
    assert vol.extract_indexed_mesh()[0].shape == (0, 4)
    vol.close()

    vol = sphere["vol"]
    verts, nrm, tris = sphere["mesh"]
    n, m = len(verts), len(tris)
    nrm4 = np.concatenate([nrm, np.zeros((n, 1), np.float32)], 1)
    call = lambda v, q, cv, t, ct: L.er_tsdf_extract_mesh_indexed(vol._h, None if v is None else _ffi.ptr(v), None if q is None else _ffi.ptr(q), cv,
                                                                  None if t is None else _ffi.ptr(t), ct, C.byref(nv), C.byref(nt))
    assert call(None, None, 0, None, 0) == 0 and (nv.value, nt.value) == (n, m)       # counts only
    # each array on its own
    v = np.zeros((n, 4), np.float32)
    assert call(v, None, n, None, 0) == 0 and np.array_equal(bits(v), bits(verts))
    q = np.zeros((n, 4), np.float32)
    assert call(None, q, n, None, 0) == 0 and np.array_equal(bits(q), bits(nrm4))
    t = np.zeros((m, 3), np.int32)
    assert call(None, None, 0, t, m) == 0 and np.array_equal(t, tris)
    # capacity one short: refused with the need in the message, counts set, nothing written
    v, q, t = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros((m, 3), np.int32)
    nv.value = nt.value = -1
    assert call(v, q, n - 1, t, m) != 0
    assert L.er_last_error().decode() == "er_tsdf_extract_mesh_indexed: capacity %d < %d vertices" % (n - 1, n)
    assert (nv.value, nt.value) == (n, m) and not v.any() and not q.any() and not t.any()
    assert call(v, q, n, t, m - 1) != 0
    assert L.er_last_error().decode() == "er_tsdf_extract_mesh_indexed: capacity %d < %d triangles" % (m - 1, m)
    assert (nv.value, nt.value) == (n, m) and not v.any() and not q.any() and not t.any()
    again = vol.extract_indexed_mesh()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(sphere["mesh"], again))


# ---- SaveWorld's inverse --------------------------------------------------------------------------------------------------------------

def world_keep(sdf, w):
    return (w != 0) & (sdf < np.float32(0.98)) & (sdf >= np.float32(-0.98))


def test_load_world_of_the_box_room(room):
    A, units = room["vol"], room["units"]
    world = A.extract_world()
    B = TSDFVolume(max_units=256)
    want_units = {}
    for key, (s, w) in units.items():
        keep = world_keep(s, w)
        if keep.any():
            want_units[key] = (np.where(keep, s, np.float32(0.0)).astype(np.float32), keep.astype(np.float32))
    assert B.LoadWorld(world) == len(want_units) == B.unit_count()
    assert np.array_equal(bits(B.extract_world()), bits(world))
    assert [int(k) for k in B.unit_keys()] == sorted(want_units)
    for key, (s, w) in want_units.items():
        gs, gw = B.read_unit(key)
        assert np.array_equal(bits(gs), bits(s)) and np.array_equal(bits(gw), bits(w)), key
    vb, _, tb = check_indexed(B, want_units, "box room through world.pcd")
    rows_a = set(map(bytes, bits(A.extract_mesh()).reshape(-1, 9)))
    rows_b = list(map(bytes, bits(vb[tb][..., :3]).reshape(-1, 9)))
    assert all(r in rows_a for r in rows_b), "a triangle of the loaded volume is not one of the resident volume's"
    print("box room: the volume loaded from its SaveWorld list keeps %d of %d triangles (%.2f %%), %d of %d vertices"
          % (len(rows_b), len(rows_a), 100.0 * len(rows_b) / len(rows_a), len(vb), len(room["want"][0])))
    B.close()


def test_load_world_of_the_analytic_sphere_gives_the_same_mesh(sphere):
    """A crossing cell's corners lie within sqrt(3) voxels of the surface: |sdf| <= sqrt(3) * (3/512) / 0.03 = 0.34 < 0.98, so SaveWorld's
    filter keeps every corner of every cell that yields triangles, and the loaded volume has the very same mesh."""
    A = sphere["vol"]
    B = TSDFVolume(max_units=8)
    assert B.LoadWorld(A.extract_world()) == 8
    got = B.extract_indexed_mesh()
    for x, y in zip(sphere["mesh"], got):
        assert x.tobytes() == y.tobytes()
    closed_genus_0(got[0], got[2], "analytic sphere through world.pcd")
    B.close()


def test_load_world_refusals_leave_an_empty_reusable_volume(gpu):
    vol = TSDFVolume(max_units=2)
    good = np.array([[0, 0, 0, 0.25], [1, 0, 0, -0.25], [64, 0, 0, 0.5]], np.float32)

    def refused(rows, *needles):
        with pytest.raises(_ffi.ErError) as e:
            vol.LoadWorld(np.array(rows, np.float32))
        for s in needles:
            assert s in str(e.value), (s, str(e.value))
        assert vol.unit_count() == 0 and vol.extract_world().shape == (0, 4) and vol.sum_weight() == 0.0
        assert vol.LoadWorld(good) == 2 and vol.unit_count() == 2                     # reusable
        assert np.array_equal(bits(vol.extract_world()), bits(good))
        vol.reset()

    refused([[0, 0, 0, 0.1], [0.5, 0, 0, 0.1]], "row 1", "x = 0.5")
    refused([[0, 0, 0, 0.1], [0, 1, 0, 0.1], [0, 0, 16384, 0.1]], "row 2", "z = 16384")
    refused([[0, -16385, 0, 0.1]], "row 0", "y = -16385")
    refused([[np.nan, 0, 0, 0.1]], "row 0", "x = ")
    refused([[0, 0, 0, 0.1], [0, 0, 1, np.nan]], "row 1", "NaN")
    refused([[0, 0, 0, 0.1], [64, 0, 0, 0.1], [0, 64, 0, 0.1]], "3 units", "max_units is 2")
    refused([[0, 0, 0, 0.1], [5, 6, 7, 0.2], [0, 0, 1, 0.3], [5, 6, 7, 0.4], [0, 0, 0, 0.5]], "row 3", "(5, 6, 7)", "row 1")
    # a volume that already holds units
    assert vol.LoadWorld(good) == 2
    with pytest.raises(_ffi.ErError, match="already holds 2 units"):
        vol.LoadWorld(good)
    assert vol.unit_count() == 0
    # the lattice's ends, -0.0, and an empty list
    ends = np.array([[-16384, -16384, -16384, -0.0], [16383, 16383, 16383, 0.75]], np.float32)
    assert vol.LoadWorld(ends) == 2 and np.array_equal(bits(vol.extract_world()), bits(ends))
    assert [int(k) for k in vol.unit_keys()] == [0, 511 << 18 | 511 << 9 | 511]
    vol.reset()
    assert vol.LoadWorld(np.zeros((0, 4), np.float32)) == 0 and vol.unit_count() == 0
    vol.close()
