"""er_mesh_components and er_tsdf_extract_mesh_cleaned on the GPU against tests/mesh_components_restatement.py: labels,
counts and component numbers of index lists at the wave and workgroup edges of the kernels; and the cleaned extraction of crafted volumes --
an analytic sphere with planted voxels, the box room, a coloured volume -- against the restatement applied to the unfiltered
extract_indexed_mesh of the same volume, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers
import mesh_components_cases as cases
from elasticreconstruction_amd import _ffi, mesh, synth
from elasticreconstruction_amd.tsdf import TSDFVolume
from mesh_components_restatement import clean, components
from test_mesh_indexed_gpu import bits, closed_genus_0, sphere_planes

pytestmark = pytest.mark.gpu


# ---- the labelling entry ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cases.index_lists()))
def test_components_of_index_lists_match_the_restatement(gpu, name):
    tris, nv = cases.index_lists()[name]
    wl, wc, wn = components(tris, nv)
    labels, counts, n, rounds = mesh.components(tris, nv, rounds=True)
    print("%s: %d triangles, %d vertices, %d components, %d rounds on the device" % (name, len(tris), nv, n, rounds))
    assert labels.dtype == np.int32 and counts.dtype == np.int64 and labels.shape == (nv,) and counts.shape == (nv,)
    assert np.array_equal(labels, wl), "%s: %d labels differ" % (name, int((labels != wl).sum()))
    assert np.array_equal(counts, wc), "%s: %d counts differ" % (name, int((counts != wc).sum()))
    assert n == wn
    assert (rounds == 0) == (len(tris) == 0) and rounds <= 256                 # (a quarter of the cap of the round loop)
    if name.startswith(("strip", "fan")):
        assert not labels.any() and n == 1
    again = mesh.components(tris, nv)
    assert again[0].tobytes() == labels.tobytes() and again[1].tobytes() == counts.tobytes() and again[2] == n


def test_components_nullable_outputs_and_refusals(gpu):
    L = _ffi.lib()
    tris, nv = cases.unused_vertices()
    wl, wc, wn = components(tris, nv)
    nc, r = C.c_long(-1), C.c_int(-1)
    assert L.er_mesh_components(_ffi.ptr(tris), len(tris), nv, 0, None, None, C.byref(nc), None) == 0 and nc.value == wn
    lab = np.full(nv, -7, np.int32)
    assert L.er_mesh_components(_ffi.ptr(tris), len(tris), nv, 0, _ffi.ptr(lab), None, C.byref(nc), C.byref(r)) == 0
    assert np.array_equal(lab, wl) and r.value >= 1
    cnt = np.full(nv, -7, np.int64)
    assert L.er_mesh_components(_ffi.ptr(tris), len(tris), nv, 0, None, _ffi.ptr(cnt), C.byref(nc), None) == 0 and np.array_equal(cnt, wc)
    # no triangle, no vertex
    assert L.er_mesh_components(None, 0, 0, 0, None, None, C.byref(nc), C.byref(r)) == 0 and (nc.value, r.value) == (0, 0)
    # an index that names no vertex: the first offending triangle in triangle order, nothing written
    for bad, at in ((nv, 3), (-1, 1), (2 ** 31 - 1, 4)):
        t = tris.copy()
        t[at, 1] = bad
        t[4, 2] = nv + 5                                                        # a later offender is not the one named
        lab[:], cnt[:], nc.value, r.value = -7, -7, -7, -7
        assert L.er_mesh_components(_ffi.ptr(t), len(t), nv, 0, _ffi.ptr(lab), _ffi.ptr(cnt), C.byref(nc), C.byref(r)) != 0
        msg = L.er_last_error().decode()
        assert msg == "er_mesh_components: triangle %d names vertex %d, outside [0, %d)" % (at, bad, nv), msg
        assert (lab == -7).all() and (cnt == -7).all() and (nc.value, r.value) == (-7, -7)
    with pytest.raises(_ffi.ErError, match="triangle 0 names vertex 3"):
        mesh.components(np.array([[0, 1, 3]], np.int32), 3)
    with pytest.raises(_ffi.ErError, match="device 99"):
        mesh.components(tris, nv, device=99)


# ---- the cleaned extraction -------------------------------------------------------------------------------------------------------------

# Voxels planted in the analytic sphere's eight units (global voxel 0 .. 127 per axis; the sphere's centre is near (63, 65, 64), its radius 42.7
# voxels, its band 5.1 voxels: beyond 48 voxels from the centre the sdf is +1, within 37 it is -1).  tests/test_mesh_components_cpu.py asserts
# the shell each kind gives.
OUTSIDE = {
    "interior octahedron a": ([(5, 5, 5)], [8]),
    "interior octahedron b": ([(120, 121, 122)], [8]),
    "at a face of the lattice of units": ([(0, 30, 40)], [4]),
    "at an edge": ([(127, 127, 40)], [2]),
    "at a corner": ([(0, 127, 0)], [1]),
    "across a unit border": ([(63, 10, 10), (64, 10, 10)], [16]),
    "voxel 63 with the +x unit present": ([(63, 20, 5)], [8]),
    "adjacent pair": ([(10, 100, 10), (10, 101, 10)], [16]),
    "face-diagonal pair": ([(100, 10, 10), (101, 11, 10)], [8, 8]),
    "body-diagonal pair": ([(100, 100, 10), (101, 101, 11)], [8, 8]),
}
INSIDE = [(60, 60, 60)]                                                          # an inverted octahedron: one free voxel inside the sphere
SHELLS = sorted([c for _, counts in OUTSIDE.values() for c in counts] + [8])


def planted_sphere_planes():
    keys, planes = sphere_planes()
    planes = planes.copy()
    where = {int(k): q for q, k in enumerate(keys)}

    def put(g, value):
        key = (256 + (g[0] >> 6)) << 18 | (256 + (g[1] >> 6)) << 9 | (256 + (g[2] >> 6))
        v = ((g[0] & 63) * 64 + (g[1] & 63)) * 64 + (g[2] & 63)
        assert planes[where[key], 0, v] == (-value / abs(value))                 # planted in clipped free space / clipped interior only
        planes[where[key], 0, v] = value                                         # (weight 1: the plane sdf * weight is the sdf)

    for voxels, _ in OUTSIDE.values():
        for g in voxels:
            put(g, np.float32(-0.5))
    for g in INSIDE:
        put(g, np.float32(0.5))
    return keys, planes


def volume_of(keys, planes, color=False):
    buf = torch.from_numpy(planes).to("cuda:0")
    vol = TSDFVolume(max_units=16)
    if color:
        vol.enable_color()
    vol.import_weighted(keys, buf.data_ptr())
    vol.synchronize()
    return vol


@pytest.fixture(scope="module")
def planted(gpu):
    """The planted sphere: the volume, its unfiltered mesh, that mesh's components by the restatement, and the sphere's own triangle count."""
    vol = volume_of(*planted_sphere_planes())
    full = vol.extract_indexed_mesh()
    comps = components(full[2], len(full[0]))
    labels, counts, n = comps
    roots = np.flatnonzero(labels == np.arange(len(labels)))
    assert n == len(SHELLS) + 1 and sorted(counts[roots].tolist())[:-1] == SHELLS, sorted(counts[roots].tolist())[:10]
    clean_vol = volume_of(*sphere_planes())
    sphere_tris = len(clean_vol.extract_indexed_mesh()[2])
    clean_vol.close()
    assert sphere_tris == counts[roots].max() > 20000
    yield dict(vol=vol, full=full, comps=comps, sphere_tris=int(sphere_tris))
    vol.close()


def check_cleaned(vol, full, comps, min_triangles, largest_only, what):
    """extract_clean_mesh against the restatement applied to the unfiltered mesh `full` of the same volume.  Returns what the call returned."""
    verts, nrm, tris = full
    index, wt, wstats = clean(tris, len(verts), min_triangles, largest_only, comps)
    got = vol.extract_clean_mesh(min_triangles, largest_only, stats=True)
    gv, gn, gt, gi, gstats = got
    assert gv.dtype == np.float32 and gn.dtype == np.float32 and gt.dtype == np.int32 and gi.dtype == np.int32
    assert gv.shape == (len(index), 4) and gn.shape == (len(index), 3) and gt.shape == wt.shape and gi.shape == index.shape, what
    assert np.array_equal(gi, index), what + ": index differs"
    assert np.array_equal(bits(gv), bits(verts[index])), what + ": vertices differ"
    assert np.array_equal(np.isnan(gn), np.isnan(nrm[index])) and np.array_equal(bits(gn), bits(nrm[index])), what + ": normals differ"
    assert np.array_equal(gt, wt), what + ": triangles differ"
    assert tuple(gstats) == wstats, (what, gstats, wstats)
    return got


def thresholds(sphere_tris):
    return [0, 1, 2, 4, 5, 8, 9, 16, 17, sphere_tris, sphere_tris + 1]


@pytest.mark.parametrize("largest_only", [False, True], ids=["every component", "largest only"])
@pytest.mark.parametrize("which", range(11), ids=["0", "1", "2", "4", "5", "8", "9", "16", "17", "the sphere's count", "the sphere's count + 1"])
def test_cleaned_mesh_of_the_planted_sphere_matches_the_restatement(planted, which, largest_only):
    m = thresholds(planted["sphere_tris"])[which]
    got = check_cleaned(planted["vol"], planted["full"], planted["comps"], m, largest_only, "planted sphere, min_triangles %d" % m)
    n_shells = 1 if largest_only else 1 + sum(c >= m for c in SHELLS)
    if m > planted["sphere_tris"]:
        n_shells = 0
        assert got[0].shape == (0, 4) and got[2].shape == (0, 3)                  # the empty mesh, and the call succeeds
    assert got[4][0] == len(SHELLS) + 1 and got[4][1] == n_shells


def test_cleaned_mesh_of_the_planted_sphere_further_properties(planted):
    vol, full, st = planted["vol"], planted["full"], planted["sphere_tris"]
    # min_triangles = 9 leaves exactly the sphere and the two 16-triangle blobs
    verts, nrm, tris, index, stats = vol.extract_clean_mesh(9, stats=True)
    labels, counts, n = components(tris, len(verts))
    roots = np.flatnonzero(labels == np.arange(len(verts)))
    assert n == 3 and sorted(counts[roots].tolist()) == [16, 16, st] and stats[1] == 3 and stats[3] == sum(c for c in SHELLS if c < 9)
    assert np.array_equal(bits(verts), bits(full[0][index])) and (np.diff(index) > 0).all()
    # largest_only leaves the sphere: closed, genus 0, and the mesh of the volume nothing was planted in (but for the inverted octahedron's
    # neighbourhood, which lies inside and changes no sphere vertex)
    verts, nrm, tris, index = vol.extract_clean_mesh(largest_only=True)
    assert len(tris) == st
    closed_genus_0(verts, tris, "planted sphere, largest only")
    assert np.array_equal(bits(verts), bits(full[0][index]))
    # min_triangles <= 1: extract_indexed_mesh byte for byte
    for m in (0, 1):
        got = vol.extract_clean_mesh(m)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:3], full)) and np.array_equal(got[3], np.arange(len(full[0])))
    # the same bytes on every call
    a, b = vol.extract_clean_mesh(9), vol.extract_clean_mesh(9)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    with pytest.raises(_ffi.ErError, match="min_triangles = -1"):
        vol.extract_clean_mesh(-1)


def test_cleaned_mesh_counts_only_each_array_alone_small_capacities_and_an_empty_volume(planted):
    L = _ffi.lib()
    vol = planted["vol"]
    verts, nrm, tris, index, wstats = vol.extract_clean_mesh(9, stats=True)
    nrm4 = np.concatenate([nrm, np.zeros((len(nrm), 1), np.float32)], 1)
    n, m = len(verts), len(tris)
    nv, nt = C.c_long(-1), C.c_long(-1)
    st = (C.c_long * 4)(-1, -1, -1, -1)
    p = lambda a: None if a is None else _ffi.ptr(a)
    call = lambda v, q, i, cv, t, ct, s=st: L.er_tsdf_extract_mesh_cleaned(vol._h, 9, 0, p(v), p(q), p(i), cv, p(t), ct, C.byref(nv), C.byref(nt), s)
    assert call(None, None, None, 0, None, 0) == 0 and (nv.value, nt.value) == (n, m) and tuple(st) == wstats     # counts only: those after filtering
    assert call(None, None, None, 0, None, 0, None) == 0 and (nv.value, nt.value) == (n, m)                       # stats are nullable
    v, q, i, t = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros(n, np.int32), np.zeros((m, 3), np.int32)
    assert call(v, None, None, n, None, 0) == 0 and np.array_equal(bits(v), bits(verts))
    assert call(None, q, None, n, None, 0) == 0 and np.array_equal(bits(q), bits(nrm4))
    assert call(None, None, i, n, None, 0) == 0 and np.array_equal(i, index)
    assert call(None, None, None, 0, t, m) == 0 and np.array_equal(t, tris)
    # a capacity one short: refused with the need in the message, counts and stats set, nothing written
    for arrays in ((True, True, True), (False, False, True)):
        v, q, i, t = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros(n, np.int32), np.zeros((m, 3), np.int32)
        nv.value = nt.value = -1
        assert call(v if arrays[0] else None, q if arrays[1] else None, i, n - 1, t, m) != 0
        assert L.er_last_error().decode() == "er_tsdf_extract_mesh_cleaned: capacity %d < %d vertices" % (n - 1, n)
        assert (nv.value, nt.value) == (n, m) and tuple(st) == wstats and not v.any() and not q.any() and not i.any() and not t.any()
    assert call(v, q, i, n, t, m - 1) != 0
    assert L.er_last_error().decode() == "er_tsdf_extract_mesh_cleaned: capacity %d < %d triangles" % (m - 1, m)
    assert (nv.value, nt.value) == (n, m) and not v.any() and not q.any() and not i.any() and not t.any()
    # an empty volume, and observed free space without a crossing
    e = TSDFVolume(max_units=4)
    for largest in (False, True):
        got = e.extract_clean_mesh(5, largest, stats=True)
        assert got[0].shape == (0, 4) and got[1].shape == (0, 3) and got[2].shape == (0, 3) and got[3].shape == (0,) and got[4] == (0, 0, 0, 0)
    free = torch.ones((1, 2, 64 ** 3), dtype=torch.float32, device="cuda:0")
    e.import_raw(np.array([cases.KEY], np.int32), free.data_ptr())
    assert e.extract_clean_mesh(0, stats=True)[4] == (0, 0, 0, 0) and e.extract_clean_mesh(largest_only=True)[2].shape == (0, 3)
    e.close()


def test_cleaned_mesh_of_the_box_room_matches_the_restatement(gpu):
    """The box room of tests/test_mesh_indexed_gpu.py: a mesh of an integrated volume, several units wide, whatever components it has."""
    poses, _ = helpers.golden_rigid()
    wall = 447.5 * 3.0 / 512.0
    depth = synth.to_numpy_u16(synth.render_depth(poses, hi=wall, sphere=True))
    vol = TSDFVolume(max_units=256)
    vol.IntegrateFrames(depth, poses)
    full = vol.extract_indexed_mesh()
    comps = components(full[2], len(full[0]))
    labels, counts, n = comps
    roots = np.flatnonzero(labels == np.arange(len(labels)))
    sizes = sorted(counts[roots].tolist())
    print("box room: %d vertices, %d triangles, %d components, the smallest %s, the largest %s" % (len(full[0]), len(full[2]), n, sizes[:5], sizes[-3:]))
    gl, gc, gn, rounds = mesh.components(full[2], len(full[0]), rounds=True)
    print("box room: %d rounds on the device" % rounds)
    assert np.array_equal(gl, labels) and np.array_equal(gc, counts) and gn == n
    for m in sorted({0, 2, sizes[0] + 1, sizes[-1], sizes[-1] + 1}):
        for largest in (False, True):
            check_cleaned(vol, full, comps, m, largest, "box room, min_triangles %d" % m)
    vol.close()


def test_cleaned_colours_are_the_unfiltered_colours_of_the_kept_vertices(gpu):
    keys, planes = planted_sphere_planes()
    vol = volume_of(keys, planes, color=True)
    rng = np.random.default_rng(11)
    for k in keys:
        n = rng.integers(0, 4, (64 ** 3, 1)).astype(np.uint32)                   # a quarter of the voxels without a sample: level 1 and "no colour" occur
        vol.write_unit_color(int(k), np.concatenate([rng.integers(0, 256, (64 ** 3, 3)).astype(np.uint32) * n, n], 1))
    full = vol.extract_indexed_mesh(colors=True)
    assert len(np.unique(full[3], axis=0)) > 100
    for m, largest in ((9, False), (0, True), (2, False)):
        verts, nrm, tris, index, rgba = vol.extract_clean_mesh(m, largest, colors=True)
        assert rgba.dtype == np.uint8 and rgba.shape == (len(verts), 4) and np.array_equal(rgba, full[3][index])
        assert np.array_equal(bits(verts), bits(full[0][index]))
    verts, nrm, tris, index, rgba, stats = vol.extract_clean_mesh(9, colors=True, stats=True)
    assert stats[1] == 3 and rgba.shape == (len(verts), 4)
    vol.close()
