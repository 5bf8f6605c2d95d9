"""Mesh cleaning without a GPU: the numpy restatement of the definitions against scipy's connected components on every
index list the GPU tests use, the filter rule at its edges, the new symbols, the refusals that need no device, the programs' help texts, and
the facts about planted voxels that the GPU tests build their volumes on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import mesh_components_cases as cases
from elasticreconstruction_amd import _ffi
from mesh_components_restatement import clean, components, keep_vertices
from mesh_restatement import indexed_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NOT_A_HANDLE = C.create_string_buffer(4096)


def scipy_components(tris, nv):
    """scipy's components mapped to smallest-index labels, and triangles per component."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]]])
    g = coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(nv, nv))
    n, lab = connected_components(g, directed=False)
    first = np.full(n, nv, np.int64)
    np.minimum.at(first, lab, np.arange(nv))
    per = np.bincount(lab[tris[:, 0]], minlength=n) if len(tris) else np.zeros(n, np.int64)
    return first[lab].astype(np.int32), per[lab].astype(np.int64), n


@pytest.mark.parametrize("name", sorted(cases.index_lists()))
def test_restatement_equals_scipy_connected_components(name):
    tris, nv = cases.index_lists()[name]
    labels, counts, n = components(tris, nv)
    wl, wc, wn = scipy_components(tris, nv)
    assert labels.dtype == np.int32 and counts.dtype == np.int64
    assert np.array_equal(labels, wl) and np.array_equal(counts, wc) and n == wn, name
    if name.startswith("strip"):
        assert not labels.any() and n == 1 and (counts == cases.N_STRIP).all()
    if name.startswith("fan"):
        assert not labels.any() and (counts == 65536).all()


def test_restatement_on_the_small_lists_by_hand():
    tris, nv = cases.odd_triangles()
    labels, counts, n = components(tris, nv)
    assert labels.tolist() == [0, 1, 2, 1, 1, 5, 0, 5, 0, 5, 0, 5, 0, 13]
    assert counts.tolist() == [4, 3, 1, 3, 3, 3, 4, 3, 4, 3, 4, 3, 4, 0] and n == 5
    tris, nv = cases.unused_vertices()
    labels, counts, n = components(tris, nv)
    assert labels[0] == 0 and counts[0] == 0 and labels[599] == 599 and counts[599] == 0 and labels[299] == 299
    assert labels[[1, 2, 3, 4, 5, 300, 301, 302]].tolist() == [1] * 8 and counts[300] == 4
    assert labels[[596, 597, 598]].tolist() == [596] * 3 and n == 600 - 11 + 2
    tris, nv = cases.interleaved()
    labels, _, n = components(tris, nv)
    assert n == 2 and np.array_equal(labels, np.arange(nv) & 1)


def test_filter_rule_at_its_edges():
    # components: {0,1,2} 2 triangles, {3,4,5} 2 triangles, {6,7,8} 1 triangle, 9 isolated
    tris = np.array([[0, 1, 2], [5, 4, 3], [2, 1, 0], [6, 7, 8], [3, 4, 5]], np.int32)
    labels, counts, n = components(tris, 10)
    assert n == 4 and counts.tolist() == [2, 2, 2, 2, 2, 2, 1, 1, 1, 0]
    for m in (0, 1):                                         # 0 and 1 keep everything -- 0 also the isolated vertex
        assert keep_vertices(labels, counts, m, False).tolist() == [True] * 9 + [m == 0]
    assert keep_vertices(labels, counts, 2, False).tolist() == [True] * 6 + [False] * 4          # a count equal to min_triangles stays
    assert not keep_vertices(labels, counts, 3, False).any()
    assert keep_vertices(labels, counts, 0, True).tolist() == [True] * 3 + [False] * 7           # a tie for the largest: the smaller label
    assert keep_vertices(labels, counts, 2, True).tolist() == [True] * 3 + [False] * 7
    assert not keep_vertices(labels, counts, 3, True).any()                                      # largest_only below the threshold: empty
    index, out, stats = clean(tris, 10, 2, False)
    assert index.tolist() == [0, 1, 2, 3, 4, 5] and out.tolist() == [[0, 1, 2], [5, 4, 3], [2, 1, 0], [3, 4, 5]] and stats == (4, 2, 4, 1)
    index, out, stats = clean(tris, 10, 2, True)
    assert index.tolist() == [0, 1, 2] and out.tolist() == [[0, 1, 2], [2, 1, 0]] and stats == (4, 1, 7, 3)
    index, out, stats = clean(tris[[1, 3, 4]], 10, 2, False)                                     # the re-index: kept vertices before it
    assert index.tolist() == [3, 4, 5] and out.tolist() == [[2, 1, 0], [0, 1, 2]] and stats == (6, 1, 7, 1)
    index, out, stats = clean(tris, 10, 3, True)
    assert len(index) == 0 and out.shape == (0, 3) and stats == (4, 0, 10, 5)
    # isolated vertices only: with largest_only the largest is vertex 0, with 0 triangles
    index, out, stats = clean(np.zeros((0, 3), np.int32), 3, 0, True)
    assert index.tolist() == [0] and stats == (3, 1, 2, 0)


def test_new_symbols_are_in_the_header_the_binding_and_the_library():
    hdr = open(os.path.join(ROOT, "include", "er_hip.h")).read()
    L = _ffi.lib()
    for sym in ("er_mesh_components", "er_tsdf_extract_mesh_cleaned"):
        assert re.search(r"\bint %s\(" % sym, hdr) and sym in _ffi.SYMBOLS and hasattr(L, sym), sym
    from elasticreconstruction_amd import mesh
    from elasticreconstruction_amd.tsdf import TSDFVolume
    assert callable(mesh.components) and callable(TSDFVolume.extract_clean_mesh)


def test_refusals_that_need_no_device():
    L = _ffi.lib()
    err = lambda: L.er_last_error().decode()
    tri = np.array([[0, 1, 2]], np.int32)
    nc, nv, nt = C.c_long(-7), C.c_long(-7), C.c_long(-7)
    lab = np.full(3, -7, np.int32)
    assert L.er_mesh_components(_ffi.ptr(tri), 1, 3, 0, None, None, None, None) != 0 and err() == "er_mesh_components: NULL argument"
    assert L.er_mesh_components(None, 1, 3, 0, None, None, C.byref(nc), None) != 0 and err() == "er_mesh_components: NULL argument"
    assert L.er_mesh_components(_ffi.ptr(tri), -1, 3, 0, None, None, C.byref(nc), None) != 0 and "-1 triangles" in err()
    assert L.er_mesh_components(_ffi.ptr(tri), 1, -3, 0, None, None, C.byref(nc), None) != 0 and "-3 vertices" in err()
    assert L.er_mesh_components(_ffi.ptr(tri), 1, 2 ** 31, 0, None, None, C.byref(nc), None) != 0 and "2^31 - 1" in err()
    assert nc.value == -7
    fake = C.cast(_NOT_A_HANDLE, C.c_void_p)                 # never dereferenced: every call with it is refused before the handle is looked at
    call = lambda h, m, pv, pt: L.er_tsdf_extract_mesh_cleaned(h, m, 0, None, None, None, 0, None, 0, pv, pt, None)
    assert call(None, 0, C.byref(nv), C.byref(nt)) != 0 and err() == "er_tsdf_extract_mesh_cleaned: NULL argument"
    assert call(fake, 0, None, C.byref(nt)) != 0 and err() == "er_tsdf_extract_mesh_cleaned: NULL argument"
    assert call(fake, 0, C.byref(nv), None) != 0 and err() == "er_tsdf_extract_mesh_cleaned: NULL argument"
    assert call(fake, -1, C.byref(nv), C.byref(nt)) != 0 and err() == "er_tsdf_extract_mesh_cleaned: min_triangles = -1"
    assert (nv.value, nt.value) == (-7, -7)
    if L.er_device_count() <= 0:
        assert L.er_mesh_components(_ffi.ptr(tri), 1, 3, 0, _ffi.ptr(lab), None, C.byref(nc), None) != 0
        assert err() == "er_mesh_components: no HIP device available (liber_hip has no CPU fallback)"
        assert call(fake, 0, C.byref(nv), C.byref(nt)) != 0
        assert err() == "er_tsdf_extract_mesh_cleaned: no HIP device available (liber_hip has no CPU fallback)"
        assert nc.value == -7 and (lab == -7).all() and (nv.value, nt.value) == (-7, -7)
    else:
        assert L.er_mesh_components(_ffi.ptr(tri), 1, 3, 0, _ffi.ptr(lab), None, C.byref(nc), None) == 0 and nc.value == 1 and not lab.any()


def test_programs_name_the_new_flags_in_their_help():
    bin_ = os.path.join(ROOT, "elasticreconstruction_amd", "bin")
    r = subprocess.run([os.path.join(bin_, "MeshOutput"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--min_triangles" in r.stdout and "--largest_only" in r.stdout, r.stdout
    r = subprocess.run([os.path.join(bin_, "Integrate"), "--help"], capture_output=True, text=True, timeout=60)
    assert "--mesh_min_triangles" in r.stdout + r.stderr and "--mesh_largest_only" in r.stdout + r.stderr


def shells(units):
    """(triangles, vertices) of every component of the units' indexed mesh, largest first."""
    verts, tris, _ = indexed_mesh(units)
    labels, counts, n = components(tris, len(verts))
    roots = np.flatnonzero(labels == np.arange(len(verts)))
    assert len(roots) == n and np.array_equal(np.unique(tris), np.arange(len(verts)))
    return sorted(((int(counts[r]), int((labels == r).sum())) for r in roots), reverse=True)


@pytest.mark.parametrize("what,units,want", [
    ("one negative voxel", lambda: cases.planted([(20, 21, 22)]), [(8, 6)]),
    ("at a face of the lattice of existing units", lambda: cases.planted([(0, 21, 22)]), [(4, 5)]),
    ("at an edge", lambda: cases.planted([(0, 21, 0)]), [(2, 4)]),
    ("at a corner", lambda: cases.planted([(0, 0, 0)]), [(1, 3)]),
    ("two face-adjacent negative voxels", lambda: cases.planted([(20, 21, 22), (20, 22, 22)]), [(16, 10)]),
    ("two voxels across a face diagonal", lambda: cases.planted([(20, 21, 22), (21, 22, 22)]), [(8, 6), (8, 6)]),
    ("two voxels across a body diagonal", lambda: cases.planted([(20, 21, 22), (21, 22, 23)]), [(8, 6), (8, 6)]),
    ("voxel i = 63 with the +x unit present", lambda: cases.planted([(63, 21, 22)], True), [(8, 6)]),
    ("a pair across that border", lambda: cases.planted([(63, 21, 22)], True, [(0, 21, 22)]), [(16, 10)]),
], ids=lambda x: x if isinstance(x, str) else "")
def test_planted_voxels_give_the_shells_the_gpu_tests_rely_on(what, units, want):
    assert shells(units()) == want, what
