"""The mesh output stage (er_tsdf_extract_mesh_indexed, er_tsdf_import_world, PLY, bin/MeshOutput), the part that needs no GPU: the numpy
restatement of the indexed mesh (tests/mesh_restatement.py) on hand-made volumes with known answers and against test_tsdf_gpu._mesh_oracle,
the PLY writers of formats.py and csrc/host/er_formats.h, the new symbols, and the program's behaviour without work to do."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from elasticreconstruction_amd import _ffi, formats
from mesh_restatement import UL, crossed_observed_edges, indexed_mesh
from test_oriented_gpu import hand_made_units
from test_tsdf_gpu import _mesh_oracle, _surface_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elasticreconstruction_amd", "bin")
KEY = 256 << 18 | 256 << 9 | 256                    # the unit whose voxel (0, 0, 0) sits at the origin
BLOCKS = [("middle", (256, 255, 300)), ("far corner", (510, 510, 510)), ("near corner", (0, 0, 0))]


def one_unit(voxels):
    """{KEY: (sdf, weight)} with the given {(i, j, k): sdf} observed (weight 1) and nothing else."""
    sdf, w = np.zeros((64, 64, 64), np.float32), np.zeros((64, 64, 64), np.float32)
    for (i, j, k), s in voxels.items():
        sdf[i, j, k], w[i, j, k] = s, 1.0
    return {KEY: (sdf.reshape(-1), w.reshape(-1))}


def pos(*g):
    return (np.array(g, np.float64) * UL).astype(np.float32)


def test_one_cell_with_one_negative_corner_gives_three_vertices_and_one_triangle():
    cell = {(10 + a, 20 + b, 30 + c): 0.5 for a in range(2) for b in range(2) for c in range(2)}
    cell[(10, 20, 30)] = -0.5
    verts, tris, _ = indexed_mesh(one_unit(cell))
    half = np.float32(np.float32(-0.5) / np.float32(-1.0)) * np.float32(UL)           # F_L / (F_L - F_H) * voxel size
    p = pos(10, 20, 30)
    want = np.array([[p[0] + half, p[1], p[2], 0], [p[0], p[1] + half, p[2], 1], [p[0], p[1], p[2] + half, 2]], np.float32)
    assert verts.shape == (3, 4) and np.array_equal(verts.view(np.uint32), want.view(np.uint32)), verts
    assert tris.shape == (1, 3) and tris.dtype == np.int32 and sorted(tris[0]) == [0, 1, 2]
    # the triangle faces the free space: away from the negative corner
    a, b, c = (verts[q, :3].astype(np.float64) for q in tris[0])
    assert np.dot(np.cross(b - a, c - a), np.ones(3)) > 0
    assert np.array_equal(verts[tris][..., :3].view(np.uint32), _mesh_oracle(one_unit(cell)).view(np.uint32))


def test_a_cell_with_an_unobserved_corner_gives_nothing_although_its_edges_are_crossed():
    cell = {(10 + a, 20 + b, 30 + c): 0.5 for a in range(2) for b in range(2) for c in range(2)}
    cell[(10, 20, 30)] = -0.5
    del cell[(11, 21, 31)]
    units = one_unit(cell)
    verts, tris, codes = indexed_mesh(units)
    assert verts.shape == (0, 4) and tris.shape == (0, 3) and codes.size == 0
    assert _surface_oracle(units).shape == (3, 4)                                    # the surface list needs no complete cell
    assert crossed_observed_edges(units).size == 3


def test_a_zero_voxel_between_negative_neighbours_gives_coincident_positions_under_distinct_indices():
    slab = {(10 + a, 20 + b, 30 + c): (0.0 if a == 1 else -0.5) for a in range(3) for b in range(2) for c in range(2)}
    verts, tris, codes = indexed_mesh(one_unit(slab))
    # sdf == 0 is outside: the four edges 10 -> 11 (t = 1) and the four edges 11 -> 12 (t = 0) are crossed, all eight meet at i = 11
    assert verts.shape == (8, 4) and (verts[:, 3] == 0).all() and len(np.unique(codes)) == 8
    want = np.array([pos(11, 20 + b, 30 + c) for b in range(2) for c in range(2)], np.float32)
    assert np.array_equal(verts[:4, :3].view(np.uint32), want.view(np.uint32))       # lower voxel i = 10: pos(10) + 1 * voxel
    assert np.array_equal(verts[4:, :3].view(np.uint32), want.view(np.uint32))       # lower voxel i = 11: pos(11) + 0
    assert len(np.unique(verts[:, :3].view(np.uint32), axis=0)) == 4
    assert tris.shape == (4, 3) and sorted(np.unique(tris)) == list(range(8))        # two quads, each on its own four vertices
    assert not set(tris[:2].reshape(-1)) & set(tris[2:].reshape(-1))


@pytest.fixture(scope="module", params=BLOCKS, ids=[b[0] for b in BLOCKS])
def block(request):
    name, base = request.param
    units = hand_made_units(1234 + base[0], base, holes=0.2)
    return name, units, indexed_mesh(units)


def test_the_restatements_soup_is_the_soup_oracles(block):
    name, units, (verts, tris, codes) = block
    want = _mesh_oracle(units)
    got = verts[tris][..., :3]
    assert got.shape == want.shape and got.shape[0] > 100000, (name, got.shape, want.shape)
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.unique(tris), np.arange(len(verts)))                    # every vertex is referenced
    assert (np.diff(codes) > 0).all()


def test_mesh_vertices_are_a_proper_share_of_the_crossed_observed_edges(block):
    """Both kinds of crossed, observed edges are well represented in the fixtures: those a complete cell makes a vertex, and those no
    complete cell touches (with holes = 0.2 about 63 % / 37 %; at 0.1 it would be 90 % / 10 %)."""
    name, units, (verts, tris, codes) = block
    edges = crossed_observed_edges(units)
    assert np.isin(codes, edges).all(), "a mesh vertex is not a crossed, observed edge"
    share = len(codes) / len(edges)
    print("%s: %d crossed observed edges, %.1f %% of them mesh vertices" % (name, len(edges), 100 * share))
    assert share >= 0.10 and 1.0 - share >= 0.10, share


# ---- PLY ------------------------------------------------------------------------------------------------------------------------------

def small_mesh():
    rng = np.random.default_rng(7)
    verts = np.concatenate([rng.normal(size=(9, 3)), rng.integers(0, 3, (9, 1))], 1).astype(np.float32)
    verts[0, :3] = [-0.0, 1.0e-30, 123456.789]
    nrm = rng.normal(size=(9, 3)).astype(np.float32)
    nrm[2] = np.nan
    nrm[5, 1] = np.nan
    tris = rng.integers(0, 9, (5, 3)).astype(np.int32)
    return verts, nrm, tris


def ply_header(n, m, normals, binary):
    lines = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "element vertex %d" % n,
             "property float x", "property float y", "property float z"]
    if normals:
        lines += ["property float nx", "property float ny", "property float nz"]
    lines += ["element face %d" % m, "property list uchar int vertex_indices", "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


@pytest.fixture(scope="module")
def ply_check():
    src = os.path.join(ROOT, "tests", "hostcheck", "ply_check.cpp")
    out = os.path.join(ROOT, "tests", "hostcheck", "_build", "ply_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    hdr = os.path.join(ROOT, "elasticreconstruction_amd", "csrc", "host", "er_formats.h")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", out, "-lz"], check=True)
    return out


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "ascii"])
@pytest.mark.parametrize("with_normals", [True, False], ids=["normals", "no normals"])
def test_ply_round_trip_header_and_the_host_writers_bytes(tmp_path, ply_check, binary, with_normals):
    verts, nrm, tris = small_mesh()
    path = str(tmp_path / "m.ply")
    formats.save_ply(path, verts, tris, nrm if with_normals else None, binary=binary)
    raw = open(path, "rb").read()
    hdr = ply_header(9, 5, with_normals, binary)
    assert raw[:len(hdr)] == hdr, raw[:len(hdr) + 20]
    if binary:
        assert len(raw) == len(hdr) + 9 * 4 * (6 if with_normals else 3) + 5 * 13
    v, t, n = formats.load_ply(path)
    assert v.dtype == np.float32 and np.array_equal(v.view(np.uint32), verts[:, :3].view(np.uint32))     # %.9g carries a float32 exactly
    assert t.dtype == np.int32 and np.array_equal(t, tris)
    if with_normals:
        want = nrm.copy()
        want[[2, 5]] = 0.0                                                            # a normal with a NaN component: 0 0 0
        assert np.array_equal(n.view(np.uint32), want.view(np.uint32))
        assert not np.isnan(n).any() and np.isnan(nrm).any()                          # (the caller's array keeps its NaN)
    else:
        assert n is None
    # the same arrays through er_formats.h
    arrays = str(tmp_path / "arrays.bin")
    with open(arrays, "wb") as f:
        f.write(np.array([9, 5], np.int64).tobytes())
        f.write(verts.tobytes())
        f.write(np.concatenate([nrm, np.zeros((9, 1), np.float32)], 1).tobytes())
        f.write(tris.tobytes())
    other = str(tmp_path / "host.ply")
    subprocess.run([ply_check, arrays, other, "1" if binary else "0", "1" if with_normals else "0"], check=True, timeout=60)
    assert open(other, "rb").read() == raw


def test_ply_of_an_empty_mesh(tmp_path):
    path = str(tmp_path / "e.ply")
    formats.save_ply(path, np.zeros((0, 4), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32))
    assert open(path, "rb").read() == ply_header(0, 0, True, True)
    v, t, n = formats.load_ply(path)
    assert v.shape == (0, 3) and t.shape == (0, 3) and n.shape == (0, 3)


# ---- the ABI and the program ----------------------------------------------------------------------------------------------------------

def test_the_new_entry_points_are_declared_bound_exported_and_refuse_a_null_handle():
    header = open(os.path.join(ROOT, "include", "er_hip.h")).read()
    L = _ffi.lib()
    for name in ("er_tsdf_extract_mesh_indexed", "er_tsdf_import_world"):
        assert "int %s(" % name in header and name in _ffi.SYMBOLS and hasattr(L, name), name
    nv, nt, nu = C.c_long(-1), C.c_long(-1), C.c_int(-1)
    rc = L.er_tsdf_extract_mesh_indexed(None, None, None, 0, None, 0, C.byref(nv), C.byref(nt))
    assert rc != 0 and "er_tsdf_extract_mesh_indexed" in L.er_last_error().decode()
    rc = L.er_tsdf_import_world(None, None, 0, C.byref(nu))
    assert rc != 0 and "er_tsdf_import_world" in L.er_last_error().decode()


def test_mesh_output_prints_its_usage_and_names_a_missing_file(tmp_path):
    exe = os.path.join(BIN, "MeshOutput")
    for args in ([], ["--help"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
        assert r.returncode == 0 and "Usage: MeshOutput <world.pcd>" in r.stdout and "--save_to" in r.stdout, (r.returncode, r.stdout, r.stderr)
    r = subprocess.run([exe, "no_such_world.pcd"], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode != 0 and "no_such_world.pcd" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(str(tmp_path / "mesh.ply"))
