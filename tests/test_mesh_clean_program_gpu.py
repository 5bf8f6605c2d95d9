"""The mesh cleaning flags of the programs on the GPU: bin/MeshOutput --min_triangles / --largest_only against TSDFVolume.LoadWorld +
SaveMesh(min_triangles, largest_only) byte for byte, and without the flags the file of today; bin/Integrate --save_mesh with the flags against
the Python mirror, and its refusal of the flags without --save_mesh."""
import os
import subprocess

import numpy as np
import pytest

import mesh_components_cases as cases
from elasticreconstruction_amd import formats, synth
from elasticreconstruction_amd.tsdf import TSDFVolume
from mesh_components_restatement import components
from test_oriented_gpu import volume_from_units

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elasticreconstruction_amd", "bin")


@pytest.fixture(scope="module")
def world(gpu, tmp_path_factory):
    """world.pcd of two units of observed space at sdf 0.9 (SaveWorld keeps it: |sdf| < 0.98) that hold a ball of 8 voxels' radius, two
    single voxels, a pair across the unit border and a voxel at the face of the lattice of units."""
    d = str(tmp_path_factory.mktemp("mesh_clean"))
    i, j, k = np.meshgrid(np.arange(64), np.arange(64), np.arange(64), indexing="ij")
    units = {}
    for key in (cases.KEY, cases.KEY + cases.DX):
        units[key] = (np.full(64 ** 3, 0.9, np.float32), np.ones(64 ** 3, np.float32))
    ball = np.clip((np.sqrt((i - 30.0) ** 2 + (j - 31.0) ** 2 + (k - 32.0) ** 2) - 8.0) / 5.0, -0.9, 0.9).astype(np.float32)
    units[cases.KEY] = (ball.reshape(-1).copy(), units[cases.KEY][1])
    cases.plant(units, cases.KEY, [(5, 5, 5), (50, 6, 7), (63, 50, 50), (0, 20, 20)])
    cases.plant(units, cases.KEY + cases.DX, [(0, 50, 50), (40, 40, 40)])
    vol = volume_from_units(units)
    vol.SaveWorld(os.path.join(d, "world.pcd"))
    vol.close()
    B = TSDFVolume(max_units=4)
    B.LoadWorld(os.path.join(d, "world.pcd"))
    yield dict(d=d, vol=B)
    B.close()


def read(d, name):
    return open(os.path.join(d, name), "rb").read()


def mesh_output(d, out, *flags):
    r = subprocess.run([os.path.join(BIN, "MeshOutput"), "world.pcd", "--save_to", out] + list(flags), cwd=d, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ER_TIMING="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_the_world_holds_what_the_flags_are_to_drop(world):
    verts, _, tris = world["vol"].extract_indexed_mesh()
    labels, counts, n = components(tris, len(verts))
    sizes = sorted(counts[labels == np.arange(len(verts))].tolist())
    assert sizes[:-1] == [4, 8, 8, 8, 16] and sizes[-1] > 500, sizes


@pytest.mark.parametrize("flags,kw,kept", [(["--min_triangles", "9"], dict(min_triangles=9), 2), (["--largest_only"], dict(largest_only=True), 1),
                                           (["--min_triangles", "5", "--largest_only", "--ascii"], dict(min_triangles=5, largest_only=True, binary=False), 1),
                                           (["--min_triangles", "8", "--no_normals"], dict(min_triangles=8, normals=False), 5)],
                         ids=["min_triangles 9", "largest_only", "both, ascii", "min_triangles 8, no normals"])
def test_mesh_output_with_the_cleaning_flags_equals_the_python_route(world, flags, kw, kept):
    d, vol = world["d"], world["vol"]
    tag = "_".join(f.strip("-") for f in flags)
    r = mesh_output(d, "mo_%s.ply" % tag, *flags)
    n, m = vol.SaveMesh(os.path.join(d, "py_%s.ply" % tag), **kw)
    assert read(d, "mo_%s.ply" % tag) == read(d, "py_%s.ply" % tag)
    assert "%d vertices, %d triangles" % (n, m) in r.stdout and "%d of 6 components kept" % kept in r.stdout, r.stdout
    assert "er_tsdf_extract_mesh_cleaned" in r.stderr + r.stdout                 # ER_TIMING's line of the cleaning stage
    v, t, _ = formats.load_ply(os.path.join(d, "mo_%s.ply" % tag))
    got = vol.extract_clean_mesh(kw.get("min_triangles", 0), kw.get("largest_only", False))
    assert np.array_equal(v.view(np.uint32), got[0][:, :3].view(np.uint32)) and np.array_equal(t, got[2])


def test_mesh_output_without_the_flags_writes_the_unfiltered_mesh(world):
    d, vol = world["d"], world["vol"]
    r = mesh_output(d, "mo_plain.ply")
    n, m = vol.SaveMesh(os.path.join(d, "py_plain.ply"))
    assert read(d, "mo_plain.ply") == read(d, "py_plain.ply") and "components kept" not in r.stdout
    mesh_output(d, "mo_one.ply", "--min_triangles", "1")                          # 0 and 1 keep everything
    assert read(d, "mo_one.ply") == read(d, "py_plain.ply")
    v, t, _ = formats.load_ply(os.path.join(d, "mo_plain.ply"))
    verts, _, tris = vol.extract_indexed_mesh()
    assert np.array_equal(v.view(np.uint32), verts[:, :3].view(np.uint32)) and np.array_equal(t, tris)
    r = subprocess.run([os.path.join(BIN, "MeshOutput"), "world.pcd", "--min_triangles", "-2"], cwd=d, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--min_triangles" in r.stderr and not os.path.exists(os.path.join(d, "mesh.ply"))


def test_integrate_save_mesh_with_the_cleaning_flags(gpu, tmp_path):
    d = str(tmp_path)
    W = synth.kinfu_camera_path(3, 50, 50)[::20]
    F = W[0] @ np.linalg.inv(synth.basepose())
    seg = [np.linalg.inv(F) @ w for w in W]
    depth = synth.to_numpy_u16(synth.render_depth(W))
    formats.save_log(os.path.join(d, "traj.log"), [formats.FramedTransformation(i, i, i + 1, seg[min(i, 2)]) for i in range(4)])
    depth.tofile(os.path.join(d, "frames.raw"))
    args = [os.path.join(BIN, "Integrate"), "--ref_traj", "traj.log", "-oni", "frames.raw", "--max_units", "512"]
    for flags in (["--mesh_min_triangles", "9"], ["--mesh_largest_only"]):
        r = subprocess.run(args + flags, cwd=d, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "need --save_mesh" in r.stderr and not os.path.exists(os.path.join(d, "world.pcd")), r.stderr
    r = subprocess.run(args + ["--save_mesh", "m.ply", "--mesh_largest_only", "--mesh_min_triangles", "100"], cwd=d, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    logged = formats.load_log(os.path.join(d, "traj.log"))
    vol = TSDFVolume(max_units=512)
    vol.IntegrateFrames(depth, np.stack([logged[f].T for f in range(3)]))
    n, m = vol.SaveMesh(os.path.join(d, "m_py.ply"), min_triangles=100, largest_only=True)
    full = vol.extract_indexed_mesh()
    vol.close()
    assert read(d, "m.ply") == read(d, "m_py.ply") and 100 <= m <= len(full[2])
    assert "%d mesh vertices and %d triangles have been written." % (n, m) in r.stdout and "mesh components kept" in r.stdout
