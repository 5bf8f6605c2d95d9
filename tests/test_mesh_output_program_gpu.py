"""The programs of the mesh output stage on the GPU: bin/MeshOutput (world.pcd in, PLY out) against TSDFVolume.LoadWorld + SaveMesh, and
bin/Integrate --save_mesh against TSDFVolume.SaveMesh after the same frames."""
import os
import subprocess

import numpy as np
import pytest

from elasticreconstruction_amd import formats, synth
from elasticreconstruction_amd.tsdf import TSDFVolume

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elasticreconstruction_amd", "bin")


@pytest.fixture(scope="module")
def run(gpu, tmp_path_factory):
    """Three frames of one sweep through bin/Integrate, with and without --save_mesh, and through the Python mirror."""
    d = str(tmp_path_factory.mktemp("mesh_output"))
    W = synth.kinfu_camera_path(3, 50, 50)[::20]
    F = W[0] @ np.linalg.inv(synth.basepose())
    seg = [np.linalg.inv(F) @ w for w in W]
    depth = synth.to_numpy_u16(synth.render_depth(W))
    formats.save_log(os.path.join(d, "traj.log"), [formats.FramedTransformation(i, i, i + 1, seg[min(i, 2)]) for i in range(4)])
    depth.tofile(os.path.join(d, "frames.raw"))
    args = [os.path.join(BIN, "Integrate"), "--ref_traj", "traj.log", "-oni", "frames.raw", "--max_units", "512"]
    r0 = subprocess.run(args + ["--save_to", "w0.pcd"], cwd=d, capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    r1 = subprocess.run(args + ["--save_to", "w1.pcd", "--save_mesh", "m.ply"], cwd=d, capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stdout + r1.stderr
    logged = formats.load_log(os.path.join(d, "traj.log"))
    vol = TSDFVolume(max_units=512)
    vol.IntegrateFrames(depth, np.stack([logged[f].T for f in range(3)]))
    yield dict(d=d, r0=r0, r1=r1, vol=vol)
    vol.close()


def read(d, name):
    return open(os.path.join(d, name), "rb").read()


def test_integrate_save_mesh_equals_the_python_mirror_and_leaves_world_pcd_alone(run):
    d, vol = run["d"], run["vol"]
    n, m = vol.SaveMesh(os.path.join(d, "m_py.ply"))
    assert n > 10000 and m > 20000
    assert read(d, "m.ply") == read(d, "m_py.ply")
    assert read(d, "w0.pcd") == read(d, "w1.pcd")
    assert "%d mesh vertices and %d triangles have been written." % (n, m) in run["r1"].stdout
    assert [l for l in run["r1"].stdout.splitlines() if "mesh vertices and" not in l] == run["r0"].stdout.splitlines()    # one more line, nothing else
    v, t, nr = formats.load_ply(os.path.join(d, "m.ply"))
    verts, nrm, tris = vol.extract_indexed_mesh()
    assert np.array_equal(v.view(np.uint32), verts[:, :3].view(np.uint32)) and np.array_equal(t, tris)
    assert np.array_equal(nr.view(np.uint32), np.where(np.isnan(nrm).any(1)[:, None], np.float32(0), nrm).view(np.uint32))
    r2 = subprocess.run([os.path.join(BIN, "Integrate"), "--ref_traj", "traj.log", "-oni", "frames.raw", "--save_to", "w2.pcd", "--save_mesh", "m2.ply",
                         "--gpus", "2", "--same_device"], cwd=d, capture_output=True, text=True, timeout=300)
    assert r2.returncode != 0 and "--save_mesh" in r2.stderr and "--gpus" in r2.stderr, r2.stderr
    assert not os.path.exists(os.path.join(d, "w2.pcd")) and not os.path.exists(os.path.join(d, "m2.ply"))


@pytest.mark.parametrize("flags,kw", [([], {}), (["--ascii"], dict(binary=False)), (["--no_normals"], dict(normals=False))],
                         ids=["binary", "ascii", "no normals"])
def test_mesh_output_equals_load_world_and_save_mesh(run, flags, kw):
    d = run["d"]
    tag = "_".join(f.strip("-") for f in flags) or "binary"
    r = subprocess.run([os.path.join(BIN, "MeshOutput"), "w0.pcd", "--save_to", "mo_%s.ply" % tag] + flags, cwd=d, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    B = TSDFVolume(max_units=512)
    B.LoadWorld(os.path.join(d, "w0.pcd"))
    n, m = B.SaveMesh(os.path.join(d, "py_%s.ply" % tag), **kw)
    B.close()
    assert n > 10000 and m > 20000 and "%d vertices, %d triangles" % (n, m) in r.stdout, r.stdout
    assert read(d, "mo_%s.ply" % tag) == read(d, "py_%s.ply" % tag)


def test_mesh_output_reports_a_refusal(run, tmp_path):
    rows = np.array([[0, 0, 0, 0.1], [0.5, 0, 0, 0.1]], np.float32)
    formats.save_pcd_xyzi(str(tmp_path / "bad.pcd"), rows)
    r = subprocess.run([os.path.join(BIN, "MeshOutput"), "bad.pcd"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "er_tsdf_import_world: row 1" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(str(tmp_path / "mesh.ply"))
