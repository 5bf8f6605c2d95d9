"""The simplification switches of the programs on the GPU: bin/MeshOutput --cell against TSDFVolume.LoadWorld +
SaveMesh(cell=...) byte for byte, alone and with the cleaning switches; bin/Integrate --save_mesh --mesh_cell against the Python mirror, alone,
with the cleaning switches and with colour; and the refusal of --mesh_cell without --save_mesh."""
import os
import subprocess

import numpy as np
import pytest

import mesh_simplify_restatement as rs
from elasticreconstruction_amd import formats, synth
from elasticreconstruction_amd.tsdf import IntegrateApp, TSDFVolume
from test_mesh_clean_program_gpu import mesh_output, read, world  # noqa: F401  (the fixture: two units with a ball and planted voxels)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elasticreconstruction_amd", "bin")
UL = 3.0 / 512.0
CELL = "0.01171875"                                                              # 2 voxels, exact in float32


@pytest.mark.parametrize("flags,kw", [([], {}), (["--min_triangles", "9"], dict(min_triangles=9)), (["--largest_only", "--ascii"], dict(largest_only=True, binary=False)),
                                      (["--min_triangles", "8", "--no_normals"], dict(min_triangles=8, normals=False))],
                         ids=["alone", "min_triangles 9", "largest_only, ascii", "min_triangles 8, no normals"])
def test_mesh_output_with_a_cell_equals_the_python_route(world, flags, kw):
    d, vol = world["d"], world["vol"]
    tag = "cell_" + "_".join(f.strip("-") for f in flags)
    r = mesh_output(d, "mo_%s.ply" % tag, "--cell", CELL, *flags)
    n, m = vol.SaveMesh(os.path.join(d, "py_%s.ply" % tag), cell=float(CELL), **kw)
    assert read(d, "mo_%s.ply" % tag) == read(d, "py_%s.ply" % tag)
    assert "-> %d vertices and %d triangles" % (n, m) in r.stdout and "%d vertices, %d triangles" % (n, m) in r.stdout, r.stdout
    assert "er_tsdf_extract_mesh_simplified" in r.stderr + r.stdout             # ER_TIMING's line of the stage
    v, t, _ = formats.load_ply(os.path.join(d, "mo_%s.ply" % tag))
    src = vol.extract_clean_mesh(kw.get("min_triangles", 0), kw.get("largest_only", False))
    want = rs.simplify(src[0], src[2], float(CELL), src[1])
    assert 0 < n < len(src[0]) and np.array_equal(v.view(np.uint32), want["verts"][:, :3].view(np.uint32)) and np.array_equal(t, want["tris"])


def test_mesh_output_refuses_a_bad_cell_and_leaves_the_plain_file_alone(world):
    d, vol = world["d"], world["vol"]
    for bad in ("0", "-0.01", "inf", "1e40", "0.01x"):
        r = subprocess.run([os.path.join(BIN, "MeshOutput"), "world.pcd", "--save_to", "bad.ply", "--cell", bad], cwd=d, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "--cell" in r.stderr and not os.path.exists(os.path.join(d, "bad.ply")), (bad, r.stderr)
    mesh_output(d, "mo_nocell.ply")
    vol.SaveMesh(os.path.join(d, "py_nocell.ply"), cell=0.0)                      # cell == 0 takes the route of before
    vol.SaveMesh(os.path.join(d, "py_before.ply"))
    assert read(d, "mo_nocell.ply") == read(d, "py_nocell.ply") == read(d, "py_before.ply")


def test_integrate_save_mesh_with_a_cell(gpu, tmp_path):
    d = str(tmp_path)
    W = synth.kinfu_camera_path(3, 50, 50)[::20]
    F = W[0] @ np.linalg.inv(synth.basepose())
    seg = [np.linalg.inv(F) @ w for w in W]
    dt, ct = synth.render_rgbd(W)
    depth, rgb = synth.to_numpy_u16(dt), ct.numpy()
    formats.save_log(os.path.join(d, "traj.log"), [formats.FramedTransformation(i, i, i + 1, seg[min(i, 2)]) for i in range(4)])
    depth.tofile(os.path.join(d, "frames.raw"))
    rgb.tofile(os.path.join(d, "colour.raw"))
    args = [os.path.join(BIN, "Integrate"), "--ref_traj", "traj.log", "-oni", "frames.raw", "--max_units", "512"]
    r = subprocess.run(args + ["--mesh_cell", CELL], cwd=d, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--mesh_cell needs --save_mesh" in r.stderr and not os.path.exists(os.path.join(d, "world.pcd")), r.stderr
    r = subprocess.run(args + ["--save_mesh", "bad.ply", "--mesh_cell", "-1"], cwd=d, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--mesh_cell" in r.stderr and not os.path.exists(os.path.join(d, "bad.ply")), r.stderr
    runs = {"plain": [], "clean": ["--mesh_largest_only", "--mesh_min_triangles", "100"], "colour": ["--color_raw", "colour.raw"],
            "all": ["--color_raw", "colour.raw", "--mesh_min_triangles", "50"]}
    out = {}
    for tag, flags in runs.items():
        r = subprocess.run(args + ["--save_mesh", "m_%s.ply" % tag, "--mesh_cell", CELL] + flags, cwd=d, capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, ER_TIMING="1"))
        assert r.returncode == 0, r.stdout + r.stderr
        assert "mesh simplified with cells of 0.0117188 m" in r.stdout and "er_tsdf_extract_mesh_simplified" in r.stderr + r.stdout, r.stdout
        out[tag] = r.stdout
    # the Python mirror: one volume without colour, one with
    for colour in (False, True):
        app = IntegrateApp(max_units=512)
        app.traj_filename_ = os.path.join(d, "traj.log")
        app.Init()
        for f in range(3):
            app.Execute(f + 1, depth[f], rgb[f] if colour else None)
        app.Flush()
        vol = app.volume_
        for tag, kw in ((("colour", {}), ("all", dict(min_triangles=50))) if colour else (("plain", {}), ("clean", dict(min_triangles=100, largest_only=True)))):
            n, m = vol.SaveMesh(os.path.join(d, "py_%s.ply" % tag), cell=float(CELL), **kw)
            assert read(d, "m_%s.ply" % tag) == read(d, "py_%s.ply" % tag), tag
            assert "%d mesh vertices and %d triangles have been written." % (n, m) in out[tag] and n > 1000
        if colour:
            c = formats.load_ply_colors(os.path.join(d, "m_colour.ply"))[3]
            assert c is not None and (c[:, 3] == 255).mean() > 0.9 and len(np.unique(c[:, :3])) > 50
        else:
            assert len(vol.extract_indexed_mesh()[0]) > 2 * n
        vol.close()
