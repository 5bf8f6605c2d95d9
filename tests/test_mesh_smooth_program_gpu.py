"""The smoothing switches of the programs on the GPU: bin/MeshOutput --smooth against TSDFVolume.LoadWorld + SaveMesh(smooth=...)
byte for byte, alone and with the cleaning and clustering switches; bin/Integrate --save_mesh --mesh_smooth against the Python mirror, alone,
with the other switches and with colour; and, without the switch, the file of before."""
import os
import subprocess

import numpy as np
import pytest

import mesh_smooth_restatement as rs
from elasticreconstruction_amd import formats, synth
from elasticreconstruction_amd.tsdf import IntegrateApp
from test_mesh_clean_program_gpu import mesh_output, read, world  # noqa: F401  (the fixture: two units with a ball and planted voxels)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elasticreconstruction_amd", "bin")
CELL = "0.01171875"                                                              # 2 voxels, exact in float32


@pytest.mark.parametrize("flags,kw", [(["--smooth", "10"], dict(smooth=10)),
                                      (["--smooth", "3", "--smooth_lambda", "0.75", "--smooth_mu", "0", "--min_triangles", "9"], dict(smooth=3, smooth_lambda=0.75, smooth_mu=0.0, min_triangles=9)),
                                      (["--smooth", "2", "--smooth_fix_boundary", "--largest_only", "--ascii"], dict(smooth=2, smooth_fix_boundary=True, largest_only=True, binary=False)),
                                      (["--smooth", "4", "--cell", CELL, "--no_normals"], dict(smooth=4, cell=float(CELL), normals=False)),
                                      (["--smooth", "4", "--smooth_mu", "-0.5", "--cell", CELL, "--min_triangles", "8"], dict(smooth=4, smooth_mu=-0.5, cell=float(CELL), min_triangles=8))],
                         ids=["alone", "laplacian, min_triangles 9", "boundary fixed, largest_only, ascii", "cell, no normals", "mu, cell, min_triangles 8"])
def test_mesh_output_with_smoothing_equals_the_python_route(world, flags, kw):
    d, vol = world["d"], world["vol"]
    tag = "smooth_" + "_".join(f.strip("-") for f in flags if f.startswith("--"))
    r = mesh_output(d, "mo_%s.ply" % tag, *flags)
    n, m = vol.SaveMesh(os.path.join(d, "py_%s.ply" % tag), **kw)
    assert read(d, "mo_%s.ply" % tag) == read(d, "py_%s.ply" % tag)
    assert "%d iterations of lambda" % kw["smooth"] in r.stdout and "%d vertices, %d triangles" % (n, m) in r.stdout, r.stdout
    assert "er_tsdf_extract_mesh_smoothed" in r.stderr + r.stdout               # ER_TIMING's line of the stage
    if "cell" not in kw:
        v, t, _ = formats.load_ply(os.path.join(d, "mo_%s.ply" % tag))
        src = vol.extract_clean_mesh(kw.get("min_triangles", 0), kw.get("largest_only", False))
        want = rs.smooth(src[0], src[2], kw["smooth"], kw.get("smooth_lambda", 0.5), kw.get("smooth_mu", -0.53), kw.get("smooth_fix_boundary", False))
        assert n == len(src[0]) and np.array_equal(t, src[2])
        if kw.get("binary", True):
            assert np.array_equal(v.view(np.uint32), want["verts"][:, :3].view(np.uint32))


def test_mesh_output_without_the_switch_writes_the_file_of_before(world):
    d, vol = world["d"], world["vol"]
    mesh_output(d, "mo_nosmooth.ply")
    mesh_output(d, "mo_smooth0.ply", "--smooth", "0")                            # no iteration: the stage is skipped
    vol.SaveMesh(os.path.join(d, "py_smooth0.ply"), smooth=0)
    vol.SaveMesh(os.path.join(d, "py_before.ply"))
    assert read(d, "mo_nosmooth.ply") == read(d, "mo_smooth0.ply") == read(d, "py_smooth0.ply") == read(d, "py_before.ply")
    mesh_output(d, "mo_cell.ply", "--cell", CELL)
    mesh_output(d, "mo_cell_smooth0.ply", "--cell", CELL, "--smooth", "0")
    assert read(d, "mo_cell.ply") == read(d, "mo_cell_smooth0.ply")
    for bad in (["--smooth", "-3"], ["--smooth", "2", "--smooth_mu", "1.01"]):
        r = subprocess.run([os.path.join(BIN, "MeshOutput"), "world.pcd", "--save_to", "bad.ply"] + bad, cwd=d, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "--smooth" in r.stderr and not os.path.exists(os.path.join(d, "bad.ply")), (bad, r.stderr)


def test_integrate_save_mesh_with_smoothing(gpu, tmp_path):
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
    r = subprocess.run(args + ["--mesh_smooth", "3"], cwd=d, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--mesh_smooth needs --save_mesh" in r.stderr and not os.path.exists(os.path.join(d, "world.pcd")), r.stderr
    runs = {"plain": ["--mesh_smooth", "5"], "clean": ["--mesh_smooth", "2", "--mesh_smooth_fix_boundary", "--mesh_largest_only"],
            "colour": ["--mesh_smooth", "5", "--color_raw", "colour.raw"],
            "all": ["--mesh_smooth", "3", "--mesh_smooth_lambda", "0.6", "--mesh_smooth_mu", "-0.6", "--color_raw", "colour.raw", "--mesh_min_triangles", "50", "--mesh_cell", CELL],
            "none": [], "none_colour": ["--color_raw", "colour.raw"]}
    out = {}
    for tag, flags in runs.items():
        r = subprocess.run(args + ["--save_mesh", "m_%s.ply" % tag] + flags, cwd=d, capture_output=True, text=True, timeout=300, env=dict(os.environ, ER_TIMING="1"))
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("mesh smoothed with" in r.stdout) == ("--mesh_smooth" in flags) == ("er_tsdf_extract_mesh_smoothed" in r.stderr + r.stdout), r.stdout
        out[tag] = r.stdout
    mirror = {"plain": dict(smooth=5), "clean": dict(smooth=2, smooth_fix_boundary=True, largest_only=True), "colour": dict(smooth=5),
              "all": dict(smooth=3, smooth_lambda=0.6, smooth_mu=-0.6, min_triangles=50, cell=float(CELL)), "none": {}, "none_colour": {}}
    for colour in (False, True):
        app = IntegrateApp(max_units=512)
        app.traj_filename_ = os.path.join(d, "traj.log")
        app.Init()
        for f in range(3):
            app.Execute(f + 1, depth[f], rgb[f] if colour else None)
        app.Flush()
        vol = app.volume_
        for tag in (("colour", "all", "none_colour") if colour else ("plain", "clean", "none")):
            n, m = vol.SaveMesh(os.path.join(d, "py_%s.ply" % tag), **mirror[tag])
            assert read(d, "m_%s.ply" % tag) == read(d, "py_%s.ply" % tag), tag
            assert "%d mesh vertices and %d triangles have been written." % (n, m) in out[tag] and n > 1000
        if colour:
            # the colours travel by vertex index: those of the unsmoothed mesh
            c = formats.load_ply_colors(os.path.join(d, "m_colour.ply"))[3]
            assert c is not None and np.array_equal(c[:, :3], vol.extract_indexed_mesh(colors=True)[3][:, :3])
        else:
            v, t, _ = formats.load_ply(os.path.join(d, "m_plain.ply"))
            src = vol.extract_indexed_mesh()
            assert np.array_equal(v.view(np.uint32), rs.smooth(src[0], src[2], 5)["verts"][:, :3].view(np.uint32)) and np.array_equal(t, src[2])
        vol.close()
