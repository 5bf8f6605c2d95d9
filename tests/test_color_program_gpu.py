"""bin/Integrate with a colour stream (--color_raw, --color_list), rigid and with --ctr, against the Python route (IntegrateApp.Execute with
colour, TSDFVolume.SaveMesh): the coloured PLY must match byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from elasticreconstruction_amd import formats, synth
from elasticreconstruction_amd.tsdf import IntegrateApp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elasticreconstruction_amd", "bin")


def read(d, name):
    return open(os.path.join(d, name), "rb").read()


def python_route(d, n, depth, rgb, out, **files):
    app = IntegrateApp(max_units=512)
    for k, v in files.items():
        setattr(app, k, os.path.join(d, v) if isinstance(v, str) else v)
    app.Init()
    for f in range(n):
        app.Execute(f + 1, depth[f], rgb[f])
    app.Flush()
    nv, nt = app.volume_.SaveMesh(os.path.join(d, out))
    col = app.volume_.extract_indexed_mesh(colors=True)[3]
    app.volume_.close()
    return nv, nt, col


def test_rigid_frames_with_raw_and_with_png_colour(gpu, tmp_path):
    from PIL import Image
    d = str(tmp_path)
    W = synth.kinfu_camera_path(3, 50, 50)[::20]
    F = W[0] @ np.linalg.inv(synth.basepose())
    seg = [np.linalg.inv(F) @ w for w in W]
    dt, ct = synth.render_rgbd(W)
    depth, rgb = synth.to_numpy_u16(dt), ct.numpy()
    # the texture lives in world coordinates, the volume in the fragment's: the colours are the same, only where they sit differs
    formats.save_log(os.path.join(d, "traj.log"), [formats.FramedTransformation(i, i, i + 1, seg[min(i, 2)]) for i in range(4)])
    depth.tofile(os.path.join(d, "frames.raw"))
    rgb.tofile(os.path.join(d, "colour.raw"))
    with open(os.path.join(d, "colour.txt"), "w") as f:
        for i in range(3):
            img = rgb[i].reshape(480, 640, 3)
            if i == 1:                                                                 # one of them RGBA
                Image.fromarray(np.concatenate([img, np.full((480, 640, 1), 200, np.uint8)], -1), "RGBA").save(os.path.join(d, "c1.png"))
            else:
                Image.fromarray(img, "RGB").save(os.path.join(d, "c%d.png" % i))
            f.write("c%d.png\n" % i)
    args = [os.path.join(BIN, "Integrate"), "--ref_traj", "traj.log", "-oni", "frames.raw", "--max_units", "512"]
    plain = subprocess.run(args + ["--save_to", "w0.pcd", "--save_mesh", "m0.ply"], cwd=d, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    for tag, src in (("raw", ["--color_raw", "colour.raw"]), ("png", ["--color_list", "colour.txt"])):
        r = subprocess.run(args + src + ["--save_to", "w_%s.pcd" % tag, "--save_mesh", "m_%s.ply" % tag], cwd=d, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "left without colour." in r.stdout
    nv, nt, col = python_route(d, 3, depth, rgb, "m_py.ply", traj_filename_="traj.log")
    assert nv > 10000 and nt > 20000
    assert read(d, "m_raw.ply") == read(d, "m_py.ply") and read(d, "m_png.ply") == read(d, "m_py.ply")
    assert read(d, "w_raw.pcd") == read(d, "w0.pcd") and read(d, "w_png.pcd") == read(d, "w0.pcd")    # colour leaves world.pcd alone
    v, t, n, c = formats.load_ply_colors(os.path.join(d, "m_raw.ply"))
    v0, t0, n0, c0 = formats.load_ply_colors(os.path.join(d, "m0.ply"))
    assert c0 is None and np.array_equal(v, v0) and np.array_equal(t, t0) and np.array_equal(n, n0)    # the same mesh, plus colours
    assert np.array_equal(c, col) and (c[:, 3] == 255).mean() > 0.9
    # ... with the texture on it: a vertex of the fragment's frame sits at F * vertex in the world the texture is defined in
    world = v.astype(np.float64) @ F[:3, :3].T + F[:3, 3]
    err = np.abs(c[:, :3].astype(np.float64) - synth.texture(world)).max(axis=1)[c[:, 3] == 255]
    bound = synth.TEXTURE_G * (2 * np.sqrt(3) * 3.0 / 512.0 + 0.001) + 1
    print("%d coloured vertices, max |colour - texture| = %.2f levels (level-1 bound %.2f)" % (len(err), err.max(), bound))
    assert err.max() <= bound


def test_warped_frames_with_raw_colour(gpu, tmp_path):
    d = str(tmp_path)
    sc = synth.make_scenario(4, interval=2, warp=True, amplitude=0.004, seed=21)
    depth = synth.to_numpy_u16(sc["depth"])
    dt, ct = synth.render_rgbd(synth.circle_trajectory(4, revolutions=1.0))
    assert np.array_equal(synth.to_numpy_u16(dt), depth)                              # the scenario's own frames, with colour
    rgb = ct.numpy()
    n, I, num = 4, 2, 2
    pose = [formats.FramedTransformation(i, i, i + 1, sc["pose"][i]) for i in range(num)]
    seg = [formats.FramedTransformation(i, i, i + 1, sc["seg"][i]) for i in range(n)]
    formats.save_log(os.path.join(d, "pose.log"), pose + [formats.FramedTransformation(num, num, num + 1, sc["pose"][-1])])
    formats.save_log(os.path.join(d, "seg.log"), seg + [formats.FramedTransformation(n + j, n + j, n + j + 1, sc["seg"][-1]) for j in range(I)])
    formats.save_ctr(os.path.join(d, "grids.ctr"), sc["grids"])
    depth.tofile(os.path.join(d, "frames.raw"))
    rgb.tofile(os.path.join(d, "colour.raw"))
    args = ["--pose_traj", "pose.log", "--seg_traj", "seg.log", "--ctr", "grids.ctr", "--num", "2", "--resolution", "8", "--length", "3.0",
            "--interval", "2", "-oni", "frames.raw", "--max_units", "512"]
    r = subprocess.run([os.path.join(BIN, "Integrate")] + args + ["--color_raw", "colour.raw", "--save_mesh", "m.ply"], cwd=d, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    nv, nt, col = python_route(d, 4, depth, rgb, "m_py.ply", pose_filename_="pose.log", seg_filename_="seg.log", ctr_filename_="grids.ctr", ctr_num_=2,
                               ctr_resolution_=8, ctr_length_=3.0, ctr_interval_=2)
    assert nv > 10000 and read(d, "m.ply") == read(d, "m_py.ply")
    c = formats.load_ply_colors(os.path.join(d, "m.ply"))[3]
    assert np.array_equal(c, col) and (c[:, 3] == 255).mean() > 0.9 and len(np.unique(c[:, :3])) > 50
