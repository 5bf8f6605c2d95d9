"""bin/MakeFragments (csrc/host/MakeFragments.cpp) on files: the 14 frames of tests/test_fragments_gpu.py at 320 x 240 as a raw
stream and as 16-bit PNGs, against the Python builder -- the segment log as text, every cloud_bin_<k>.pcd byte for byte -- and the log handed
to bin/Integrate --seg_traj."""
import os
import subprocess

import numpy as np
import pytest

import odometry_cases as oc
from elasticreconstruction_amd import formats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elasticreconstruction_amd", "bin")
COLS, ROWS, N, INTERVAL, UNITS = 320, 240, 14, 4, 256
_cache = {}


def inputs(tmp):
    """frames.raw, list.txt + PNGs and cam.param in `tmp`; -> the frames."""
    from PIL import Image
    d, _, cam = oc.scene(COLS, ROWS, N)
    d = d.reshape(N, -1).copy()
    d.tofile(os.path.join(tmp, "frames.raw"))
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        for i in range(N):
            Image.fromarray(d[i].reshape(ROWS, COLS)).save(os.path.join(tmp, "%03d.png" % i))
            f.write("%03d.png\n" % i)
    formats.save_camera(os.path.join(tmp, "cam.param"), np.array(list(cam) + [2.5, 4.0], np.float32))
    return d


def python_files(tmp, d):
    """What FragmentBuilder.save writes for the same frames, at the base pose: {name: bytes}."""
    from elasticreconstruction_amd import FragmentBuilder
    cam6 = formats.load_camera(os.path.join(tmp, "cam.param"))
    b = FragmentBuilder(COLS, ROWS, cam6, interval=INTERVAL, lanes=2, max_units=UNITS)
    W, S, frags = b.build(d)
    out = os.path.join(tmp, "py")
    paths = b.save(out)
    b.close()
    assert len(frags) == 4 and [os.path.basename(p) for p in paths] == ["cloud_bin_%d.pcd" % k for k in range(4)] + ["100-0.log"]
    # the log after the %.8f round trip: load_log of the text gives W to 8 decimals, and save_log of W is that text
    logged = formats.load_log(paths[-1])
    assert len(logged) == N and all(ft.id1 == i and ft.id2 == i and ft.frame == i + 1 for i, ft in enumerate(logged))
    assert np.abs(np.stack([ft.T for ft in logged]) - W).max() <= 0.5e-8 + 1e-15
    return {os.path.basename(p): open(p, "rb").read() for p in paths}, S


def run(tmp, out, source, extra=()):
    os.makedirs(os.path.join(tmp, out))
    cmd = [os.path.join(BIN, "MakeFragments")] + source + ["--dir", out, "--cols", str(COLS), "--rows", str(ROWS), "--camera", "cam.param",
                                                          "--interval", str(INTERVAL), "--max_units", str(UNITS)] + list(extra)
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return {n: open(os.path.join(tmp, out, n), "rb").read() for n in sorted(os.listdir(os.path.join(tmp, out)))}, r


def test_program_equals_the_python_builder_from_raw_and_png_for_any_lanes(gpu, tmp_path):
    tmp = str(tmp_path)
    d = inputs(tmp)
    want, status = python_files(tmp, d)
    raw1, r = run(tmp, "raw1", ["--depth_raw", "frames.raw"], ["--lanes", "1"])
    assert sorted(raw1) == sorted(want)
    for name in want:
        assert raw1[name] == want[name], name
    assert r.stderr.count("lost at frame") == int((status != 0).sum())
    raw3, _ = run(tmp, "raw3", ["--depth_raw", "frames.raw"], ["--lanes", "3"])
    assert raw3 == raw1, "--lanes is not part of any file"
    png, _ = run(tmp, "png", ["--depth_list", "list.txt"], ["--seg_log", "png/seg.log"])
    assert png.pop("seg.log") == want["100-0.log"] and png == {k: v for k, v in want.items() if k.endswith(".pcd")}
    # Integrate --seg_traj with an identity --pose_traj takes the log.  (Integrate reads 640 x 480 frames: it sees the stream's bytes as three
    # of them; what is checked is that the log is read, composed with the poses and integrated without a complaint.)
    formats.save_log(os.path.join(tmp, "pose.log"), [formats.FramedTransformation(k, k, k + 1, np.eye(4)) for k in range(3)])
    r = subprocess.run([os.path.join(BIN, "Integrate"), "--pose_traj", "pose.log", "--seg_traj", "raw1/100-0.log", "--interval", str(INTERVAL),
                        "--depth_raw", "frames.raw", "--save_to", "world.pcd"], cwd=tmp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and os.path.exists(os.path.join(tmp, "world.pcd")), r.stdout + r.stderr
    assert "seg_traj" not in r.stderr
