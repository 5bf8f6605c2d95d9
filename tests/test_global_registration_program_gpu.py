"""bin/GlobalRegistration on PCD files against the Python route.  Fragments: synth.relief_fragments(num=3, n_points=30000) written as
cloud_bin_<i>.pcd; alignment.config: max_iteration=200000, inlier_fraction=0.2, everything else the defaults; --seed 1.
do_all must write result.txt / result.info byte for byte as formats.save_log / save_info write
global_registration_fragments(clouds, cfg, seed=1, batch=True, inverse=inverse4f) of the same files.  (inverse4f, because the program's
float32 inverse of a swapped pair is the cofactor formula of csrc/host/er_globalreg.h, which icp.inverse4f restates operation for
operation; np.linalg.inv's float32 bits are those of whatever LAPACK build numpy carries, and a file of 8 decimals shows them.)
What the numpy restatements alone (tests/fpfh_restatement.py, tests/ransac_restatement.py, the CPU oracle's getFitness) give for these
inputs, without a GPU: 3963, 4284 and 4441 points after downsampling, so smart swap turns every pair round; (0,1) converges with 3963
inliers of 3963 (48 018 hypotheses scored of 200 000 iterations), (0,2) with 3963 of 3963 (49 705 scored), (1,2) with 4284 of 4284 (57 955 scored): all three pairs are in result.txt.
The odometry mode runs on a segment.log of 3 x 5 poses made from the fragments' ground-truth poses and a seeded perturbation of 0.3
degrees / 3 mm; a second run, with one pose moved 2 m, finds result.txt and skips do_all."""
import os
import subprocess

import numpy as np
import pytest

from elasticreconstruction_amd import formats, synth
from elasticreconstruction_amd.icp import Cloud, global_registration_fragments, inverse4f, ransac_inliers
from test_global_registration_cpu import np_trajectories

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elasticreconstruction_amd", "bin", "GlobalRegistration")
CONFIG = "max_iteration=200000\ninlier_fraction=0.2\n"
FRAGMENT = 5
_cache = {}


def run(cwd, *args, timing=False):
    env = dict(os.environ, ER_TIMING="1") if timing else {k: v for k, v in os.environ.items() if k != "ER_TIMING"}
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, cwd=str(cwd), env=env, timeout=120)


def reasons(r):
    return [line for line in r.stderr.splitlines() if line.startswith("GlobalRegistration:")]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The fragment directory, and the Python route's result on the files in it."""
    if "w" not in _cache:
        root = tmp_path_factory.mktemp("globalreg")
        frags = root / "frags"
        frags.mkdir()
        frs = synth.relief_fragments(num=3, n_points=30000)
        for i, (x, n, _) in enumerate(frs):
            formats.save_pcd_xyzn(str(frags / ("cloud_bin_%d.pcd" % i)), x, n)
        clouds = []
        for i in range(3):
            f = formats.load_pcd(str(frags / ("cloud_bin_%d.pcd" % i)))
            clouds.append(Cloud(np.stack([f["x"], f["y"], f["z"]], axis=1), np.stack([f["normal_x"], f["normal_y"], f["normal_z"]], axis=1), 0.075))
        cfgfile = root / "alignment.config"
        cfgfile.write_text(CONFIG)
        cfg = formats.load_alignment_config(str(cfgfile))
        traj, info, down, feats = global_registration_fragments(clouds, cfg, seed=1, batch=True, inverse=inverse4f)
        _cache["w"] = dict(root=root, frags=str(frags) + "/", frs=frs, cfg=cfg, traj=traj, info=info, down=down)
    return _cache["w"]


def workdir(world, name, config=CONFIG):
    d = world["root"] / name
    d.mkdir()
    if config is not None:
        (d / "alignment.config").write_text(config)
    return d


def test_do_all_writes_the_python_routes_files(gpu, world):
    d = workdir(world, "do_all")
    r = run(d, world["frags"], "--seed", 1, timing=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "3 detected." in r.stdout and "max_iteration = 200000" in r.stdout
    assert len(world["traj"]) >= 1, "no pair converges: nothing would be compared"
    swapped = [world["down"][t.id2].n > world["down"][t.id1].n for t in world["traj"]]
    print("pairs in the file:", [(t.id1, t.id2, s) for t, s in zip(world["traj"], swapped)])
    formats.save_log(str(d / "expected.txt"), world["traj"])
    formats.save_info(str(d / "expected.info"), world["info"])
    assert (d / "result.txt").read_bytes() == (d / "expected.txt").read_bytes()
    assert (d / "result.info").read_bytes() == (d / "expected.info").read_bytes()
    assert all(t.frame == 3 for t in world["traj"]) and [(t.id1, t.id2) for t in world["traj"]] == sorted((t.id1, t.id2) for t in world["traj"])
    assert "[timing] RANSAC (er_ransac_align_batch)" in r.stderr and "[timing] Preprocess" in r.stderr
    r = run(d, world["frags"], "--seed", 1)                                                 # without ER_TIMING: no report, the same files
    assert r.returncode == 0 and "[timing]" not in r.stderr
    assert (d / "result.txt").read_bytes() == (d / "expected.txt").read_bytes()
    r = run(workdir(world, "no_config", None), world["frags"])
    assert r.returncode == 0 and "alignment.config not found! Use default parameters." in r.stdout


def segment_log(frs, broken=False):
    """15 poses: fragment f's five start at an arbitrary pose and end so that the odometry of the pair (f - 1, f) comes out as the ground
    truth inv(F[f-1]) F[f] times a small perturbation.  broken: the last pose of the third fragment is moved 2 m."""
    A = synth.perturbation(21, 30.0, 0.5)
    G = [np.linalg.inv(frs[f - 1][2]) @ frs[f][2] @ synth.perturbation(40 + f, 0.3, 0.003) for f in (1, 2)]
    B = synth.perturbation(22, 50.0, 1.0)
    key = {0: A, 4: G[0] @ A, 5: B, 9: B @ np.linalg.inv(A) @ G[1] @ A, 10: synth.perturbation(23, 20.0, 0.3)}
    if broken:
        key[9] = key[9].copy()
        key[9][:3, 3] += 2.0
    seg = []
    for i in range(15):
        seg.append(key[i] if i in key else seg[-1] @ synth.perturbation(60 + i, 2.0, 0.02))
    return seg


def check_logs(d, seg, num=3):
    ref = np_trajectories(seg, FRAGMENT, num)
    for name, want in zip(("init.log", "pose.log", "odometry.log"), ref):
        got = formats.load_log(str(d / name))
        assert [(t.id1, t.id2, t.frame) for t in got] == [(a, b, f) for a, b, f, _ in want], name
        assert max(np.abs(t.T - T).max() for t, (_, _, _, T) in zip(got, want)) < 1e-7, name   # the files carry 8 decimals
    return ref[2]


def expected_info(world, odo):
    out, counts = [], []
    cfg = world["cfg"]
    for (a, b, f, T) in odo:
        src, tgt = world["down"][b], world["down"][a]
        inl, _, _, info_s, _ = ransac_inliers(src, tgt, T.astype(np.float32), cfg["max_correspondence_distance"])
        ok = len(inl) > 0 and (np.float32(len(inl)) / np.float32(src.n) >= np.float32(cfg["inlier_fraction"]) or len(inl) > cfg["inlier_number"])
        out.append(formats.FramedInformation(a, b, f, info_s if ok else np.zeros((6, 6))))
        counts.append((len(inl), src.n, bool(ok)))
    return out, counts


def test_odometry_mode(gpu, world):
    d = workdir(world, "odometry")
    seg = segment_log(world["frs"])
    formats.save_log(str(d / "segment.log"), [formats.FramedTransformation(i, i, i + 1, T) for i, T in enumerate(seg)])
    r = run(d, world["frags"], "segment.log", FRAGMENT, "--seed", 1)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "result.txt detected" not in r.stdout
    odo = check_logs(d, [t.T for t in formats.load_log(str(d / "segment.log"))])            # from the poses as the file's 8 decimals give them
    info, counts = expected_info(world, odo)
    print("odometry guesses (inliers, points, accepted):", counts)
    assert all(ok for _, _, ok in counts) and all(i.info.any() for i in info)
    formats.save_info(str(d / "expected.info"), info)
    assert (d / "odometry.info").read_bytes() == (d / "expected.info").read_bytes()
    formats.save_log(str(d / "expected.txt"), world["traj"])                                # do_all ran afterwards: the same result.txt as on its own
    assert (d / "result.txt").read_bytes() == (d / "expected.txt").read_bytes()
    # the second run: one pose moved 2 m makes the guess of the pair (1, 2) useless, and result.txt is there
    seg = segment_log(world["frs"], broken=True)
    formats.save_log(str(d / "segment.log"), [formats.FramedTransformation(i, i, i + 1, T) for i, T in enumerate(seg)])
    (d / "result.txt").write_text("kept\n")
    r = run(d, world["frags"], "segment.log", FRAGMENT)
    assert r.returncode == 0 and "result.txt detected. skip global registration." in r.stdout
    assert (d / "result.txt").read_text() == "kept\n"
    odo = check_logs(d, [t.T for t in formats.load_log(str(d / "segment.log"))])
    info, counts = expected_info(world, odo)
    print("with the 2 m shift:", counts)
    assert counts[0][2] and not counts[1][2] and not info[1].info.any()
    formats.save_info(str(d / "expected.info"), info)
    assert (d / "odometry.info").read_bytes() == (d / "expected.info").read_bytes()
    got = formats.load_info(str(d / "odometry.info"))
    assert [(i.id1, i.id2, i.frame) for i in got] == [(0, 1, 3), (1, 2, 3)] and not got[1].info.any()   # the pair is written in either case


def test_refusals(gpu, world):
    import shutil
    d = workdir(world, "missing")
    part = d / "frags"
    part.mkdir()
    for i in (0, 2):
        shutil.copy(world["frags"] + "cloud_bin_%d.pcd" % i, str(part / ("cloud_bin_%d.pcd" % i)))
    r = run(d, str(part) + "/")
    assert r.returncode != 0 and len(reasons(r)) == 1 and "cloud_bin_1.pcd" in reasons(r)[0] and not (d / "result.txt").exists()
    d = workdir(world, "short")
    seg = segment_log(world["frs"])[:10]                                                    # three fragments of five need 11
    formats.save_log(str(d / "segment.log"), [formats.FramedTransformation(i, i, i + 1, T) for i, T in enumerate(seg)])
    r = run(d, world["frags"], "segment.log", FRAGMENT)
    assert r.returncode != 0 and len(reasons(r)) == 1 and "10 entries" in reasons(r)[0] and "11" in reasons(r)[0]
    assert not (d / "init.log").exists() and not (d / "result.txt").exists()
    d = workdir(world, "aux", CONFIG + "aux_data=true\n")
    r = run(d, world["frags"])
    assert r.returncode != 0 and len(reasons(r)) == 1 and "aux_data=true is refused" in reasons(r)[0] and not (d / "result.txt").exists()
