"""bin/GraphOptimizer on files against the Python route (posegraph.graph_optimizer) byte for byte on the N = 10 fixture of
tests/posegraph_cases.py -- both modes, the three spellings of an option, the default file names, missing .info files, --help, no device -- and
the chain GlobalRegistration -> GraphOptimizer -> BuildCorrespondence on the relief fragments of tests/test_global_registration_program_gpu.py:
the files one program writes are the files the next one reads."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import posegraph_cases as pc
import test_global_registration_program_gpu as grp
from elasticreconstruction_amd import formats
from elasticreconstruction_amd.posegraph import graph_optimizer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elasticreconstruction_amd", "bin")
OUT = ("opt_output.log", "loop_remain.log", "refine.log")
world = grp.world                                                             # the module-scoped fixture with the fragment files (made once per process)


def run(cwd, *args, env=None):
    return subprocess.run([os.path.join(BIN, "GraphOptimizer")] + [str(a) for a in args], capture_output=True, text=True, cwd=str(cwd), timeout=120,
                          env=dict(os.environ, **(env or {})))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the N = 10 files and, per mode, the Python route's outputs on them"""
    d = tmp_path_factory.mktemp("pgo_program")
    paths = pc.write_files(pc.case("n10"), d)
    want = {}
    for method, it in (("switchable", 100), ("em", pc.EM_ROUNDS)):
        o = d / ("py_" + method)
        o.mkdir()
        out = graph_optimizer(paths["odometry"], paths["loop"], paths["odometryinfo"], paths["loopinfo"], pose=str(o / OUT[0]), keep=str(o / OUT[1]),
                              refine=str(o / OUT[2]), method=method, iteration=it)
        assert np.array_equal(out["kept"], pc.case("n10")["is_true"])
        want[method] = {n: (o / n).read_bytes() for n in OUT if (o / n).exists()}
    assert set(want["switchable"]) == set(OUT) and set(want["em"]) == set(OUT[:2])
    return dict(dir=d, want=want)


def same(d, want):
    for n in OUT:
        assert ((d / n).read_bytes() if (d / n).exists() else None) == want.get(n), n


def test_both_modes_in_every_spelling(gpu, files):
    d = files["dir"]
    io = ["--odometry", "odometry.log", "--odometryinfo", "odometry.info", "--loop", "result.txt", "--loopinfo", "result.info"]
    spellings = {
        "switchable": (io, [a + "=" + b for a, b in zip(io[::2], io[1::2])] + ["--function=switchable", "--weight=1.0", "--iteration=100"],
                       io + ["-f", "switchable", "-w", "1", "-i", "100"], io + ["--function", "switchable", "--weight", "1.0", "--iteration", "100"]),
        "em": (io + ["--function", "em", "--iteration", pc.EM_ROUNDS], io + ["--function=em", "--iteration=%d" % pc.EM_ROUNDS], io + ["-f", "em", "-i", pc.EM_ROUNDS]),
    }
    for method, forms in spellings.items():
        for args in forms:
            for n in OUT:
                if (d / n).exists():
                    (d / n).unlink()
            r = run(d, *args, env=dict(ER_TIMING="1"))
            assert r.returncode == 0, r.stdout + r.stderr
            same(d, files["want"][method])
            assert "[timing] optimize (er_pgo_optimize)" in r.stderr and "10 poses, 25 loop closures, 20 kept" in r.stdout
    out = d / "named"
    out.mkdir()
    r = run(d, *io, "--pose", out / "p.log", "--keep=" + str(out / "k.log"), "--refine", out / "r.log")
    assert r.returncode == 0 and "[timing]" not in r.stderr
    assert [(out / n).read_bytes() for n in ("p.log", "k.log", "r.log")] == [files["want"]["switchable"][n] for n in OUT]


def test_default_names_and_missing_information(gpu, files):
    d = files["dir"] / "defaults"
    d.mkdir()
    for src, dst in (("odometry.log", "odometry.log"), ("odometry.info", "odometry.info"), ("result.txt", "loop.log"), ("result.info", "loop.info")):
        shutil.copy(str(files["dir"] / src), str(d / dst))
    r = run(d, "-f", "switchable")
    assert r.returncode == 0, r.stdout + r.stderr
    same(d, files["want"]["switchable"])
    e = files["dir"] / "no_info"                                              # identity information: another result, the Python route's
    e.mkdir()
    for n in ("odometry.log", "loop.log"):
        shutil.copy(str(d / n), str(e / n))
    r = run(e, "--iteration", 100)
    assert r.returncode == 0, r.stdout + r.stderr
    o = e / "py"
    o.mkdir()
    graph_optimizer(str(e / "odometry.log"), str(e / "loop.log"), str(e / "odometry.info"), str(e / "loop.info"), pose=str(o / OUT[0]), keep=str(o / OUT[1]),
                    refine=str(o / OUT[2]))
    same(e, {n: (o / n).read_bytes() for n in OUT})
    assert (e / OUT[0]).read_bytes() != files["want"]["switchable"][OUT[0]]
    r = run(e, "--function", "neither")                                       # the reference runs neither branch and returns 0
    assert r.returncode == 0


def test_help_no_work_and_no_device(gpu, files):
    d = files["dir"] / "empty"
    d.mkdir()
    for args in ((), ("--help",), ("-h",)):
        r = run(d, *args)
        assert r.returncode == 1 and "--odometryinfo" in r.stdout and "--refine" in r.stdout
    r = run(d, "--weight", 2)
    assert r.returncode == 0 and not any((d / n).exists() for n in OUT)       # no odometry.log: no work
    io = ["--loop", "result.txt", "--loopinfo", "result.info"]
    r = run(files["dir"], *io, "--pose", d / "p.log", env=dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert r.returncode == 1 and "no HIP device" in r.stderr and not (d / "p.log").exists()


def test_chain_global_registration_to_build_correspondence(gpu, world):
    """GlobalRegistration's odometry mode writes odometry.log / odometry.info / result.txt / result.info; GraphOptimizer reads exactly those and
    writes refine.log; BuildCorrespondence --reg_traj refine.log --registration reads that."""
    d = grp.workdir(world, "pgo_chain")
    seg = grp.segment_log(world["frs"])
    formats.save_log(str(d / "segment.log"), [formats.FramedTransformation(i, i, i + 1, T) for i, T in enumerate(seg)])
    r = grp.run(d, world["frags"], "segment.log", grp.FRAGMENT, "--seed", 1)
    assert r.returncode == 0, r.stdout + r.stderr
    r = run(d, "--odometry", "odometry.log", "--odometryinfo", "odometry.info", "--loop", "result.txt", "--loopinfo", "result.info")
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    odo, refine = formats.load_log(str(d / "odometry.log")), formats.load_log(str(d / "refine.log"))
    assert len(odo) == 2 and len(refine) >= len(odo)
    for a, b in zip(odo, refine):
        assert (a.id1, a.id2, a.frame) == (b.id1, b.id2, b.frame) and np.array_equal(a.T, b.T)
    assert all(t.id1 + 1 < t.id2 for t in refine[len(odo):])
    assert len(formats.load_log(str(d / "opt_output.log"))) == 3
    for i in range(3):
        shutil.copy(world["frags"] + "cloud_bin_%d.pcd" % i, str(d / ("cloud_bin_%d.pcd" % i)))
    r = subprocess.run([os.path.join(BIN, "BuildCorrespondence"), "--reg_traj", "refine.log", "--registration"], cwd=str(d), capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and len(formats.load_log(str(d / "reg_output.log"))) >= 1
