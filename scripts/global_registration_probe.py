"""All-pairs GlobalRegistration, timed: the loop of one er_ransac_align and one er_ransac_inliers call per pair against ONE
er_ransac_align_batch call, and the drop-in program.
python scripts/global_registration_probe.py [repetitions] [sections: a b c, or `trace` for section (a)'s batch route alone]
  (a) the 28 pairs of synth.fragment_set(8, 24000) with synth.landmark_features at outlier_frac 0.7, alignment.config's parameters,
      4 000 000 iterations -- the scene of profiles/ransac_align.txt, all pairs of it
  (b) the 3 pairs of synth.relief_fragments() from their full clouds, the device's own descriptors (the preprocessing is outside the clock)
  (c) bin/GlobalRegistration on the relief fragments written as PCD files, process start to exit, with its stage report
Host clock around calls that end synchronised, a warm-up of each route first, the routes alternating in one process; medians and ranges.
The probe asserts that the two routes return the same bits."""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import ransac_restatement as rr
from elasticreconstruction_amd import formats, synth
from elasticreconstruction_amd.icp import Cloud, Features, global_registration, preprocess_fragment, ransac_align_batch

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
sections = sys.argv[2:] or ["a", "b", "c"]


def same(a, b):
    return (len(a[0]) == len(b[0]) and all((p.id1, p.id2, p.frame) == (q.id1, q.id2, q.frame) and p.T.tobytes() == q.T.tobytes() for p, q in zip(a[0], b[0]))
            and all(p.info.tobytes() == q.info.tobytes() for p, q in zip(a[1], b[1])))


def report(name, t):
    t = np.array(t) * 1e3
    print("  %-46s median %9.2f ms  (min %.2f .. max %.2f; %s)" % (name, np.median(t), t.min(), t.max(), " ".join("%.2f" % v for v in t)))
    return float(np.median(t)), float(t.max() - t.min())


def compare(what, clouds, feats, **kw):
    loop = lambda: global_registration(clouds, feats, **kw)
    one = lambda: global_registration(clouds, feats, batch=True, **kw)
    a, b = loop(), one()                                                                     # warm-up of both routes
    assert same(a, b), "the two routes differ"
    t_loop, t_one = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); a = loop(); t_loop.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); b = one(); t_one.append(time.perf_counter() - t0)
        assert same(a, b), "the two routes differ"
    n = len(clouds) * (len(clouds) - 1) // 2
    print("%s: %d pairs, %d converged, sizes %s; the two routes return the same bits: True" % (what, n, len(a[0]), [c.n for c in clouds]))
    ml, sl = report("loop: ransac_align + ransac_inliers per pair", t_loop)
    mo, _ = report("one call: ransac_align_batch(want_info=True)", t_one)
    print("  per pair: loop %.2f ms, one call %.2f ms; one call / loop = %.3f; the loop's own min-to-max spread %.2f ms; batch median %s loop median + spread"
          % (ml / n, mo / n, mo / ml, sl, "<=" if mo <= ml + sl else ">"))
    assert mo <= ml + sl, "the batch route is slower than the loop by more than the loop's own spread"


if "a" in sections or "trace" in sections:
    sc = rr.common_scene(frs=synth.fragment_set(8, target_points=24000), outlier_frac=0.7)
    cl = [Cloud(x, n, 0.075) for x, n, _, _ in sc]
    ft = [Features(f) for _, _, _, f in sc]
    if "trace" in sections:
        pairs = [(i, j) for i in range(8) for j in range(i + 1, 8)]
        for _ in range(2):
            ransac_align_batch([cl[j] for _, j in pairs], [cl[i] for i, _ in pairs], [ft[j] for _, j in pairs], [ft[i] for i, _ in pairs],
                               want_info=True, max_iterations=4000000, seed=1)
        sys.exit(0)
    compare("(a) fragment_set(8, 24000), outlier_frac 0.7, 4 000 000 iterations", cl, ft, max_iterations=4000000, seed=1)

frs = None
if "b" in sections or "c" in sections:
    frs = synth.relief_fragments()
if "b" in sections:
    pre = [preprocess_fragment(Cloud(x, n, 0.03)) for x, n, _ in frs]
    compare("(b) relief_fragments(), 4 000 000 iterations", [p[0] for p in pre], [p[1] for p in pre], max_iterations=4000000, seed=1)
if "c" in sections:
    exe = os.path.join(ROOT, "elasticreconstruction_amd", "bin", "GlobalRegistration")
    with tempfile.TemporaryDirectory() as d:
        os.mkdir(os.path.join(d, "frags"))
        for i, (x, n, _) in enumerate(frs):
            formats.save_pcd_xyzn(os.path.join(d, "frags", "cloud_bin_%d.pcd" % i), x, n)
        t, last = [], None
        for _ in range(reps + 1):                                                            # the first run is the warm-up (file cache, code objects)
            t0 = time.perf_counter()
            last = subprocess.run([exe, os.path.join(d, "frags") + "/", "--seed", "1"], cwd=d, capture_output=True, text=True, env=dict(os.environ, ER_TIMING="1"))
            t.append(time.perf_counter() - t0)
            assert last.returncode == 0, last.stderr
        print("(c) bin/GlobalRegistration on relief_fragments() as PCD (3 x 100 000 points, default alignment.config, 4 000 000 iterations), process start to exit")
        report("bin/GlobalRegistration <dir>/ --seed 1", t[1:])
        print("  %d pairs in result.txt; the last run's stages:" % len(formats.load_log(os.path.join(d, "result.txt"))))
        print("\n".join("    " + line for line in last.stderr.splitlines() if line.startswith("[timing]")))
