"""Voxel grid, normals and FPFH on one fragment, stage by stage, next to the numpy / scipy restatement on the same host:
python scripts/fpfh_probe.py [points] [repetitions]
  device   Cloud.voxel_grid, Cloud.estimate_normals, fpfh, and the whole preprocess_fragment, from a cloud that is already in HBM
  host     tests/fpfh_restatement.py's preprocess on the fragment's host arrays (one run: it takes seconds)
Host clock around calls that return synchronised (every entry point ends with a stream synchronisation and hands back a finished
handle).  The figures are CALL times, not kernel times: each call allocates and frees its device buffers, builds the temporary grid of
its radius and the grid of the cloud it returns, and synchronises several times on the way.  A warm-up of every stage first; medians of
the repetitions.  The script prints; its output is kept by hand in profiles/fpfh.txt."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import fpfh_restatement as fr
from elasticreconstruction_amd import synth
from elasticreconstruction_amd.icp import Cloud, fpfh, preprocess_fragment

points = int(sys.argv[1]) if len(sys.argv) > 1 else 250000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
x, n, _ = synth.fragment_set(1, target_points=points)[0]
c = Cloud(x, n, 0.03)


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, time.perf_counter() - t0


down = c.voxel_grid(0.05, 0.075)
est = down.estimate_normals(0.1)
feat = fpfh(est, 0.25)
preprocess_fragment(c)
t = {"voxel_grid": [], "estimate_normals": [], "fpfh": [], "preprocess_fragment": []}
for _ in range(reps):
    t["voxel_grid"].append(timed(lambda: c.voxel_grid(0.05, 0.075))[1])
    t["estimate_normals"].append(timed(lambda: down.estimate_normals(0.1))[1])
    t["fpfh"].append(timed(lambda: fpfh(est, 0.25))[1])
    t["preprocess_fragment"].append(timed(lambda: preprocess_fragment(c))[1])
ref, t_host = timed(lambda: fr.preprocess(x, n))
got = feat.read()
ulp = np.abs(got.view(np.int32).astype(np.int64) - ref["feat"].view(np.int32).astype(np.int64))
print("fragment of %d points -> %d after the voxel grid (restatement: %d); FPFH neighbourhoods %d .. %d"
      % (len(x), down.n, len(ref["xyz"]), ref["nn"].min(), ref["nn"].max()))
print("descriptors against the restatement's (device normals, so last-bit differences in the inputs): %.4f %% of the values differ by more than one float32"
      % (100.0 * float((ulp > 1).mean())))
for k, v in t.items():
    print("  %-20s median %8.3f ms  (%s)" % (k, np.median(v) * 1e3, " ".join("%.3f" % (q * 1e3) for q in v)))
print("  %-20s %8.0f ms once -> preprocess_fragment is %.0f x faster" % ("numpy / scipy host", t_host * 1e3, t_host / np.median(t["preprocess_fragment"])))
