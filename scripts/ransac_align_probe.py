"""The RANSAC pose search on one pair, timed, next to the route it replaces:
python scripts/ransac_align_probe.py [points] [iterations] [repetitions] [outlier fractions ...]
  one call   feature_knn, then ransac_align (everything on the device)
  baseline   what the library offered before er_ransac_align: the same generator, samples, matches and polygon test in numpy on the
             host (tests/ransac_restatement.py, fed the same k-NN table), a float64 Kabsch per survivor, the normal test, then
             er_ransac_fitness_batch on the survivors and the selection on the host
Host clock around calls that end synchronised, a warm-up of each route first, the routes alternating; medians."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import ransac_restatement as rr
from elasticreconstruction_amd import synth
from elasticreconstruction_amd.icp import Cloud, Features, feature_knn, ransac_align, ransac_fitness_batch

points = int(sys.argv[1]) if len(sys.argv) > 1 else 24000
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 4000000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
fracs = [float(a) for a in sys.argv[4:]] or [0.5, 0.7]
frs = synth.fragment_set(2, target_points=points)


def baseline(sc, cl, knn, seed):
    (x0, n0, _, _), (x1, n1, _, _) = sc
    its, s, c = rr.propose(seed, 0, iters, len(x1), 4, knn, x1, x0, 0.9)
    M, _ = rr.estimate(x1, x0, s, c)
    keep = ~(rr.normal_min_dot(M, n1, n0, s, c).astype(np.float64) < np.cos(np.float64(np.float32(0.52359878))))
    cnt, fit = ransac_fitness_batch(cl[1], cl[0], M[keep], 0.075)
    w = rr.select(its[keep], cnt, fit, len(x1), 0.33, 30000)
    return M[keep][w], int(cnt[w]), len(its), int(keep.sum())


for frac in fracs:
    sc = rr.common_scene(frs=frs, outlier_frac=frac)
    cl = [Cloud(x, n, 0.075) for x, n, _, _ in sc]
    ft = [Features(f) for _, _, _, f in sc]
    knn, _ = feature_knn(ft[1], ft[0], 2)
    r = ransac_align(cl[1], cl[0], ft[1], ft[0], max_iterations=iters, seed=1)                     # warm-up of both routes
    Tb, cb, surv, scored = baseline(sc, cl, knn, 1)
    same = r.converged and np.array_equal(Tb, r.T) and cb == r.n_inliers and scored == r.stats["scored"]
    print("the two routes agree on the winner, its inlier count and the number of scored hypotheses: %s" % same)
    t_knn, t_one, t_base = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter(); feature_knn(ft[1], ft[0], 2); t_knn.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); ransac_align(cl[1], cl[0], ft[1], ft[0], max_iterations=iters, seed=1); t_one.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); baseline(sc, cl, knn, 1); t_base.append(time.perf_counter() - t0)
    gt = np.linalg.inv(sc[0][2]) @ sc[1][2]
    k, o, b = np.median(t_knn), np.median(t_one), np.median(t_base)
    print("outlier_frac %.1f, %d x %d points, %d iterations: %s" % (frac, len(sc[1][0]), len(sc[0][0]), iters, r.stats))
    print("  feature_knn            median %8.2f ms  (%s)" % (k * 1e3, " ".join("%.2f" % (t * 1e3) for t in t_knn)))
    print("  ransac_align (one call, its k-NN included) median %8.2f ms  (%s)  %.1f M iterations/s, %.0f scored hypotheses/s"
          % (o * 1e3, " ".join("%.2f" % (t * 1e3) for t in t_one), iters / o / 1e6, r.stats["scored"] / o))
    print("  host generator + er_ransac_fitness_batch   median %8.2f ms  (%s)  -> one call is %.1f x faster"
          % (b * 1e3, " ".join("%.0f" % (t * 1e3) for t in t_base), b / o))
    print("  result: %d inliers, |T - ground truth|max %.4f" % (r.n_inliers, float(np.abs(r.T.astype(np.float64) - gt).max())))
