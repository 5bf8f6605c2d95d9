#!/usr/bin/env python3
"""Timing of the pose graph optimiser (record: profiles/pose_graph.txt).

    python scripts/posegraph_probe.py [--sizes 64 256 1024] [--density 0.3] [--repeats 5]

Per size: a seeded random-walk graph in the style of tests/posegraph_cases.py (generated in bulk here, information matrices from a pool of 64),
PoseGraph.optimize("switchable") once to warm up and `repeats` times measured with profiling off: the wall time of the synchronous call
(median) and the iteration / trial counts; then `repeats` runs with HIP events round the stages of every trial (er_pgo_set_profiling) for
the per-stage split: linearise, assemble, factor, solve, apply + evaluate.  For the smallest size also the numpy restatement on this host (dense numpy, not g2o) and bin/GraphOptimizer
from process start to exit on the same graph's files."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def rigids(rng, n, max_rot, max_trans, least=0.0):
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = max_rot * rng.uniform(least, 1.0, n)
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    T = np.tile(np.eye(4), (n, 1, 1))
    T[:, :3, :3] = np.eye(3) + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * (K @ K)
    t = rng.normal(size=(n, 3))
    T[:, :3, 3] = t / np.linalg.norm(t, axis=1, keepdims=True) * (max_trans * rng.uniform(least, 1.0, n))[:, None]
    return T


def make_graph(N, density, seed=1):
    import posegraph_cases as pc
    rng = np.random.RandomState(seed)
    steps = rigids(rng, N - 1, 0.5, 0.4, 0.3)
    truth = [np.eye(4)]
    for S in steps:
        truth.append(truth[-1] @ S)
    truth = np.stack(truth)
    inv = np.linalg.inv(truth)
    odo = steps @ rigids(rng, N - 1, 0.002, 0.002)
    iu, ju = np.triu_indices(N, 1)
    pick = (ju == iu + 1) | (rng.uniform(size=len(iu)) < density)
    ti, tj = iu[pick], ju[pick]
    rest = np.flatnonzero(~pick)
    nf = min(len(rest), int(round(0.25 * len(ti))))
    fsel = np.sort(rng.choice(rest, nf, replace=False)) if nf else np.zeros(0, np.int64)
    fi, fj = iu[fsel], ju[fsel]
    Tt = inv[ti] @ truth[tj] @ rigids(rng, len(ti), 0.0015, 0.001)
    Tf = inv[fi] @ truth[fj] @ rigids(rng, nf, 1.0, 0.5, 0.3) if nf else np.zeros((0, 4, 4))
    ids = np.concatenate([np.stack([ti, tj], 1), np.stack([fi, fj], 1)]).astype(np.int32)
    T = np.concatenate([Tt, Tf])
    is_true = np.concatenate([np.ones(len(ti), bool), np.zeros(nf, bool)])
    order = np.lexsort((ids[:, 1], ids[:, 0]))
    pool = np.stack([pc.information(rng) for _ in range(64)])
    return dict(N=N, truth=truth, odo_T=odo, odo_info=pool[rng.randint(0, 64, N - 1)], loop_ids=ids[order], loop_T=T[order],
                loop_info=pool[rng.randint(0, 64, len(ids))], is_true=is_true[order])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--density", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import posegraph_cases as pc
    import posegraph_restatement as pr
    from elasticreconstruction_amd.posegraph import PoseGraph
    for N in a.sizes:
        c = make_graph(N, a.density)
        t0 = time.perf_counter()
        g = PoseGraph(c["odo_T"], (c["loop_ids"], c["loop_T"]), c["odo_info"], c["loop_info"])
        t_create = time.perf_counter() - t0
        g.optimize()                                                          # warm-up
        wall, stages, o = [], [], None
        for _ in range(a.repeats):                                            # the wall time with profiling off: no event in the timed region
            t0 = time.perf_counter()
            o = g.optimize()
            wall.append(time.perf_counter() - t0)
        g.profile(True)
        for _ in range(a.repeats):                                            # the stage split in runs of its own
            g.optimize()
            stages.append(g.profile())
        g.close()
        med = statistics.median(wall)
        ok = bool(np.array_equal(o["kept"], c["is_true"]))
        print("N = %4d: %6d loops (%d false), dimension %d; create %.1f ms; optimize median of %d: %.2f ms (min %.2f, max %.2f); %d iterations, %d trials, "
              "%.3f ms per trial; kept set == true set: %s; worst pose entry %.2g off the truth" % (
                  N, len(c["is_true"]), int((~c["is_true"]).sum()), 6 * (N - 1), t_create * 1e3, a.repeats, med * 1e3, min(wall) * 1e3, max(wall) * 1e3,
                  o["iterations"], o["trials"], med * 1e3 / max(o["trials"], 1), ok, np.abs(o["poses"] - c["truth"]).max()))
        keys = list(stages[0])
        print("          per stage, ms summed over the trials (median): " + ", ".join("%s %.3f" % (k, statistics.median(s[k] for s in stages)) for k in keys))
        if N == min(a.sizes):
            t0 = time.perf_counter()
            ref = pr.Graph(c["odo_T"], c["loop_ids"], c["loop_T"], c["odo_info"], c["loop_info"]).optimize()
            t_ref = time.perf_counter() - t0
            print("          the numpy restatement on this host (dense numpy, not g2o): %.0f ms, %d trials: %.0f x the device's %.2f ms; poses %.2g apart" % (
                t_ref * 1e3, ref["trials"], t_ref / med, med * 1e3, np.abs(ref["poses"] - o["poses"]).max()))
            with tempfile.TemporaryDirectory() as d:
                pc.write_files(c, d)
                exe = os.path.join(ROOT, "elasticreconstruction_amd", "bin", "GraphOptimizer")
                cmd = [exe, "--odometry", "odometry.log", "--odometryinfo", "odometry.info", "--loop", "result.txt", "--loopinfo", "result.info"]
                ts = []
                for _ in range(a.repeats + 1):
                    t0 = time.perf_counter()
                    subprocess.run(cmd, cwd=d, check=True, capture_output=True, timeout=300)
                    ts.append(time.perf_counter() - t0)
                print("          bin/GraphOptimizer, process start to exit on these files (median of %d after one warm-up): %.0f ms" % (a.repeats, statistics.median(ts[1:]) * 1e3))


if __name__ == "__main__":
    main()
