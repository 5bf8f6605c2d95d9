#!/usr/bin/env python3
"""Depth odometry on one MI355X (profiles/depth_odometry.txt): wall time of DepthOdometry.track on N frames of 640 x 480 that were rendered
into HBM, with the frames given as a device pointer and as host memory, and the same frames through the numpy restatement
(tests/odometry_restatement.py) on the same host -- the only baseline there is: the feature has no parent and the reference tree no KinFu.
The per-kernel split comes from running this script under `rocprofv3 --kernel-trace --stats` with --no-baseline (a run of its own).

usage: python scripts/odometry_probe.py [--frames 64 512] [--repeat 3] [--baseline-pairs 4] [--no-baseline]"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def sweep(n, step_deg=0.3):
    """n poses of a hand-held sweep around the room centre looking inward: step_deg of arc per frame, one slow tilt up and down."""
    from elasticreconstruction_amd import synth
    return synth.kinfu_camera_path(0, 4, frames=n, arc_deg=step_deg * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--baseline-pairs", type=int, default=4)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    from elasticreconstruction_amd import DepthOdometry, synth
    import odometry_restatement as orr
    cols, rows, cam = 640, 480, synth.CAM
    od = DepthOdometry(cols, rows, cam)
    print("device: %s; frames %d x %d, levels %d, iterations %s" % (torch.cuda.get_device_name(0), cols, rows, od.levels, od.iterations))
    for n in a.frames:
        W = sweep(n)
        depth = synth.render_depth(W, device="cuda:0")
        torch.cuda.synchronize()
        host = synth.to_numpy_u16(depth)
        for name, src in (("device pointer", depth), ("host memory", host)):
            times = []
            for _ in range(a.repeat + 1):                      # the first call allocates the window and loads the code objects: not timed
                t0 = time.perf_counter()
                T, status = od.track(src)
                times.append(time.perf_counter() - t0)
            t = np.array(times[1:])
            print("track, %4d frames, %-14s: %8.2f ms (min of %d; max %.2f)  = %.1f pairs/s, %.3f ms per pair; lost %d" % (
                n, name, t.min() * 1e3, a.repeat, t.max() * 1e3, (n - 1) / t.min(), t.min() * 1e3 / (n - 1), int(status.sum())))
        err = [orr.pose_error(T[i], np.linalg.inv(W[i]) @ W[i + 1]) for i in range(n - 1)]
        print("       against the renderer's poses: worst rotation error %.4f deg, worst translation error %.3f mm (motion per pair %.3f deg)" % (
            max(e[0] for e in err), max(e[1] for e in err) * 1e3, orr.pose_error(np.eye(4), np.linalg.inv(W[0]) @ W[1])[0]))
        if not a.no_baseline and n == a.frames[0]:
            m = a.baseline_pairs
            ref = orr.Odometry(cols, rows, cam)
            t0 = time.perf_counter()
            maps = [ref.maps(f) for f in host[:m + 1].reshape(m + 1, rows, cols)]
            t1 = time.perf_counter()
            out = [ref.align_maps(maps[i], maps[i + 1]) for i in range(m)]
            t2 = time.perf_counter()
            worst = max(np.abs(out[i][0] - T[i]).max() for i in range(m))
            print("restatement (numpy, this host), first %d pairs: maps %.1f ms per frame, align %.1f ms per pair; |T - T_device| max %.3g" % (
                m, (t1 - t0) * 1e3 / (m + 1), (t2 - t1) * 1e3 / m, worst))
    od.close()


if __name__ == "__main__":
    main()
