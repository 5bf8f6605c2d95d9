#!/usr/bin/env python3
"""The ray caster on one MI355X (profiles/raycast.txt): wall time of TSDFVolume.raycast(device=True) -- one 640 x 480 image, and the three
levels DepthOdometry.align_model takes -- of a volume built from the first 200 frames of configs[1] (bench.py's workload, no warp), with the
hit rate, the samples per ray of the plain march (the restatement's count: the kernel skips through units that do not exist and takes
fewer, how many is not counted), and the same image through csrc/er_raycast_math.h compiled for the host, one thread, with and without
the skip -- the only baseline there is: the feature has no parent and the reference tree no ray caster.  The kernel's own time comes from
running this script under `rocprofv3 --kernel-trace --stats` with --no-baseline (a run of its own).  Then track_model beside track on 6
frames of the 320 x 240 scene against the renderer's poses (the series tests/test_odometry_model_gpu.py asserts on).

usage: python scripts/raycast_probe.py [--frames 200] [--repeat 20] [--no-baseline]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, repeat):
    fn()                                                       # (the first call loads the code object: not timed)
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * min(t), 1e3 * max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    from elasticreconstruction_amd import DepthOdometry, accumulate, synth
    from elasticreconstruction_amd.tsdf import TSDFVolume
    import odometry_cases as oc
    import odometry_restatement as orr
    import raycast_cases as rcc
    import raycast_restatement as rcr
    cols, rows = 640, 480
    sc = synth.make_scenario(a.frames, interval=50, warp=False, total_frames=3000, device="cuda:0")
    torch.cuda.synchronize()
    vol = TSDFVolume(max_units=4096)
    vol.IntegrateFrames(None, sc["traj"], None, device_ptr=sc["depth"].data_ptr())
    vol.synchronize()
    cam = vol.camera_[:4]
    T = sc["traj"][a.frames // 2]
    print("device: %s; volume: %d frames of configs[1], %d units; view: frame %d's pose" % (
        torch.cuda.get_device_name(0), a.frames, vol.unit_count(), a.frames // 2))
    lo, hi = timed(lambda: vol.raycast(T, device=True), a.repeat)
    print("raycast 640 x 480, device tensors            : %7.3f ms (min of %d; max %.3f), call to return" % (lo, a.repeat, hi))
    lo, hi = timed(lambda: vol.raycast(T, levels=3, device=True), a.repeat)
    print("raycast 640 x 480 + 320 x 240 + 160 x 120    : %7.3f ms (min of %d; max %.3f)" % (lo, a.repeat, hi))
    lo, hi = timed(lambda: vol.raycast(T), max(a.repeat // 4, 1))
    print("raycast 640 x 480, numpy arrays (host copies) : %7.3f ms (min; max %.3f)" % (lo, hi))
    dep = vol.raycast(T)[0][0]
    print("hit rate %.4f (%d of %d pixels)" % ((dep > 0).mean(), int((dep > 0).sum()), dep.size))
    if not a.no_baseline:
        import test_raycast_cpu as host
        units = {int(k): vol.read_unit(int(k)) for k in vol.unit_keys()}
        st = {}
        t0 = time.perf_counter()
        want = rcr.raycast(units, cols, rows, cam, T, stats=st)
        print("restatement (numpy, plain march)              : %7.1f ms; %.1f samples per ray, %d hits; depth equal to the device's: %s" % (
            1e3 * (time.perf_counter() - t0), st["samples"] / (cols * rows), st["hits"], np.array_equal(want[0], dep)))
        for skip in (False, True):
            t0 = time.perf_counter()
            got = host.host_raycast(units, cols, rows, cam, T, skip=skip)
            print("header on the host, one thread, skip %-5s    : %7.1f ms; depth equal to the device's: %s" % (
                skip, 1e3 * (time.perf_counter() - t0), np.array_equal(got[0], dep)))
    vol.close()
    # frame-to-model beside frame-to-frame
    n, c, r = 6, 320, 240
    d, W, cam = oc.scene(c, r, n)
    W = np.asarray(W, np.float64).copy()
    W[:, :3, 3] += rcc.SCENE_SHIFT
    od = DepthOdometry(c, r, cam)
    vol = TSDFVolume(c, r, np.array(list(cam) + [2.5, 4.0], np.float32), max_units=1024)
    P, S = od.track_model(vol, d, T0=W[0])
    A = accumulate(od.track(d)[0], W[0])
    print("6 frames of the scene at 320 x 240, error against the renderer's poses (lost: %d):" % int(S.sum()))
    for i in range(1, n):
        print("  frame %d: track_model %.4f deg %.3f mm; track %.4f deg %.3f mm" % ((i,) + orr.pose_error(P[i], W[i])[:1] + (
            orr.pose_error(P[i], W[i])[1] * 1e3,) + orr.pose_error(A[i], W[i])[:1] + (orr.pose_error(A[i], W[i])[1] * 1e3,)))
    t0 = time.perf_counter()
    vol.reset()
    od.track_model(vol, d, T0=W[0])
    print("track_model, 6 frames of 320 x 240, host frames: %.2f ms" % (1e3 * (time.perf_counter() - t0)))


if __name__ == "__main__":
    main()
