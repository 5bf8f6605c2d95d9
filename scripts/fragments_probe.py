"""Measures the fragment builder on one GPU: 8 fragments x 50 frames of 640 x 480, synth.kinfu_camera_path rendered on the
device, every fragment started at the kinfu base pose.

    python scripts/fragments_probe.py [--fragments 8] [--frames 50] [--lanes 1,2,4,8,16] [--max_units 512] [--kernels-only L]

Prints, per lane count, frames per second from FragmentBuilder.build's call to its return (device depth; min and max of --repeat runs), the
device memory a lane takes, and -- in the same process -- the loop the builder replaces: DepthOdometry.track_model per fragment on a fresh
TSDFVolume, then extract_oriented.  Checks that both routes give the same poses.  --kernels-only L runs ONE build with L lanes and nothing
else: the run to put under `rocprofv3 --kernel-trace --stats -- python scripts/fragments_probe.py --kernels-only 8` (and once more with the
baseline, --kernels-only 0) to set k_raycast_batch per step against lanes x levels k_raycast."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fragments", type=int, default=8)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--lanes", default="1,2,4,8,16")
    ap.add_argument("--max_units", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--kernels-only", type=int, default=None)
    a = ap.parse_args()
    import torch
    from elasticreconstruction_amd import DepthOdometry, ErError, FragmentBuilder, synth
    from elasticreconstruction_amd.tsdf import TSDFVolume
    cols, rows = 640, 480
    cam6 = np.array(list(synth.CAM) + [2.5, 2.5], np.float32)
    nf, fr = a.fragments, a.frames
    depth = torch.cat([synth.render_depth(synth.kinfu_camera_path(i, nf, fr), device="cuda:0").view(torch.int16) for i in range(nf)])
    torch.cuda.synchronize()
    print("device: %s; %d fragments x %d frames of %d x %d, max_units %d" % (torch.cuda.get_device_name(0), nf, fr, cols, rows, a.max_units))

    def baseline():
        od = DepthOdometry(cols, rows, synth.CAM)
        vol = TSDFVolume(cols, rows, cam6, max_units=a.max_units)
        host = synth.to_numpy_u16(depth)                         # track_model takes host frames (the transfer is outside the timing)
        t0 = time.perf_counter()
        Ws, lost = [], 0
        for k in range(nf):
            vol.reset()
            W, S = od.track_model(vol, host[k * fr:(k + 1) * fr], T0=synth.basepose(3.0))
            vol.extract_oriented()
            Ws.append(W)
            lost += int(S.sum())
        dt = time.perf_counter() - t0
        od.close()
        vol.close()
        return np.concatenate(Ws), lost, dt

    def build(lanes, repeat):
        free0 = torch.cuda.mem_get_info(0)[0]
        b = FragmentBuilder(cols, rows, cam6, interval=fr, lanes=lanes, max_units=a.max_units)
        used = free0 - torch.cuda.mem_get_info(0)[0]
        times = []
        for _ in range(repeat):
            t0 = time.perf_counter()
            W, S, frags = b.build(depth)
            times.append(time.perf_counter() - t0)
        lane_bytes = b.lane_bytes()
        b.close()
        return W, S, frags, times, lane_bytes, used

    if a.kernels_only is not None:
        if a.kernels_only == 0:
            _, lost, dt = baseline()
            print("baseline only: %.1f frames/s, %d lost" % (nf * fr / dt, lost))
        else:
            _, S, _, times, _, _ = build(a.kernels_only, 1)
            print("lanes %d only: %.1f frames/s, %d lost" % (a.kernels_only, nf * fr / times[0], int(S.sum())))
        return
    baseline()                                                   # warm-up: code objects, allocator
    Wb, lost_b, dt_b = baseline()
    print("track_model loop (the route the builder replaces): %8.1f frames/s (%.3f s), %d frames lost" % (nf * fr / dt_b, dt_b, lost_b))
    for lanes in [int(x) for x in a.lanes.split(",")]:
        try:
            W, S, frags, times, lane_bytes, used = build(lanes, a.repeat + 1)
        except ErError as e:                                     # (a lane that cannot be allocated is a refusal)
            print("lanes %2d: %s" % (lanes, e))
            continue
        times = times[1:]
        same = np.array_equal(W.view(np.uint64), Wb.view(np.uint64))
        print("lanes %2d: %8.1f frames/s (best of %d; worst %.1f), %.2f x the loop; poses equal the loop's: %s; %d lost; %d points; "
              "first lane %.3f GB, handle %.3f GB" % (lanes, nf * fr / min(times), len(times), nf * fr / max(times), dt_b / min(times), same,
                                                      int(S.sum()), sum(len(x) for x, _ in frags), lane_bytes / 1e9, used / 1e9))


if __name__ == "__main__":
    main()
