#!/usr/bin/env python3
"""Colour on one MI355X (profiles/color.txt): wall time, call to return, on the first 200 frames of configs[1] (bench.py's workload) of
  - TSDFVolume.ColorFrames per 640 x 480 frame, rigid and under the control-grid warp, beside IntegrateFrames of the same frames in the same run
    (device-resident frames, each call synchronised),
  - TSDFVolume.sample_colors on the mesh vertices and the coloured extract_indexed_mesh, against the uncoloured call,
  - bin/Integrate --save_mesh with and without --color_raw, from process start to exit.
Nothing here is a target: nobody had measured any of it before.

usage: python scripts/color_probe.py [--frames 200] [--repeat 5]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    from elasticreconstruction_amd import formats, synth
    from elasticreconstruction_amd.tsdf import TSDFVolume
    n = a.frames
    print("device: %s; %d frames of configs[1], 640 x 480" % (torch.cuda.get_device_name(0), n))
    for warped in (False, True):
        sc = synth.make_scenario(n, interval=50, warp=warped, total_frames=3000, device="cuda:0")
        world = synth.circle_trajectory(3000, revolutions=1.0)[:n]
        depth, rgb = synth.render_rgbd(world, device="cuda:0")
        assert torch.equal(depth, sc["depth"])
        torch.cuda.synchronize()
        warp = synth.warp_arrays(sc) if warped else None
        probe = TSDFVolume(max_units=4096)
        probe.IntegrateFrames(None, sc["traj"], warp, device_ptr=depth.data_ptr())
        units = probe.unit_count()
        probe.close()
        vol = TSDFVolume(max_units=units + 16)
        vol.enable_color()

        def integrate():
            vol.reset()
            vol.IntegrateFrames(None, sc["traj"], warp, device_ptr=depth.data_ptr())
            vol.synchronize()

        def reset_only():
            vol.reset()
            vol.synchronize()
        lo_r, _ = timed(reset_only, a.repeat)
        lo_i, hi_i = timed(integrate, a.repeat)
        stats = []

        def color():
            stats.append(vol.ColorFrames(None, None, sc["traj"], warp, device_ptrs=(depth.data_ptr(), rgb.data_ptr())))
        lo_c, hi_c = timed(color, a.repeat)
        tag = "warped" if warped else "rigid "
        print("%s: %d units (%.1f GiB of colour accumulators); reset() alone %.2f ms" % (tag, units, (units + 16) * 4 / 1024.0, lo_r))
        print("%s: reset + IntegrateFrames + synchronize : %8.2f ms (min of %d; max %.2f) = %.3f ms a frame" % (tag, lo_i, a.repeat, hi_i, (lo_i - lo_r) / n))
        print("%s: ColorFrames                           : %8.2f ms (min of %d; max %.2f) = %.3f ms a frame; added, no_unit, out_of_range = %s" % (
            tag, lo_c, a.repeat, hi_c, lo_c / n, stats[-1]))
        if not warped:
            verts, nrm, tris = vol.extract_indexed_mesh()
            lo_m, hi_m = timed(vol.extract_indexed_mesh, a.repeat)
            lo_s, hi_s = timed(lambda: vol.sample_colors(verts), a.repeat)
            lo_cm, hi_cm = timed(lambda: vol.extract_indexed_mesh(colors=True), a.repeat)
            rgba, counts = vol.sample_colors(verts, counts=True)
            print("mesh: %d vertices, %d triangles; coloured at level 0: %d, at level 1: %d, uncoloured: %d (%.3f %%)" % (
                len(verts), len(tris), counts[0], counts[1], len(verts) - sum(counts), 100.0 * (len(verts) - sum(counts)) / max(len(verts), 1)))
            print("extract_indexed_mesh                          : %8.2f ms (min of %d; max %.2f)" % (lo_m, a.repeat, hi_m))
            print("sample_colors of its vertices                 : %8.2f ms (min of %d; max %.2f)" % (lo_s, a.repeat, hi_s))
            print("extract_indexed_mesh(colors=True)             : %8.2f ms (min of %d; max %.2f)" % (lo_cm, a.repeat, hi_cm))
            with tempfile.TemporaryDirectory() as d:
                F = [formats.FramedTransformation(i, i, i + 1, sc["traj"][min(i, n - 1)]) for i in range(n + 1)]
                formats.save_log(os.path.join(d, "traj.log"), F)
                synth.to_numpy_u16(depth).tofile(os.path.join(d, "frames.raw"))
                rgb.cpu().numpy().tofile(os.path.join(d, "colour.raw"))
                exe = os.path.join(ROOT, "elasticreconstruction_amd", "bin", "Integrate")
                base = [exe, "--ref_traj", "traj.log", "-oni", "frames.raw", "--max_units", str(units + 16), "--save_mesh", "mesh.ply"]
                for name, extra in (("without colour", []), ("with --color_raw", ["--color_raw", "colour.raw"])):
                    t = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        r = subprocess.run(base + extra, cwd=d, capture_output=True, text=True, timeout=900)
                        t.append(time.perf_counter() - t0)
                        assert r.returncode == 0, r.stdout + r.stderr
                    print("bin/Integrate --save_mesh %-17s, process start to exit: %8.1f ms (min of 3; max %.1f); mesh.ply %.1f MB" % (
                        name, 1e3 * min(t), 1e3 * max(t), os.path.getsize(os.path.join(d, "mesh.ply")) / 1e6))
                v, t_, nr, c = formats.load_ply_colors(os.path.join(d, "mesh.ply"))
                err = np.abs(c[:, :3].astype(np.float64) - synth.texture(v.astype(np.float64))).max(axis=1)[c[:, 3] == 255]
                print("the coloured mesh.ply through load_ply_colors: %d vertices, %.3f %% coloured, max |colour - texture at the vertex| = %.2f levels" % (
                    len(v), 100.0 * (c[:, 3] == 255).mean(), err.max()))
        vol.close()


if __name__ == "__main__":
    main()
