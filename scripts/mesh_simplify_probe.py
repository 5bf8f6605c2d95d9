#!/usr/bin/env python3
"""Mesh simplification on one MI355X (profiles/mesh_simplify.txt): wall time, call to return, of
  - TSDFVolume.extract_simplified_mesh (er_tsdf_extract_mesh_simplified: extraction and vertex clustering in device memory),
  - the route that existed before it on the same host: TSDFVolume.extract_indexed_mesh, then the numpy statement of the same definitions
    (tests/mesh_simplify_restatement.py: np.unique on the cell keys, np.add.at on int64 sums),
  - TSDFVolume.extract_indexed_mesh alone, for the cost the clustering adds to the extraction,
on the volume of the first 200 frames of configs[1] (bench.py's workload, no warp), coloured from every 8th frame, at cells of 2 and 4 voxels,
without and with colours.  One untimed call each, then the routes alternate in one process; minimum and maximum of the repetitions.  Also:
the counts and stats, the share of vertices without colour before and after, and the longest probe sequences of the two hash tables.

usage: python scripts/mesh_simplify_probe.py [--frames 200] [--repeat 10] [--cells 2 4] [--no_host]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
UL = 3.0 / 512.0


def equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.uint32)[~np.isnan(a)], b.view(np.uint32)[~np.isnan(b)])
    return np.array_equal(a, b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0], help="in voxels of 3/512 m")
    ap.add_argument("--no_host", action="store_true", help="leave out the host route (a profiler run of the device kernels)")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    import mesh_simplify_restatement as rs
    from elasticreconstruction_amd import mesh, synth
    from elasticreconstruction_amd.tsdf import TSDFVolume
    sc = synth.make_scenario(a.frames, interval=50, warp=False, total_frames=3000, device="cuda:0")
    torch.cuda.synchronize()
    vol = TSDFVolume(max_units=4096)
    vol.IntegrateFrames(None, sc["traj"], None, device_ptr=sc["depth"].data_ptr())
    vol.synchronize()
    vol.enable_color()
    every = sc["traj"][::8]
    dt, ct = synth.render_rgbd(every, device="cuda:0")
    vol.ColorFrames(synth.to_numpy_u16(dt), ct.cpu().numpy(), every)
    full = vol.extract_indexed_mesh(colors=True)
    print("device: %s; volume: %d frames of configs[1], %d units, coloured from %d frames" % (torch.cuda.get_device_name(0), a.frames, vol.unit_count(), len(every)))
    print("unsimplified: %d vertices, %d triangles, %.2f %% of the vertices without colour" % (len(full[0]), len(full[2]), 100.0 * (full[3][:, 3] == 0).mean()))

    def timed(routes):
        for _, fn in routes:
            fn()                                               # (one untimed call each)
        t = {name: [] for name, _ in routes}
        for _ in range(a.repeat):                              # the routes alternate
            for name, fn in routes:
                t0 = time.perf_counter()
                fn()
                t[name].append(1e3 * (time.perf_counter() - t0))
        for name, _ in routes:
            print("  %-64s: %8.2f ms (min of %d; max %.2f)" % (name, min(t[name]), a.repeat, max(t[name])))

    for k in a.cells:
        cell = float(np.float32(k * UL))
        got = vol.extract_simplified_mesh(cell, colors=True, stats=True)
        probes = mesh.simplify(full[0], full[2], cell, probes=True)["probes"]
        print("cell %g voxels = %.6f m: %d vertices, %d triangles; stats (cells, degenerate, duplicates, cells dropped) = %s; %.2f %% of the "
              "vertices without colour; longest probe sequences (vertex table, triangle table) = %s" % (
                  k, cell, len(got[0]), len(got[2]), got[4][:4], 100.0 * (got[3][:, 3] == 0).mean() if len(got[3]) else 0.0, probes))

        def host(colors):
            m = vol.extract_indexed_mesh(colors=colors)
            return rs.simplify(m[0], m[2], cell, m[1], m[3] if colors else None)

        routes = [("extract_simplified_mesh", lambda: vol.extract_simplified_mesh(cell)),
                  ("extract_simplified_mesh, colours", lambda: vol.extract_simplified_mesh(cell, colors=True)),
                  ("extract_indexed_mesh alone", vol.extract_indexed_mesh),
                  ("extract_indexed_mesh with colours alone", lambda: vol.extract_indexed_mesh(colors=True))]
        if not a.no_host:
            want = host(True)
            assert equal(got[0], want["verts"]) and equal(got[1], want["normals"]) and equal(got[2], want["tris"]) and equal(got[3], want["colors"])
            assert got[4][:4] == want["stats"]
            routes += [("extract_indexed_mesh + numpy restatement on the host", lambda: host(False)),
                       ("extract_indexed_mesh with colours + numpy restatement on the host", lambda: host(True))]
        timed(routes)
    vol.close()
    print("device memory of the clustering: per vertex 4 (slot) + 4 (lead) + 4 (used) + 4 (rank) + 32 (position sums) + 32 each for normal and colour "
          "sums where asked for, 4 per table slot (2 to 4 slots per vertex and per triangle), 4 per triangle (slot), next to the unsimplified mesh")


if __name__ == "__main__":
    main()
