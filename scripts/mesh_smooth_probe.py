#!/usr/bin/env python3
"""Mesh smoothing on one MI355X (profiles/mesh_smooth.txt): wall time, call to return, of
  - TSDFVolume.extract_smoothed_mesh (er_tsdf_extract_mesh_smoothed: extraction, adjacency, Taubin passes and triangle normals in device memory),
  - the route that existed before it on the same host: TSDFVolume.extract_indexed_mesh, then the numpy statement of the same definitions
    (tests/mesh_smooth_restatement.py: np.unique on the sorted pairs, np.add.at on int64 sums),
  - TSDFVolume.extract_indexed_mesh alone, for the cost the smoothing adds to the extraction,
on the volume of the first 200 frames of configs[1] (bench.py's workload, no warp).  The build (edge table, rows, normals) and the passes are
told apart by calls that differ only in the number of passes: factors of 0 run none, 10 iterations run 20, 100 run 200.  One untimed call each,
then the routes alternate in one process; minimum and maximum of the repetitions.  Also the counts, the stats and the longest probe sequence.

usage: python scripts/mesh_smooth_probe.py [--frames 200] [--repeat 10] [--iterations 10] [--no_host]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.uint32)[~np.isnan(a)], b.view(np.uint32)[~np.isnan(b)])
    return np.array_equal(a, b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--no_host", action="store_true", help="leave out the host route (a profiler run of the device kernels)")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    import mesh_smooth_restatement as rs
    from elasticreconstruction_amd import mesh, synth
    from elasticreconstruction_amd.tsdf import TSDFVolume
    sc = synth.make_scenario(a.frames, interval=50, warp=False, total_frames=3000, device="cuda:0")
    torch.cuda.synchronize()
    vol = TSDFVolume(max_units=4096)
    vol.IntegrateFrames(None, sc["traj"], None, device_ptr=sc["depth"].data_ptr())
    vol.synchronize()
    full = vol.extract_indexed_mesh()
    nv, nt = len(full[0]), len(full[2])
    print("device: %s; volume: %d frames of configs[1], %d units; mesh: %d vertices, %d triangles" % (torch.cuda.get_device_name(0), a.frames, vol.unit_count(), nv, nt))
    n = a.iterations
    got = vol.extract_smoothed_mesh(n, stats=True)
    alone = mesh.smooth(full[0], full[2], n, probes=True)
    print("%d iterations: stats (edges, boundary edges, non-manifold edges, vertices held) = %s; mean degree %.2f, largest %d; longest probe sequence %d of %d slots"
          % (n, got[3][:4], alone["degree"].mean(), alone["degree"].max(), alone["probes"], 1 << int(np.ceil(np.log2(max(6 * nt, 2))))))
    moved = np.linalg.norm(got[0][:, :3].astype(np.float64) - full[0][:, :3], axis=1)
    print("displacement of a vertex: mean %.3f mm, largest %.3f mm (a voxel is %.3f mm)" % (1e3 * moved.mean(), 1e3 * moved.max(), 1e3 * 3.0 / 512.0))

    def host():
        m = vol.extract_indexed_mesh()
        return rs.smooth(m[0], m[2], n)

    routes = [("extract_indexed_mesh alone", vol.extract_indexed_mesh),
              ("extract_smoothed_mesh, factors 0: build and normals, no pass", lambda: vol.extract_smoothed_mesh(n, lam=0.0, mu=0.0)),
              ("extract_smoothed_mesh, %d iterations" % n, lambda: vol.extract_smoothed_mesh(n)),
              ("extract_smoothed_mesh, %d iterations" % (10 * n), lambda: vol.extract_smoothed_mesh(10 * n)),
              ("mesh.smooth of host arrays, %d iterations" % n, lambda: mesh.smooth(full[0], full[2], n))]
    if not a.no_host:
        want = host()
        assert equal(got[0], want["verts"]) and equal(got[1], want["normals"]) and equal(got[2], full[2]) and got[3][:4] == want["stats"]
        routes.append(("extract_indexed_mesh + numpy restatement on the host, %d iterations" % n, host))
    for _, fn in routes:
        fn()                                                   # (one untimed call each)
    t = {name: [] for name, _ in routes}
    for _ in range(a.repeat):                                  # the routes alternate
        for name, fn in routes:
            t0 = time.perf_counter()
            fn()
            t[name].append(1e3 * (time.perf_counter() - t0))
    for name, _ in routes:
        print("  %-72s: %8.2f ms (min of %d; max %.2f)" % (name, min(t[name]), a.repeat, max(t[name])))
    lo = min(t[routes[2][0]])
    hi = min(t[routes[3][0]])
    # (extract_smoothed_mesh asks twice, counts then arrays, as extract_indexed_mesh does; only the second call smooths)
    per_pass = (hi - lo) / (2.0 * 9 * n)
    print("one pass: %.1f us = %.3f ns per vertex (from the difference of the two iteration counts, %d passes)" % (1e3 * per_pass, 1e6 * per_pass / nv, 18 * n))
    print("build and normals: %.2f ms over the extraction alone; %d iterations: %.2f ms over the extraction alone"
          % (min(t[routes[1][0]]) - min(t[routes[0][0]]), n, lo - min(t[routes[0][0]])))
    vol.close()
    print("device memory of the smoothing: per triangle 12 (slots) + 24 (row entries), 8 per table slot (6 to 12 slots per triangle); per vertex 4 (degree) + 1 "
          "(boundary) + 4 (row start) + 4 (cursor) + 2 x 16 (positions) + 32 (normal sums) + 16 (normals), next to the unsmoothed mesh")


if __name__ == "__main__":
    main()
