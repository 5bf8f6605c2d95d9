#!/usr/bin/env python3
"""The mesh output stage on one MI355X (profiles/mesh_output.txt): wall time, call to return, of
  - TSDFVolume.extract_indexed_mesh (er_tsdf_extract_mesh_indexed: vertices, normals, int32 triangles in host arrays),
  - the route that existed before it: TSDFVolume.extract_mesh (the triangle soup) followed by the host-side weld the soup tests use,
    np.unique over the vertex bits,
  - TSDFVolume.LoadWorld of the volume's own SaveWorld list (er_tsdf_import_world, rows already in host memory),
  - bin/MeshOutput on that list as a world.pcd, from process start to exit,
on the volume of the first 200 frames of configs[1] (bench.py's workload, no warp), with the mesh's counts, the PLY's size, the share of
the resident volume's triangles that survive the trip through world.pcd, and the device memory the indexed extraction takes per unit.

usage: python scripts/mesh_probe.py [--frames 200] [--repeat 10]"""
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
    ap.add_argument("--repeat", type=int, default=10)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    from elasticreconstruction_amd import synth
    from elasticreconstruction_amd.tsdf import TSDFVolume
    sc = synth.make_scenario(a.frames, interval=50, warp=False, total_frames=3000, device="cuda:0")
    torch.cuda.synchronize()
    vol = TSDFVolume(max_units=4096)
    vol.IntegrateFrames(None, sc["traj"], None, device_ptr=sc["depth"].data_ptr())
    vol.synchronize()
    units = vol.unit_count()
    print("device: %s; volume: %d frames of configs[1], %d units" % (torch.cuda.get_device_name(0), a.frames, units))

    verts, nrm, tris = vol.extract_indexed_mesh()
    print("indexed mesh: %d vertices, %d triangles; %.1f %% of the vertices without a normal" % (len(verts), len(tris), 100 * np.isnan(nrm).any(1).mean()))
    lo, hi = timed(vol.extract_indexed_mesh, a.repeat)
    print("extract_indexed_mesh (verts, normals, tris)     : %8.2f ms (min of %d; max %.2f)" % (lo, a.repeat, hi))
    lo, hi = timed(vol.extract_mesh, a.repeat)
    print("extract_mesh (the soup alone)                   : %8.2f ms (min of %d; max %.2f)" % (lo, a.repeat, hi))

    def soup_and_weld():
        flat = vol.extract_mesh().reshape(-1, 3)
        return np.unique(flat.view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True)
    uniq, _ = soup_and_weld()
    lo, hi = timed(soup_and_weld, max(a.repeat // 5, 1))
    print("extract_mesh + np.unique weld on the host       : %8.2f ms (min of %d; max %.2f); %d welded vertices (by position: %d fewer)" % (
        lo, max(a.repeat // 5, 1), hi, len(uniq), len(verts) - len(uniq)))
    nslab = units * 64
    print("device temporaries of the indexed extraction    : %.1f KiB per unit (edge bitmap 96, row prefixes 16, slab counts and offsets 2) "
          "+ 16 B per vertex (+ 16 with normals) + 12 B per triangle" % ((nslab * 64 * 3 * 8 + nslab * 64 * 4 + nslab * 4 * 8) / units / 1024.0))

    world = vol.extract_world()
    soup_a = vol.extract_mesh()
    B = TSDFVolume(max_units=max(units, 1))

    def load():
        B.reset()
        return B.LoadWorld(world)
    lo, hi = timed(load, a.repeat)
    t0 = time.perf_counter()
    B.reset()
    t_reset = 1e3 * (time.perf_counter() - t0)
    load()
    print("LoadWorld of the SaveWorld list (%d voxels, %d units) : %8.2f ms (min of %d; max %.2f), of which reset() about %.2f" % (
        len(world), B.unit_count(), lo, a.repeat, hi, t_reset))
    vb, _, tb = B.extract_indexed_mesh()
    rows_a = set(map(bytes, np.ascontiguousarray(soup_a).view(np.uint32).reshape(-1, 9)))
    rows_b = list(map(bytes, np.ascontiguousarray(vb[tb][..., :3]).view(np.uint32).reshape(-1, 9)))
    print("through world.pcd: %d of %d triangles survive (%.2f %%), all of them triangles of the resident volume: %s" % (
        len(rows_b), len(rows_a), 100.0 * len(rows_b) / max(len(rows_a), 1), all(r in rows_a for r in rows_b)))
    B.close()

    with tempfile.TemporaryDirectory() as d:
        vol.SaveWorld(os.path.join(d, "world.pcd"))
        exe = os.path.join(ROOT, "elasticreconstruction_amd", "bin", "MeshOutput")
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = subprocess.run([exe, "world.pcd", "--save_to", "mesh.ply"], cwd=d, capture_output=True, text=True, timeout=600,
                               env=dict(os.environ, ER_TIMING="1"))
            t.append(time.perf_counter() - t0)
            assert r.returncode == 0, r.stdout + r.stderr
        print("bin/MeshOutput world.pcd (%.1f MB) -> mesh.ply (%.1f MB), process start to exit: %8.1f ms (min of 3; max %.1f)" % (
            os.path.getsize(os.path.join(d, "world.pcd")) / 1e6, os.path.getsize(os.path.join(d, "mesh.ply")) / 1e6, 1e3 * min(t), 1e3 * max(t)))
        print(r.stdout.strip())
        print(r.stderr.strip())
        n, m = vol.SaveMesh(os.path.join(d, "resident.ply"))
        print("SaveMesh of the resident volume: %d vertices, %d triangles, %.1f MB binary PLY with normals" % (
            n, m, os.path.getsize(os.path.join(d, "resident.ply")) / 1e6))
    vol.close()


if __name__ == "__main__":
    main()
