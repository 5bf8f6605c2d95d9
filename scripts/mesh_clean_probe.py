#!/usr/bin/env python3
"""Mesh cleaning on one MI355X (profiles/mesh_clean.txt): wall time, call to return, of
  - TSDFVolume.extract_clean_mesh (er_tsdf_extract_mesh_cleaned: extraction, labelling, selection and compaction in device memory),
  - the route that existed before it on the same host: TSDFVolume.extract_indexed_mesh, scipy.sparse.csgraph.connected_components over the
    index list, then the numpy filter and re-index,
  - TSDFVolume.extract_indexed_mesh alone, for the cost the cleaning adds to the extraction,
on the volume of the first 200 frames of configs[1] (bench.py's workload, no warp) as it is and with a few thousand seeded voxels planted in
observed free space, so that there is something to drop.  One untimed call each, then the two routes alternate in one process; minimum and
maximum of the repetitions.  Also: the labelling rounds the device needs on these meshes and on the index lists of
tests/mesh_components_cases.py, and the device memory of the cleaning per vertex and per triangle.

usage: python scripts/mesh_clean_probe.py [--frames 200] [--repeat 10] [--plant 4000] [--min_triangles 9] [--no_host] [--no_lists]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_route(vol, min_triangles, largest_only):
    """What a user of extract_indexed_mesh had to do: components by scipy, the filter and the re-index by numpy."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    verts, nrm, tris = vol.extract_indexed_mesh()
    nv = len(verts)
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]]])
    n, lab = connected_components(coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(nv, nv)), directed=False)
    per = np.bincount(lab[tris[:, 0]], minlength=n)
    keep_c = per >= min_triangles
    if largest_only:
        first = np.full(n, nv, np.int64)
        np.minimum.at(first, lab, np.arange(nv))
        best = np.lexsort((first, -per))[0]
        keep_c &= np.arange(n) == best
    keep = keep_c[lab]
    new = np.cumsum(keep) - keep
    index = np.flatnonzero(keep).astype(np.int32)
    return verts[index], nrm[index], new[tris[keep[tris[:, 0]]]].astype(np.int32), index


def plant(vol, count, seed):
    """Flips up to `count` seeded voxels to sdf -0.5: interior voxels of their unit whose 3 x 3 x 3 neighbourhood is observed free space
    (weight != 0, sdf > 0), at least 3 voxels apart.  Returns the number planted."""
    import torch
    rng = np.random.default_rng(seed)
    keys = vol.unit_keys()
    per_unit = max(1, count // max(len(keys), 1) + 1)
    done, changed_keys, planes = 0, [], []
    for key in keys:
        if done >= count:
            break
        s, w = (a.reshape(64, 64, 64).copy() for a in vol.read_unit(int(key)))
        free = (w != 0) & (s > 0)
        ok = free[1:-1, 1:-1, 1:-1].copy()
        for di in range(3):
            for dj in range(3):
                for dk in range(3):
                    ok &= free[di:di + 62, dj:dj + 62, dk:dk + 62]
        cand = np.argwhere(ok) + 1
        if not len(cand):
            continue
        taken = np.zeros((64, 64, 64), bool)
        n_here = 0
        for i, j, k in cand[rng.permutation(len(cand))[:8 * per_unit]]:
            if n_here >= per_unit or done >= count:
                break
            if taken[max(i - 3, 0):i + 4, max(j - 3, 0):j + 4, max(k - 3, 0):k + 4].any():
                continue
            taken[i, j, k] = True
            s[i, j, k] = np.float32(-0.5)
            n_here += 1
            done += 1
        if n_here:
            changed_keys.append(int(key))
            planes.append(np.stack([s.reshape(-1), w.reshape(-1)]))
    if changed_keys:
        buf = torch.from_numpy(np.stack(planes).astype(np.float32)).to("cuda:0")
        torch.cuda.synchronize()
        vol.import_raw(np.array(changed_keys, np.int32), buf.data_ptr())
        vol.synchronize()
    return done


def measure(vol, what, a):
    from elasticreconstruction_amd import mesh
    verts, nrm, tris = vol.extract_indexed_mesh()
    labels, counts, n, rounds = mesh.components(tris, len(verts), rounds=True)
    sizes = np.sort(counts[labels == np.arange(len(verts))])
    print("%s: %d vertices, %d triangles, %d components (the largest %d triangles, %d of fewer than %d), %d labelling rounds" % (
        what, len(verts), len(tris), n, sizes[-1] if len(sizes) else 0, int((sizes < a.min_triangles).sum()), a.min_triangles, rounds))
    got = vol.extract_clean_mesh(a.min_triangles, stats=True)
    print("  extract_clean_mesh(min_triangles = %d): %d vertices, %d triangles; stats (found, kept, vertices dropped, triangles dropped) = %s" % (
        a.min_triangles, len(got[0]), len(got[2]), got[4]))
    routes = [("extract_clean_mesh", lambda: vol.extract_clean_mesh(a.min_triangles)), ("extract_indexed_mesh alone", vol.extract_indexed_mesh)]
    if not a.no_host:
        want = host_route(vol, a.min_triangles, False)
        assert all(np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)) for x, y in zip(got[:4], want))
        routes.append(("extract_indexed_mesh + scipy + numpy on the host", lambda: host_route(vol, a.min_triangles, False)))
    for _, fn in routes:
        fn()                                                   # (one untimed call each)
    t = {name: [] for name, _ in routes}
    for _ in range(a.repeat):                                  # the routes alternate
        for name, fn in routes:
            t0 = time.perf_counter()
            fn()
            t[name].append(1e3 * (time.perf_counter() - t0))
    for name, _ in routes:
        print("  %-50s: %8.2f ms (min of %d; max %.2f)" % (name, min(t[name]), a.repeat, max(t[name])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--plant", type=int, default=4000)
    ap.add_argument("--min_triangles", type=int, default=9)
    ap.add_argument("--no_host", action="store_true", help="leave out the host route (a profiler run of the device kernels)")
    ap.add_argument("--no_lists", action="store_true", help="leave out the index lists of tests/mesh_components_cases.py")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    from elasticreconstruction_amd import mesh, synth
    from elasticreconstruction_amd.tsdf import TSDFVolume
    sc = synth.make_scenario(a.frames, interval=50, warp=False, total_frames=3000, device="cuda:0")
    torch.cuda.synchronize()
    vol = TSDFVolume(max_units=4096)
    vol.IntegrateFrames(None, sc["traj"], None, device_ptr=sc["depth"].data_ptr())
    vol.synchronize()
    print("device: %s; volume: %d frames of configs[1], %d units" % (torch.cuda.get_device_name(0), a.frames, vol.unit_count()))
    measure(vol, "the volume as integrated", a)
    n = plant(vol, a.plant, seed=7)
    measure(vol, "with %d planted voxels" % n, a)
    vol.close()
    print("device memory of the cleaning: 16 B per vertex (label 4, triangles per root 8, new index 4) + 4 B per kept vertex (index) + 16 B per kept "
          "vertex and array (vertices, normals) + 12 B per kept triangle + 32 B per 256 vertices and 16 B per 256 triangles (block counts and offsets), "
          "next to the unfiltered mesh (16 + 16 B per vertex, 12 B per triangle) and the extraction's temporaries")
    if not a.no_lists:
        import mesh_components_cases as cases
        for name, (tris, nv) in sorted(cases.index_lists().items()):
            r = mesh.components(tris, nv, rounds=True)
            print("rounds: %-40s %6d triangles %6d vertices %6d components: %d" % (name, len(tris), nv, r[2], r[3]))


if __name__ == "__main__":
    main()
