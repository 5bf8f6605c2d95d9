"""numpy restatement of the definitions above er_mesh_components in include/er_hip.h: a union-find over the index list, the
filter and the re-index.  Independent of the device's algorithm (which hooks and jumps labels in rounds).

  components(tris, nv)             -> labels int32[nv] (the smallest vertex index of each vertex's component), counts int64[nv] (the
                                      triangles of its component, duplicates counted as often as they occur), n_components
  keep_vertices(labels, counts, min_triangles, largest_only) -> bool[nv]
  clean(tris, nv, min_triangles, largest_only) -> index int32[n] (unfiltered index of each kept vertex), tris int32[m, 3] re-indexed,
                                      stats = (components found, components kept, vertices dropped, triangles dropped)
"""
import numpy as np


def components(tris, nv):
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    parent = list(range(nv))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in tris.tolist():
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:                                     # the smaller root stays the root: a root is its component's smallest vertex
                parent[max(rx, ry)] = min(rx, ry)
    labels = np.array([find(v) for v in range(nv)], np.int32).reshape(nv)
    per_root = np.bincount(labels[tris[:, 0]], minlength=nv).astype(np.int64) if len(tris) else np.zeros(nv, np.int64)
    counts = per_root[labels] if nv else np.zeros(0, np.int64)
    return labels, counts, int((labels == np.arange(nv)).sum())


def keep_vertices(labels, counts, min_triangles, largest_only):
    assert min_triangles >= 0
    keep = counts >= min_triangles
    if largest_only and len(labels):
        roots = np.flatnonzero(labels == np.arange(len(labels)))
        best = roots[np.lexsort((roots, -counts[roots]))[0]]         # the most triangles; a tie goes to the smaller label
        keep &= labels == best
    return keep


def clean(tris, nv, min_triangles=0, largest_only=False, comps=None):
    """comps: components(tris, nv) if the caller has it already (a test that filters one mesh many times)."""
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    labels, counts, found = comps if comps is not None else components(tris, nv)
    keep = keep_vertices(labels, counts, min_triangles, largest_only)
    index = np.flatnonzero(keep).astype(np.int32)
    new = np.cumsum(keep) - keep                             # the number of kept vertices before each vertex
    tkeep = keep[tris].all(axis=1) if len(tris) else np.zeros(0, bool)
    out = new[tris[tkeep]].astype(np.int32).reshape(-1, 3)
    kept = int((keep & (labels == np.arange(nv))).sum())
    return index, out, (found, kept, int(nv - len(index)), int(len(tris) - len(out)))
