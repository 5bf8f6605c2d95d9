"""Vertex clustering of an indexed mesh in numpy, written from the definitions in include/er_hip.h above er_mesh_simplify:
np.unique on the cell keys, np.add.at on int64 sums.  csrc/er_mesh_simplify_math.h and csrc/er_mesh_simplify.hip are pinned to this file bit
for bit.  Nothing here depends on an order of execution."""
import numpy as np

BIAS = 1 << 20
QUANT = np.float64(1 << 20)
LIMIT = np.float32(4096.0)


def rows(a, n, what):
    a = np.asarray(a, np.float32)
    if a.shape not in ((n, 3), (n, 4)):
        raise ValueError("%s must be [%d, 3] or [%d, 4], not %s" % (what, n, n, a.shape))
    return np.ascontiguousarray(a[:, :3])


def cells(p, cell):
    """c_a = floor((double)p_a / (double)cell) as float64[n, 3]"""
    with np.errstate(all="ignore"):
        return np.floor(p.astype(np.float64) / np.float64(np.float32(cell)))


def offences(p, cell):
    """int[n]: 0 fine, 1 a coordinate that is not finite or not below 4096 in magnitude, 2 a cell index outside [-2^20, 2^20)"""
    with np.errstate(all="ignore"):
        bad1 = ~(np.abs(p) < LIMIT).all(axis=1)
        c = cells(p, cell)
        bad2 = ~((c >= -BIAS) & (c < BIAS)).all(axis=1)
    return np.where(bad1, 1, np.where(bad2, 2, 0))


def keys(p, cell):
    c = cells(p, cell).astype(np.int64) + BIAS
    return (c[:, 0].astype(np.uint64) << np.uint64(42)) | (c[:, 1].astype(np.uint64) << np.uint64(21)) | c[:, 2].astype(np.uint64)


def quantise(x):
    """llrint((double)x * 2^20): np.rint rounds half to even"""
    return np.rint(x.astype(np.float64) * QUANT).astype(np.int64)


def canonical(T):
    """the rotation of every row with its smallest entry first"""
    T = np.asarray(T)
    k = np.argmin(T, axis=1)
    i = (k[:, None] + np.arange(3)[None, :]) % 3
    return np.take_along_axis(T, i, axis=1)


def finish_normal(N, count):
    g = N.astype(np.float64)
    with np.errstate(all="ignore"):
        length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        out = (g / length[:, None]).astype(np.float32)
    out[(count == 0) | (length == 0)] = np.nan
    return out


def finish_color(sums, m):
    out = np.zeros((len(m), 4), np.uint8)
    has = m > 0
    out[has, :3] = ((2 * sums[has] + m[has, None]) // (2 * m[has, None])).astype(np.uint8)
    out[has, 3] = 255
    return out


def simplify(verts, tris, cell, normals=None, colors=None):
    """-> dict(verts float32[n, 4], normals float32[n, 3] | None, colors uint8[n, 4] | None, tris int32[m, 3], cluster int32[nv], members
    int32[n], tri_index int32[m], stats).  Raises ValueError with the device's words for a refused vertex or triangle."""
    v = np.asarray(verts, np.float32)
    nv = v.shape[0]
    p = rows(v, nv, "verts")
    nr = None if normals is None else rows(normals, nv, "normals")
    co = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(nv, 4)
    T = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
    nt = len(T)
    cell = np.float32(cell)
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError("cell = %g m; it has to be finite and above 0" % cell)
    empty = dict(verts=np.zeros((0, 4), np.float32), normals=None if nr is None else np.zeros((0, 3), np.float32),
                 colors=None if co is None else np.zeros((0, 4), np.uint8), tris=np.zeros((0, 3), np.int32), cluster=np.full(nv, -1, np.int32),
                 members=np.zeros(0, np.int32), tri_index=np.zeros(0, np.int32), stats=(0, 0, 0, 0))
    if nv == 0 or nt == 0:
        return empty
    off = offences(p, cell)
    if off.any():
        w = int(np.flatnonzero(off)[0])
        raise ValueError("vertex %d %s" % (w, "has a coordinate that is not finite" if off[w] == 1 else "lies in cell outside"))
    bad = ((T < 0) | (T >= nv)).any(axis=1)
    if bad.any():
        t = int(np.flatnonzero(bad)[0])
        i = int(T[t][(T[t] < 0) | (T[t] >= nv)][0])
        raise ValueError("triangle %d names vertex %d, outside [0, %d)" % (t, i, nv))

    # clusters and their leads
    _, inv = np.unique(keys(p, cell), return_inverse=True)
    inv = inv.reshape(-1)
    ncell = int(inv.max()) + 1
    lead_of_cell = np.full(ncell, nv, np.int64)
    np.minimum.at(lead_of_cell, inv, np.arange(nv))
    lead = lead_of_cell[inv]                                   # per vertex

    # triangles
    L = lead[T]
    degenerate = (L[:, 0] == L[:, 1]) | (L[:, 1] == L[:, 2]) | (L[:, 0] == L[:, 2])
    live = np.flatnonzero(~degenerate)
    keep = np.zeros(nt, bool)
    if len(live):
        _, first = np.unique(canonical(L[live]), axis=0, return_index=True)
        keep[live[first]] = True                               # (np.unique's index is that of the first occurrence)
    tri_index = np.flatnonzero(keep)

    # vertices: the clusters a kept triangle names, by ascending lead
    out_leads = np.unique(L[keep])
    rank_of_lead = np.full(nv, -1, np.int64)
    rank_of_lead[out_leads] = np.arange(len(out_leads))
    cluster = rank_of_lead[lead].astype(np.int32)
    cell_of_out = inv[out_leads]

    S = np.zeros((ncell, 3), np.int64)
    np.add.at(S, inv, quantise(p))
    n = np.bincount(inv, minlength=ncell).astype(np.int64)
    pos = np.zeros((len(out_leads), 4), np.float32)
    pos[:, :3] = ((S[cell_of_out].astype(np.float64) / n[cell_of_out].astype(np.float64)[:, None]) * (1.0 / QUANT)).astype(np.float32)
    out = dict(empty, verts=pos, tris=rank_of_lead[L[keep]].astype(np.int32).reshape(-1, 3), cluster=cluster,
               members=n[cell_of_out].astype(np.int32), tri_index=tri_index.astype(np.int32),
               stats=(ncell, int(degenerate.sum()), int(len(live) - keep.sum()), ncell - len(out_leads)))
    if nr is not None:
        with np.errstate(all="ignore"):
            contributes = (np.abs(nr) < LIMIT).all(axis=1)
        N = np.zeros((ncell, 3), np.int64)
        np.add.at(N, inv[contributes], quantise(nr[contributes]))
        count = np.bincount(inv[contributes], minlength=ncell)
        out["normals"] = finish_normal(N[cell_of_out], count[cell_of_out])
    if co is not None:
        has = co[:, 3] != 0
        sums = np.zeros((ncell, 3), np.int64)
        np.add.at(sums, inv[has], co[has, :3].astype(np.int64))
        m = np.bincount(inv[has], minlength=ncell).astype(np.int64)
        out["colors"] = finish_color(sums[cell_of_out], m[cell_of_out])
    return out
