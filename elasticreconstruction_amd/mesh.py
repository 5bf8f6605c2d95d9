"""Connected components of an indexed triangle mesh on the GPU (er_mesh_components) and its simplification by vertex
clustering (er_mesh_simplify).  The cleaned and the simplified mesh of a resident volume are TSDFVolume.extract_clean_mesh
and TSDFVolume.extract_simplified_mesh (tsdf.py)."""
import ctypes as C

import numpy as np

from . import _ffi


def components(tris, n_vertices, device=0, rounds=False):
    """Labels the mesh of n_vertices vertices and triangles int32[nt, 3]: -> (labels int32[nv] = the smallest vertex index of each vertex's
    component, counts int64[nv] = the triangles of its component, n_components).  A vertex no triangle names is a component of its own with
    0 triangles.  An index outside [0, n_vertices) is refused with the first offending triangle in the message.  rounds = True appends the
    number of labelling rounds the device needed."""
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    nv = int(n_vertices)
    labels = np.empty(max(nv, 0), dtype=np.int32)
    counts = np.empty(max(nv, 0), dtype=np.int64)
    nc, r = C.c_long(0), C.c_int(0)
    _ffi.check(_ffi.lib().er_mesh_components(_ffi.ptr(t), t.shape[0], nv, int(device), _ffi.ptr(labels), _ffi.ptr(counts), C.byref(nc), C.byref(r)),
               "er_mesh_components")
    return (labels, counts, nc.value, r.value) if rounds else (labels, counts, nc.value)


def simplify(verts, tris, cell, normals=None, colors=None, device=0, probes=False):
    """Vertex clustering of an indexed mesh on the GPU (er_mesh_simplify; the definitions stand in include/er_hip.h): verts float32[nv, 3] or
    [nv, 4] (a fourth column is ignored), tris int32[nt, 3], cell in metres, normals float32[nv, 3] or [nv, 4] or None, colors uint8[nv, 4]
    = r g b a or None.  All vertices of one cell -- floor(p / cell) per axis -- become one vertex at the mean of their positions quantised to
    2^-20 m, with the normalised sum of their finite normals and the rounded mean of their coloured members' colours; triangles with two
    corners in one cluster and repetitions of a triangle (same clusters, same winding) are dropped, clusters no kept triangle names too.
    Returns a dict: verts float32[n, 4] (x y z 0), normals float32[n, 3] or None, colors uint8[n, 4] or None, tris int32[m, 3], cluster
    int32[nv] (the output vertex of every input vertex, or -1), members int32[n], tri_index int32[m] (the input triangle behind each kept
    one), stats = (occupied cells, degenerate triangles dropped, duplicates dropped, cells dropped).  probes = True adds "probes", the longest
    probe sequences of the two hash tables (a diagnostic that depends on arrival order; every other entry is the same bytes on every call)."""
    v = np.asarray(verts, np.float32)
    if v.ndim != 2 or v.shape[1] not in (3, 4):
        raise ValueError("simplify: verts must be [n, 3] or [n, 4], not %s" % (v.shape,))
    nv = v.shape[0]

    def rows4(a, what):
        a = np.asarray(a, np.float32)
        if a.shape not in ((nv, 3), (nv, 4)):
            raise ValueError("simplify: %s must be [%d, 3] or [%d, 4], not %s" % (what, nv, nv, a.shape))
        if a.shape[1] == 3:
            a = np.concatenate([a, np.zeros((nv, 1), np.float32)], axis=1)
        return np.ascontiguousarray(a)

    v = rows4(v, "verts")
    n = None if normals is None else rows4(normals, "normals")
    c = None
    if colors is not None:
        c = np.ascontiguousarray(colors, dtype=np.uint8)
        if c.shape != (nv, 4):
            raise ValueError("simplify: colors must be [%d, 4], not %s" % (nv, c.shape))
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    L = _ffi.lib()
    p = lambda a: None if a is None else _ffi.ptr(a)
    nvo, nto = C.c_long(0), C.c_long(0)
    st, pr = (C.c_long * 4)(0, 0, 0, 0), (C.c_long * 2)(0, 0)

    def call(vo, no, co, mo, cv, to, io, ct, cl):
        _ffi.check(L.er_mesh_simplify(p(v), p(n), p(c), nv, p(t), t.shape[0], C.c_float(cell), int(device), p(vo), p(no), p(co), p(mo), cv, p(to), p(io), ct,
                                      p(cl), C.byref(nvo), C.byref(nto), st, pr), "er_mesh_simplify")

    call(None, None, None, None, 0, None, None, 0, None)
    k, m = nvo.value, nto.value
    vo = np.zeros((k, 4), np.float32)
    no = None if n is None else np.zeros((k, 4), np.float32)
    co = None if c is None else np.zeros((k, 4), np.uint8)
    mo, to, io = np.zeros(k, np.int32), np.zeros((m, 3), np.int32), np.zeros(m, np.int32)
    cl = np.full(nv, -1, np.int32)
    if nv and t.shape[0]:
        call(vo, no, co, mo, k, to, io, m, cl)
    out = dict(verts=vo, normals=None if no is None else np.ascontiguousarray(no[:, :3]), colors=co, tris=to, cluster=cl, members=mo, tri_index=io,
               stats=(st[0], st[1], st[2], st[3]))
    if probes:
        out["probes"] = (pr[0], pr[1])
    return out


def smooth(verts, tris, iterations=10, lam=0.5, mu=-0.53, fix_boundary=False, device=0, probes=False):
    """Taubin lambda|mu smoothing of an indexed mesh on the GPU and the vertex normals of its triangles (er_mesh_smooth; the definitions stand
    in include/er_hip.h): verts float32[nv, 3] or [nv, 4] (a fourth column is ignored), tris int32[nt, 3].  An iteration is a pass with
    factor lam and a pass with factor mu; a pass moves every vertex by its factor towards the mean of its distinct neighbours' positions
    quantised to 2^-20 m (all vertices read the positions the pass started with); a vertex without a neighbour stays, and with fix_boundary
    so does every end of an edge that only one triangle corner pair gives.  mu = 0 is plain Laplacian smoothing; iterations = 0 gives the
    normals of the mesh as it is.  A pass that takes a coordinate to 4096 m or beyond is refused, naming the pass and the vertex.
    Returns a dict: verts float32[nv, 4] (x y z 0), normals float32[nv, 3] (area-weighted, from the triangles at the smoothed positions; NaN
    for a vertex without one), degree int32[nv], boundary uint8[nv], stats = (distinct edges, boundary edges, non-manifold edges, vertices
    that never move).  probes = True adds "probes", the longest probe sequence of the edge table (a diagnostic that depends on arrival
    order; every other entry is the same bytes on every call)."""
    v = np.asarray(verts, np.float32)
    if v.ndim != 2 or v.shape[1] not in (3, 4):
        raise ValueError("smooth: verts must be [n, 3] or [n, 4], not %s" % (v.shape,))
    nv = v.shape[0]
    if v.shape[1] == 3:
        v = np.concatenate([v, np.zeros((nv, 1), np.float32)], axis=1)
    v = np.ascontiguousarray(v)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    vo, no = np.zeros((nv, 4), np.float32), np.zeros((nv, 4), np.float32)
    deg, bnd = np.zeros(nv, np.int32), np.zeros(nv, np.uint8)
    st, pr = (C.c_long * 4)(0, 0, 0, 0), (C.c_long * 1)(0)
    _ffi.check(_ffi.lib().er_mesh_smooth(_ffi.ptr(v), nv, _ffi.ptr(t), t.shape[0], int(iterations), C.c_float(lam), C.c_float(mu), int(bool(fix_boundary)),
                                         int(device), _ffi.ptr(vo), _ffi.ptr(no), _ffi.ptr(deg), _ffi.ptr(bnd), st, pr), "er_mesh_smooth")
    out = dict(verts=vo, normals=np.ascontiguousarray(no[:, :3]), degree=deg, boundary=bnd, stats=(st[0], st[1], st[2], st[3]))
    if probes:
        out["probes"] = pr[0]
    return out
