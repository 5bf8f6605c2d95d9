"""Taubin smoothing of an indexed mesh and vertex normals from its triangles in numpy, written from the definitions in
include/er_hip.h above er_mesh_smooth: np.unique on the sorted pairs, np.add.at on int64 sums.  csrc/er_mesh_smooth_math.h and
csrc/er_mesh_smooth.hip are pinned to this file bit for bit.  Nothing here depends on an order of execution."""
import numpy as np

QUANT = np.float64(1 << 20)
QUANT_INV = np.float64(1.0) / QUANT
AREA_QUANT = np.float64(1 << 32)
LIMIT = np.float32(4096.0)
MAX_ITERATIONS = 1024


def rows(a, what="verts"):
    a = np.asarray(a, np.float32)
    if a.ndim != 2 or a.shape[1] not in (3, 4):
        raise ValueError("%s must be [n, 3] or [n, 4], not %s" % (what, a.shape))
    return np.ascontiguousarray(a[:, :3])


def quantise(x):
    """llrint((double)x * 2^20): np.rint rounds half to even"""
    return np.rint(x.astype(np.float64) * QUANT).astype(np.int64)


def position_ok(p):
    with np.errstate(all="ignore"):
        return (np.abs(p) < LIMIT).all(axis=1)


def edges(T):
    """-> (lo int64[e], hi int64[e], multiplicity int64[e]): the distinct unordered pairs of the corners (t, c), (t, (c + 1) % 3) whose two
    entries differ, and how many (t, c) give each"""
    T = np.asarray(T, np.int64).reshape(-1, 3)
    u, w = T.reshape(-1), np.roll(T, -1, axis=1).reshape(-1)
    keep = u != w
    lo, hi = np.minimum(u, w)[keep], np.maximum(u, w)[keep]
    key, mult = np.unique((lo << 32) | hi, return_counts=True)
    return key >> 32, key & 0xFFFFFFFF, mult.astype(np.int64)


def adjacency(T, nv):
    """-> dict(lo, hi, mult, degree int32[nv], boundary uint8[nv])"""
    lo, hi, mult = edges(T)
    deg = (np.bincount(lo, minlength=nv) + np.bincount(hi, minlength=nv)).astype(np.int32)
    b = np.zeros(nv, np.uint8)
    b[lo[mult == 1]] = 1
    b[hi[mult == 1]] = 1
    return dict(lo=lo, hi=hi, mult=mult, degree=deg, boundary=b)


def move(p, S, deg, f):
    """x' = (float)((double)p + (double)f * (m - (double)p)), m = ((double)S / (double)deg) * 2^-20: p float32[n, 3], S int64[n, 3], deg[n] > 0"""
    with np.errstate(all="ignore"):
        p64 = p.astype(np.float64)
        m = (S.astype(np.float64) / deg.astype(np.float64)[:, None]) * QUANT_INV
        d = m - p64
        step = np.float64(np.float32(f)) * d
        return (p64 + step).astype(np.float32)


def one_pass(p, adj, moving, f):
    """Jacobi: every vertex reads p.  p float32[nv, 3] -> float32[nv, 3]"""
    q = quantise(p)
    S = np.zeros(p.shape, np.int64)
    np.add.at(S, adj["lo"], q[adj["hi"]])
    np.add.at(S, adj["hi"], q[adj["lo"]])
    out = p.copy()
    if moving.any():
        out[moving] = move(p[moving], S[moving], adj["degree"][moving], f)
    return out


def area_normals(p, T):
    """k int64[nt, 3] = llrint(cross * 2^32), cross = (b - a) x (c - a) in float64, each product rounded before the subtraction"""
    T = np.asarray(T, np.int64).reshape(-1, 3)
    P = p.astype(np.float64)
    d1, d2 = P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]]
    k = np.zeros((len(T), 3), np.int64)
    for q in range(3):
        r, s = (q + 1) % 3, (q + 2) % 3
        left, right = d1[:, r] * d2[:, s], d1[:, s] * d2[:, r]
        k[:, q] = np.rint((left - right) * AREA_QUANT).astype(np.int64)
    return k


def finish_normal(N):
    g = N.astype(np.float64)
    with np.errstate(all="ignore"):
        length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        out = (g / length[:, None]).astype(np.float32)
    out[length == 0] = np.nan
    return out


def vertex_normals(p, T, nv):
    """float32[nv, 3]: the normalised sum over the corners of every vertex of its triangle's k; the sums wrap in two's complement"""
    T = np.asarray(T, np.int64).reshape(-1, 3)
    N = np.zeros((nv, 3), np.uint64)
    if len(T):
        k = area_normals(p, T).view(np.uint64)
        for c in range(3):
            np.add.at(N, T[:, c], k)
    return finish_normal(N.view(np.int64))


def smooth(verts, tris, iterations=10, lam=0.5, mu=-0.53, fix_boundary=False):
    """-> dict(verts float32[nv, 4] = x y z 0, normals float32[nv, 3], degree int32[nv], boundary uint8[nv], stats = (distinct edges,
    boundary edges, non-manifold edges, vertices that never move)).  Raises ValueError with the device's words for what it refuses."""
    p = rows(verts)
    nv = len(p)
    T = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
    lam, mu = np.float32(lam), np.float32(mu)
    if not 0 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError("iterations = %d, outside [0, %d]" % (iterations, MAX_ITERATIONS))
    for name, f in (("lambda", lam), ("mu", mu)):
        if not (np.isfinite(f) and abs(f) <= 1):
            raise ValueError("%s = %g; it has to be finite and at most 1 in magnitude" % (name, f))
    if nv == 0:
        return dict(verts=np.zeros((0, 4), np.float32), normals=np.zeros((0, 3), np.float32), degree=np.zeros(0, np.int32),
                    boundary=np.zeros(0, np.uint8), stats=(0, 0, 0, 0))
    ok = position_ok(p)
    if not ok.all():
        raise ValueError("vertex %d has a coordinate that is not finite" % int(np.flatnonzero(~ok)[0]))
    bad = ((T < 0) | (T >= nv)).any(axis=1)
    if bad.any():
        t = int(np.flatnonzero(bad)[0])
        i = int(T[t][(T[t] < 0) | (T[t] >= nv)][0])
        raise ValueError("triangle %d names vertex %d, outside [0, %d)" % (t, i, nv))
    adj = adjacency(T, nv)
    still = (adj["degree"] == 0) | ((adj["boundary"] != 0) if fix_boundary else np.zeros(nv, bool))
    number = 0
    for _ in range(int(iterations)):
        for f in (lam, mu):
            if f != 0:
                p = one_pass(p, adj, ~still, f)
                ok = position_ok(p)
                if not ok.all():
                    raise ValueError("pass %d moves vertex %d to a coordinate that is not finite" % (number, int(np.flatnonzero(~ok)[0])))
            number += 1
    out = np.zeros((nv, 4), np.float32)
    out[:, :3] = p
    return dict(verts=out, normals=vertex_normals(p, T, nv), degree=adj["degree"], boundary=adj["boundary"],
                stats=(len(adj["lo"]), int((adj["mult"] == 1).sum()), int((adj["mult"] >= 3).sum()), int(still.sum())))
