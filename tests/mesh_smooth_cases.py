"""The crafted meshes of the smoothing tests.  A case is dict(verts float32[nv, 4], tris int32[nt, 3], iterations, lam, mu,
fix_boundary) -- the arguments of mesh_smooth_restatement.smooth and of mesh.smooth.  What each case is meant to reach is asserted on the
restatement in tests/test_mesh_smooth_cpu.py; the GPU test only compares."""
import numpy as np

from mesh_simplify_cases import random_mesh

SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 4097, 65537]               # block and wave edges, more than one round of the row scan
ITERATIONS = [0, 1, 2, 10]
F = np.float32


def mesh(verts, tris, iterations=2, lam=0.5, mu=-0.53, fix_boundary=False):
    v = np.zeros((len(verts), 4), F)
    v[:, :3] = np.asarray(verts, F).reshape(-1, 3)
    v[:, 3] = 7.0                                                           # (the 4th column is ignored)
    return dict(verts=v, tris=np.ascontiguousarray(tris, np.int32).reshape(-1, 3), iterations=iterations, lam=F(lam), mu=F(mu), fix_boundary=fix_boundary)


def sizes():
    out = {}
    for k, n in enumerate(SIZES):
        m = random_mesh(n, 2 * n, 300 + k)
        for it in ITERATIONS:
            out["nv %d, nt %d, %d iterations" % (n, 2 * n, it)] = mesh(m["verts"][:, :3], m["tris"], it)
    m = random_mesh(257, 65537, 320)
    out["nv 257, nt 65537"] = mesh(m["verts"][:, :3], m["tris"], 2)          # every edge many times over
    m = random_mesh(65537, 63, 321)
    out["nv 65537, nt 63"] = mesh(m["verts"][:, :3], m["tris"], 2)           # nearly every vertex without a neighbour
    m = random_mesh(4097, 0, 322)
    out["nv 4097, nt 0"] = mesh(m["verts"][:, :3], m["tris"], 2)
    return out


def fan(n, closed=False, seed=3, **kw):
    """vertex 0 in the middle, n on a wavy rim: the hub has degree n; open, its two ends and the hub are boundary vertices"""
    rng = np.random.default_rng(seed)
    a = np.arange(n) * (2 * np.pi / n) * (1.0 if closed else 0.75)
    rim = np.stack([np.cos(a), np.sin(a), 0.05 * rng.standard_normal(n)], 1)
    v = np.concatenate([[[0.01, -0.02, 0.3]], rim])
    i = np.arange(1, n)
    tris = np.stack([np.zeros(n - 1, np.int64), i, i + 1], 1)
    if closed:
        tris = np.concatenate([tris, [[0, n, 1]]])
    return mesh(v, tris, **kw)


TETRA = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) * 0.75 + 0.125
TETRA_TRIS = [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]


def tetrahedron(**kw):
    return mesh(TETRA, TETRA_TRIS, **kw)


def grid(nx, ny, step=2.0 ** -10, seed=None, reverse=False, **kw):
    """a planar nx x ny grid in z = 0 at multiples of step, two triangles a square; seed: noise on z; reverse: vertex i becomes nv - 1 - i"""
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    v = np.stack([x.reshape(-1) * step, y.reshape(-1) * step, np.zeros(nx * ny)], 1)
    if seed is not None:
        v[:, 2] = np.random.default_rng(seed).standard_normal(nx * ny) * step * 0.3
    i = (y[:-1, :-1] * nx + x[:-1, :-1]).reshape(-1)
    tris = np.concatenate([np.stack([i, i + 1, i + nx + 1], 1), np.stack([i, i + nx + 1, i + nx], 1)])
    if reverse:
        v, tris = v[::-1], len(v) - 1 - tris
    return mesh(v, tris, **kw)


def few(tris, nv, seed=4, **kw):
    v = np.random.default_rng(seed).uniform(-1, 1, (nv, 3))
    return mesh(v, tris, **kw)


def progressions(stride, m, **kw):
    """triangles (k s, k s + 1, k s + 2) and (0, k s + 1, k s + 2): edge keys min << 32 | max in arithmetic progressions of stride s in the low
    word, and of s (2^32 + 1) in both"""
    k = np.arange(m) * stride
    tris = np.concatenate([np.stack([k, k + 1, k + 2], 1), np.stack([np.zeros(m, np.int64), k + 1, k + 2], 1)[1:]])
    return few(tris, int(k[-1]) + 3, seed=5, **kw)


def negative_zeros():
    """-0.0 in an isolated vertex (it keeps its bits), in a fixed boundary vertex, and in vertices that move"""
    v = np.array([[-0.0, -0.0, -0.0], [-0.0, 0.5, -0.0], [0.5, -0.0, 0.0], [-0.0, -0.0, 0.5], [-0.0, 0.0, -0.0], [0.25, 0.25, -0.0]])
    return mesh(v, [[1, 2, 3], [1, 3, 4], [1, 4, 5]], iterations=3)


def ties():
    """coordinates (2 k + 1) 2^-21 for even and odd k: p 2^20 lies at an exact half"""
    k = np.arange(-40, 40)
    x = ((2 * k + 1) * 2.0 ** -21 + k * 2.0 ** -4).astype(np.float64)
    assert (x.astype(F).astype(np.float64) == x).all()
    v = np.stack([x, x[::-1], np.roll(x, 7)], 1)
    tris = np.random.default_rng(9).integers(0, len(v), (150, 3))
    return mesh(v, tris, iterations=1, mu=0.0)


def cancellation(n=300, seed=11):
    """n stars: a centre at p = q 2^-20 per axis with three neighbours at 2 p, 2 p and 3 p, one pass with the factor -3/4.  The mean is 7 p / 3,
    rounded; the step -3/4 (m - p) cancels p but for that rounding, so p + the ROUNDED product is 0 or an ulp of p, while a fused multiply-add
    keeps the product's own low bits: the two differ in about half the coordinates"""
    q = np.random.default_rng(seed).integers(1, 2 ** 22, (n, 3))
    p = q * 2.0 ** -20
    v = np.concatenate([p, 2 * p, 2 * p, 3 * p])
    i = np.arange(n)
    tris = np.concatenate([np.stack([i, i + n, i + 2 * n], 1), np.stack([i, i + 2 * n, i + 3 * n], 1)])
    return mesh(v, tris, iterations=1, lam=-0.75, mu=0.0)


def icosphere(level=4, radius=0.5, noise=0.01, seed=1):
    """-> (verts float64[n, 3], tris int[m, 3]) of an icosahedron subdivided `level` times, every radius multiplied by 1 + noise N(0, 1)"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, g = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    v = np.array(v)
    r = radius * (1.0 + noise * np.random.default_rng(seed).standard_normal(len(v)))
    return v * r[:, None], np.array(f, np.int64)


def guards():
    """passes that leave the range: name -> (case, pass, vertex)"""
    big = np.nextafter(F(4096.0), F(0.0))
    tri3 = [[0, 1, 2]]
    out = {
        "mu alone": (mesh([[0, 0, 0], [big, 0, 0], [0, -big, 0]], tri3, 3, lam=0.0, mu=-1.0), 1, 1),
        "lambda first": (mesh([[0, 0, 0], [0, 0, 0], [0, -big, big]], tri3, 3, lam=-1.0, mu=0.5), 0, 2),
        "second iteration": (mesh([[0, 0, 0], [0, 1500.0, 0], [0, 0, -1500.0], [1, 1, 1]], [[0, 1, 2], [3, 3, 3]], 8, lam=-0.25, mu=-0.25), None, None),
    }
    v = np.random.default_rng(6).uniform(-1, 1, (4097, 3))
    v[[3000, 2100], 1] = big                                                # two offenders in one pass, in two blocks: the smaller is named
    m = random_mesh(4097, 9000, 41)
    out["two blocks"] = (mesh(v, m["tris"], 2, lam=0.0, mu=-1.0), 1, None)
    return out


def crafted():
    out = {
        "isolated vertex": few([[0, 1, 2], [2, 1, 3]], 6),
        "hub of degree 65536": fan(65536, iterations=2),
        "open fan": fan(9, iterations=3),
        "open fan, boundary fixed": fan(9, iterations=3, fix_boundary=True),
        "closed fan": fan(9, closed=True, iterations=3),
        "closed fan, boundary fixed": fan(9, closed=True, iterations=3, fix_boundary=True),
        "tetrahedron": tetrahedron(iterations=3),
        "tetrahedron, lambda 1": tetrahedron(iterations=1, lam=1.0, mu=0.0),
        "tetrahedron, 1024 iterations": tetrahedron(iterations=1024),
        "two on an edge, equal winding": few([[0, 1, 2], [0, 1, 3]], 4),
        "two on an edge, opposite winding": few([[0, 1, 2], [1, 0, 3]], 4),
        "three on an edge": few([[0, 1, 2], [0, 1, 3], [1, 0, 4]], 5),
        "three on an edge, boundary fixed": few([[0, 1, 2], [0, 1, 3], [1, 0, 4]], 5, fix_boundary=True),
        "duplicated triangle": few([[0, 1, 2], [0, 1, 2], [2, 1, 3]], 4),
        "a a b and a a a": few([[0, 0, 1], [2, 2, 2], [1, 2, 3], [4, 3, 4]], 6),
        "grid": grid(19, 14, seed=7, iterations=10),
        "grid, boundary fixed": grid(19, 14, seed=7, iterations=10, fix_boundary=True),
        "grid in reverse order": grid(19, 14, seed=7, reverse=True, iterations=10),
        "flat grid, boundary fixed": grid(9, 7, iterations=5, fix_boundary=True),
        "progressions, stride 1": progressions(1, 4096),
        "progressions, stride 2^4": progressions(16, 4096),
        "progressions, stride 2^8": progressions(256, 1024),
        "progressions, stride 2^16": progressions(65536, 16, iterations=1),
        "negative zeros": negative_zeros(),
        "negative zeros, boundary fixed": dict(negative_zeros(), fix_boundary=True),
        "ties": ties(),
        "cancellation": cancellation(),
        "mu 0": grid(19, 14, seed=8, iterations=4, mu=0.0),
        "lambda 0": grid(19, 14, seed=8, iterations=4, lam=0.0),
        "lambda 0 and mu 0": grid(19, 14, seed=8, iterations=4, lam=0.0, mu=0.0),
        "lambda 1, mu -1": grid(19, 14, seed=8, iterations=2, lam=1.0, mu=-1.0),
        "icosphere": mesh(*icosphere(), iterations=10),
    }
    return out
