"""The crafted meshes of the vertex-clustering tests.  A case is dict(verts float32[nv, 4], tris int32[nt, 3], cell, normals
float32[nv, 4] | None, colors uint8[nv, 4] | None).  What each case is meant to reach is asserted on the restatement in
tests/test_mesh_simplify_cpu.py; the GPU test only compares."""
import numpy as np

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4096, 4097, 65536, 65537]       # block, wave and table-size edges
F = np.float32


def mesh(verts, tris, cell, normals=None, colors=None):
    v = np.zeros((len(verts), 4), F)
    v[:, :3] = np.asarray(verts, F).reshape(-1, 3)
    v[:, 3] = 7.0                                                           # (the 4th column is ignored)
    n = None
    if normals is not None:
        n = np.zeros((len(verts), 4), F)
        n[:, :3] = np.asarray(normals, F).reshape(-1, 3)
    c = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
    return dict(verts=v, tris=np.ascontiguousarray(tris, np.int32).reshape(-1, 3), cell=F(cell), normals=n, colors=c)


def random_mesh(nv, nt, seed, per_cell=4.0):
    """nv vertices in [-1, 1)^3, about per_cell of them to a cell; random triangles; normals with NaN and infinite members, colours with a == 0."""
    rng = np.random.default_rng(seed)
    side = max(1, int(round((max(nv, 1) / per_cell) ** (1.0 / 3.0))))
    verts = rng.uniform(-1, 1, (nv, 3)).astype(F)
    tris = rng.integers(0, max(nv, 1), (nt, 3)).astype(np.int32) if nv else np.zeros((0, 3), np.int32)
    nrm = rng.normal(size=(nv, 3)).astype(F)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), F(1e-6))
    if nv:
        nrm[rng.integers(0, nv, nv // 8)] = np.nan
        nrm[rng.integers(0, nv, nv // 32), 1] = np.inf
    col = rng.integers(0, 256, (nv, 4)).astype(np.uint8)
    col[:, 3] = np.where(rng.integers(0, 4, nv) == 0, 0, 255)
    return mesh(verts, tris, 2.0 / side, nrm, col)


def sizes():
    out = {}
    for k, n in enumerate(SIZES):
        out["nv %d, nt %d" % (n, n)] = random_mesh(n, n, 100 + k)
    out["nv 257, nt 65537"] = random_mesh(257, 65537, 120, per_cell=2.0)     # many duplicates
    out["nv 65537, nt 63"] = random_mesh(65537, 63, 121)
    out["nv 1, nt 4097"] = random_mesh(1, 4097, 122)
    return out


def alone(n=4097):
    """every vertex alone in its cell: the lattice points (i, j, k) + 1/2 of a 17^3 block, shuffled"""
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(*[np.arange(17) - 8] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
    g = g[rng.permutation(len(g))]
    tris = rng.integers(0, n, (2 * n, 3))
    return mesh((g + 0.5) * 0.25, tris, 0.25)


def one_cell(n, x0=0.3, seed=6):
    """n vertices in ONE cell of 0.05 m at x0, two more elsewhere, and triangles between them: one slot and one row of sums take everything."""
    rng = np.random.default_rng(seed)
    cell = F(0.05)
    base = np.floor(np.float64(F(x0)) / np.float64(cell)) * np.float64(cell)
    v = np.zeros((n + 2, 3), F)
    v[:n, 0] = (base + rng.uniform(0.1, 0.9, n) * np.float64(cell)).astype(F)
    v[:n, 1:] = rng.uniform(0.001, 0.049, (n, 2)).astype(F)
    v[n] = (1.0, 1.0, 1.0)
    v[n + 1] = (-1.0, 1.0, 1.0)
    tris = np.concatenate([rng.integers(0, n, (64, 3)), [[n - 1, n, n + 1], [n + 1, n, 5], [3, n, n + 1]]])
    nrm = np.tile(np.array([[0.6, 0.0, 0.8]], F), (n + 2, 1))
    col = np.tile(np.array([[255, 0, 1, 255]], np.uint8), (n + 2, 1))
    col[::2, 2] = 0                                                         # blue: half ones, half zeros -- a tie at one half where n is even
    return mesh(v, tris, cell, nrm, col)


def cell_arithmetic():
    """cell = 1/4: exact multiples either side of 0, -0.0, and the largest float below each boundary"""
    k = np.arange(-6, 7)
    x = np.concatenate([(k * 0.25).astype(F), np.nextafter((k * 0.25).astype(F), F(-np.inf)), np.array([-0.0, 0.0], F)])
    v = np.stack([x, np.roll(x, 5), np.roll(x, 11)], 1)
    rng = np.random.default_rng(7)
    return mesh(v, rng.integers(0, len(v), (200, 3)), 0.25)


def quotients(cell):
    """coordinates float32(k) * cell: their float64 quotient by cell lands on, just below and just above integers"""
    k = np.arange(1, 2001)
    x = (k.astype(F) * F(cell)).astype(F)
    v = np.stack([x, -x, np.roll(x, 1)], 1)
    rng = np.random.default_rng(8)
    return mesh(v, rng.integers(0, len(v), (3000, 3)), cell)


def lattice_ends():
    """cell = 2^-9: c = -2^20 and c = 2^20 - 1 are the last cells"""
    c = 2.0 ** -9
    v = np.array([[-2048.0, 0.0, 0.0], [2048.0 - c, 0.0, 0.0], [0.0, -2048.0, 2048.0 - c], [0.0, 0.0, 0.0], [-2048.0, 2048.0 - c, -2048.0]], F)
    return mesh(v, [[0, 1, 2], [2, 3, 4], [4, 0, 1]], c)


def below_4096():
    big = np.nextafter(F(4096.0), F(0.0))
    v = np.array([[big, 0.0, 0.0], [0.0, -big, 0.0], [0.0, 0.0, big], [1.0, 1.0, 1.0]], F)
    return mesh(v, [[0, 1, 2], [1, 2, 3]], 1.0)


def ties():
    """coordinates (2 k + 1) 2^-21 for even and odd k, every vertex alone in a cell of 2^-4; and clusters of 3 and of 7 whose mean is not representable"""
    k = np.arange(-40, 40)
    x = ((2 * k + 1) * 2.0 ** -21 + k * 2.0 ** -4).astype(np.float64)
    assert (x.astype(F).astype(np.float64) == x).all()
    a = np.stack([x, x[::-1], x], 1).astype(F)
    rng = np.random.default_rng(9)
    three = (np.array([[5.0, 5.0, 5.0]]) + rng.integers(1, 2 ** 16, (3, 3)) * 2.0 ** -20).astype(F)
    seven = (np.array([[6.0, 6.0, 6.0]]) + rng.integers(1, 2 ** 16, (7, 3)) * 2.0 ** -20).astype(F)
    v = np.concatenate([a, three, seven])
    n = len(a)
    tris = np.concatenate([rng.integers(0, n, (100, 3)), [[0, n, n + 3], [n + 1, n + 4, 7], [n + 9, 3, n + 2]]])
    return mesh(v, tris, 2.0 ** -4)


def hash_lines():
    """4096 occupied cells in arithmetic progressions along each axis with strides 1, 2^4 and 2^8: keys that differ in one axis only, along x
    only above bit 42"""
    c = 2.0 ** -9
    i = np.arange(4096)
    parts = []
    for axis in range(3):
        for q, stride in enumerate((1, 16, 256)):
            g = np.zeros((4096, 3))
            g[:, axis] = i * stride
            g[:, (axis + 1) % 3] = -(3 + 2 * q)                             # (each line on a row of its own)
            g[:, (axis + 2) % 3] = -(100 + axis)
            parts.append((g + 0.5) * c)
    v = np.concatenate(parts)
    rng = np.random.default_rng(10)
    return mesh(v, rng.integers(0, len(v), (20000, 3)), c)


def reversed_order(n=300):
    """vertex i and vertex i + n share cell n - i: the order of the leads is the reverse of the order of the keys"""
    x = (n - np.arange(n) + 0.5) * 0.125
    v = np.zeros((2 * n, 3))
    v[:n, 0] = x
    v[n:, 0] = x + 0.03
    t = np.arange(n - 2)
    return mesh(v, np.stack([t + n, t + 1, t + 2], 1), 0.125)


def low_triangle_high_vertices():
    v = np.zeros((12, 3))
    v[:, 0] = np.arange(12) * 0.5 + 0.1
    return mesh(v, [[9, 10, 11], [11, 10, 9], [0, 1, 2], [5, 3, 4]], 0.5)


def normals_and_colours():
    """cells of 1 m along x.  cell 0: NaN and infinite members next to finite ones; cell 1: all NaN; cell 2: two opposite normals; cell 3: one
    normal of 4096; cell 4: colours with a == 0 members; cell 5: nobody coloured; cell 6: channel sums that tie at one half"""
    nan, inf = np.nan, np.inf
    rows = [
        (0.1, (0.0, 0.0, 1.0), (10, 20, 30, 255)), (0.2, (nan, 0.0, 1.0), (11, 21, 31, 255)), (0.3, (0.0, inf, 0.0), (12, 22, 33, 1)),
        (0.4, (1.0, 0.0, 0.0), (0, 0, 0, 0)), (0.5, (0.0, -inf, nan), (250, 251, 252, 0)),
        (1.1, (nan, nan, nan), (1, 2, 3, 255)), (1.2, (nan, 1.0, 0.0), (2, 3, 4, 255)),
        (2.1, (0.36, 0.48, 0.8), (255, 255, 255, 255)), (2.2, (-0.36, -0.48, -0.8), (0, 0, 0, 255)),
        (3.1, (4096.0, 0.0, 0.0), (9, 9, 9, 255)), (3.2, (0.0, 4095.0, 0.0), (9, 9, 9, 255)),
        (4.1, (0.0, 1.0, 0.0), (100, 100, 100, 0)), (4.2, (0.0, 1.0, 0.0), (7, 8, 9, 255)), (4.3, (0.0, 1.0, 0.0), (200, 0, 0, 0)),
        (5.1, (1.0, 0.0, 0.0), (5, 5, 5, 0)), (5.2, (1.0, 0.0, 0.0), (6, 6, 6, 0)),
        (6.1, (0.0, 0.0, -1.0), (0, 1, 2, 255)), (6.2, (0.0, 0.0, -1.0), (1, 2, 3, 255)),
    ]
    v = np.array([[x, 0.5, 0.5] for x, _, _ in rows])
    tris = [[0, 5, 7], [7, 9, 11], [11, 14, 16], [16, 0, 9], [5, 11, 16]]
    return mesh(v, tris, 1.0, [n for _, n, _ in rows], [c for _, _, c in rows])


def triangle_zoo():
    """cells of 1 m along x; vertices 2 i and 2 i + 1 lie in cell i (i < 10), vertex 20 in cell 0.  Leads 0, 2, .., 18."""
    v = np.zeros((21, 3))
    v[:20, 0] = np.arange(20) // 2 + 0.25 + 0.5 * (np.arange(20) % 2)
    v[20, 0] = 0.6
    tris = [
        [0, 0, 2],        # 0  a a b in the input
        [4, 4, 4],        # 1  a a a in the input
        [0, 1, 4],        # 2  degenerate after mapping, two equal
        [0, 1, 20],       # 3  degenerate after mapping, three equal
        [5, 6, 2],        # 4  clusters (4, 6, 2): kept, with its own rotation -- the smallest is LAST
        [2, 4, 6],        # 5  a rotation of 4: dropped
        [7, 3, 5],        # 6  clusters (6, 2, 4), a rotation of 4: dropped
        [2, 6, 4],        # 7  the opposite winding: kept
        [6, 4, 2],        # 8  a rotation of 7: dropped
        [16, 18, 0],      # 9  kept
        [12, 14, 13],     # 10 clusters (12, 14, 12): degenerate; clusters 12 and 14 become orphans, clusters 8 and 10 nobody names
        [3, 5, 7],        # 11 clusters (2, 4, 6) once more: dropped
    ]
    return mesh(v, tris, 1.0)


def duplicates_at_the_ends(nt=65537):
    """vertices alone in their cells, nt distinct triangles but the last, which is a rotation of the first"""
    n = 1024
    v = np.zeros((n, 3))
    v[:, 0] = np.arange(n) + 0.5
    t = np.arange(nt)
    tris = np.stack([t % n, (t // n * 7 + t + 1) % n, (t // n * 13 + t + 500) % n], 1)
    tris[nt - 1] = tris[0][[1, 2, 0]]
    return mesh(v, tris, 1.0)


def copies(n=65536):
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5]])
    tris = np.tile(np.array([[2, 0, 1]]), (n, 1))
    tris[1::3] = [0, 1, 2]
    tris[2::3] = [1, 2, 0]
    return mesh(v, tris, 1.0)


def crafted():
    out = {
        "every vertex alone": alone(),
        "65537 vertices in one cell": one_cell(65537),
        "cell arithmetic": cell_arithmetic(),
        "quotients 0.1": quotients(F(0.1)),
        "quotients 0.3": quotients(F(0.3)),
        "quotients 0.7": quotients(F(0.7)),
        "lattice ends": lattice_ends(),
        "below 4096": below_4096(),
        "ties": ties(),
        "hash lines": hash_lines(),
        "reversed order": reversed_order(),
        "low triangle, high vertices": low_triangle_high_vertices(),
        "normals and colours": normals_and_colours(),
        "triangle zoo": triangle_zoo(),
        "duplicates at the ends": duplicates_at_the_ends(),
        "65536 copies": copies(),
    }
    return out


def far_cell():
    """2^21 + 1 vertices in the last cell of 2^-8 m below x = 4096 m, c_x = 2^20 - 1, at x = 4096 - k 2^-12 for k = 1 .. 7 (seven of the cell's
    sixteen floats): S_x > 2^53"""
    n = 2 ** 21 + 1
    rng = np.random.default_rng(12)
    v = np.zeros((n + 2, 3), F)
    v[:n, 0] = (4096.0 - rng.integers(1, 8, n) * 2.0 ** -12).astype(F)
    v[:n, 1:] = rng.uniform(0.0005, 0.0035, (n, 2)).astype(F)
    v[n] = (1.0, 1.0, 1.0)
    v[n + 1] = (-1.0, 1.0, 1.0)
    tris = np.concatenate([rng.integers(0, n, (64, 3)), [[n - 1, n, n + 1], [n + 1, n, 5], [3, n, n + 1]]])
    nrm = np.tile(np.array([[0.6, 0.0, 0.8]], F), (n + 2, 1))
    col = np.tile(np.array([[255, 0, 1, 255]], np.uint8), (n + 2, 1))
    col[::2, 2] = 0
    return mesh(v, tris, 2.0 ** -8, nrm, col)
