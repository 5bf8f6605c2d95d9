"""Crafted FragmentOptimizer inputs shared by tests/test_fopt_sums_cpu.py and tests/test_fopt_shapes_gpu.py (helper, no tests).

A fragment's points are drawn inside CHOSEN lattice cells, so a correspondence list between the points of one cell of fragment i and
one cell of fragment j is exactly one (pair, cell, cell) group of the assembly, of a chosen number of rows.  Normals have unit length
at load; every fragment gets a small pose so that p and n are general float32 numbers when the systems are assembled."""
import numpy as np

GROUP_SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 511, 512, 513, 1024, 1025)      # around the 4 rows of one MFMA, a wave's 64 lanes, kChunkMax = 512


class Case:
    def __init__(self, name, num, res, length, frags, pairs, seed):
        self.name, self.num, self.res, self.length, self.frags, self.pairs = name, num, res, float(length), frags, pairs
        self.poses = [small_pose(seed * 131 + f) for f in range(num)]
        self.Rt = np.stack([P[:3, :3].astype(np.float64).T.reshape(9) for P in self.poses])      # non-identity pose_rot_t

    def with_pairs(self, pairs, name=None):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.pairs, c.name = pairs, name or self.name
        return c

    def rows(self):
        return sum(len(p[2]) for p in self.pairs)


def small_pose(seed):
    """A rotation of about two degrees about a random axis and a centimetre of translation, float32 4 x 4."""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3)
    w *= np.radians(2.0) / np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    t = np.linalg.norm(w)
    P = np.eye(4)
    P[:3, :3] = np.eye(3) + np.sin(t) / t * K + (1 - np.cos(t)) / t ** 2 * K @ K
    P[:3, 3] = rng.normal(0, 0.01, 3)
    return P.astype(np.float32)


def unit_normals(rng, m):
    n = rng.normal(size=(m, 3))
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


def cell_points(rng, res, length, cell, m):
    """m points uniformly inside lattice cell `cell` = (cx, cy, cz), a twentieth of a cell away from its faces."""
    return ((np.asarray(cell, np.float64) + rng.uniform(0.05, 0.95, (m, 3))) * (length / res)).astype(np.float32)


def cube_points(rng, length, m):
    return rng.uniform(0.02 * length, 0.98 * length, (m, 3)).astype(np.float32)


def idx0_of(cell, res):
    """idx_[0] of a cell: its corner vertex index times three."""
    return (cell[0] + cell[1] * (res + 1) + cell[2] * (res + 1) ** 2) * 3


def group_size_case(res=4, length=3.0, seed=5):
    """Two fragments; list k pairs the GROUP_SIZES[k] points of cell a_k of fragment 0 with those of cell b_k of fragment 1: one group
    each.  Returns the case (all 13 lists) and the expected group table."""
    rng = np.random.default_rng(seed)
    x0, x1, pairs, table, o = [], [], [], [], 0
    for k, m in enumerate(GROUP_SIZES):
        a, b = (k % res, (k // res) % res, 1), ((k + 1) % res, (k // res) % res, 2 + k % 2)
        x0.append(cell_points(rng, res, length, a, m))
        x1.append(cell_points(rng, res, length, b, m))
        pairs.append((0, 1, np.stack([o + np.arange(m), o + rng.permutation(m)], 1).astype(np.int32)))
        table.append((0, 1, idx0_of(a, res), idx0_of(b, res)))
        o += m
    frags = [(np.concatenate(x), unit_normals(rng, o)) for x in (x0, x1)]
    return Case("group sizes", 2, res, length, frags, pairs, seed), np.array(table, np.int32)


RELATIONS = {                 # offset of cell c_j from cell c_i
    "same": (0, 0, 0), "face": (1, 0, 0), "edge": (1, 1, 0), "vertex": (1, 1, 1), "disjoint": (3, -3, 3),
}


def relation_cases(res, relation, length=3.0):
    """c_i and c_j in the given relation, in both index orders, each with a one-row list (every entry has one addend per coinciding
    index pattern: the bit-exact case) and a 37-row list.  Resolution 2 has no disjoint cells: every cell touches vertex (1, 1, 1)."""
    d = RELATIONS[relation]
    base = (0, 0, 0) if res == 2 else (3, 4, 2)
    other = tuple(b + x for b, x in zip(base, d))
    assert all(0 <= c < res for c in other), "no such pair of cells at resolution %d" % res
    out = []
    for ci, cj in ((base, other), (other, base)) if relation != "same" else ((base, other),):
        for m in (1, 37):
            rng = np.random.default_rng(1000 * res + 10 * sorted(RELATIONS).index(relation) + m + (ci > cj))
            frags = [(cell_points(rng, res, length, c, m), unit_normals(rng, m)) for c in (ci, cj)]
            pairs = [(0, 1, np.stack([np.arange(m), rng.permutation(m)], 1).astype(np.int32))]
            out.append(Case("res %d %s %s %d rows" % (res, relation, "ci<cj" if idx0_of(ci, res) <= idx0_of(cj, res) else "ci>cj", m), 2, res, length, frags, pairs, 7 + m))
    return out


def exact_weight_cases(res=4, length=3.0):
    """Points ON a cell face, edge or vertex: coordinates that are exact multiples of length / res (0.75, exact in float32), so the
    fractional part r is exactly 0 and trilinear weights are exactly 0 or 1."""
    ul = length / res
    out = []

    def place(rng, cell, kind, m):
        x = cell_points(rng, res, length, cell, m)
        for axis in range({"face": 1, "edge": 2, "vertex": 3}[kind]):
            x[:, axis] = np.float32(cell[axis] * ul)
        return x

    for kind, other in (("face", "edge"), ("edge", "vertex"), ("vertex", "face")):
        rng = np.random.default_rng(77 + "fev".index(kind[0]))
        frags = [(place(rng, (1, 2, 1), kind, 1), unit_normals(rng, 1)), (place(rng, (2, 2, 1), other, 1), unit_normals(rng, 1))]
        out.append(Case("weights %s / %s, one row" % (kind, other), 2, res, length, frags, [(0, 1, np.zeros((1, 2), np.int32))], 3))
    rng = np.random.default_rng(78)
    xs = [np.concatenate([place(rng, c, "face", 8), place(rng, c, "edge", 8), place(rng, c, "vertex", 4), cell_points(rng, res, length, c, 10)])
          for c in ((1, 2, 1), (1, 1, 1))]
    frags = [(x, unit_normals(rng, 30)) for x in xs]
    out.append(Case("weights mixed, 30 rows", 2, res, length, frags, [(0, 1, np.stack([np.arange(30), rng.permutation(30)], 1).astype(np.int32))], 4))
    return out


def cube_case(name, num, res, length, n_points, lists, rows, seed):
    """`num` fragments of n_points points anywhere in the cube; `lists` = [(i, j)] with `rows` random rows each."""
    rng = np.random.default_rng(seed)
    frags = [(cube_points(rng, length, n_points), unit_normals(rng, n_points)) for _ in range(num)]
    pairs = [(i, j, rng.integers(0, n_points, (rows, 2)).astype(np.int32)) for i, j in lists]
    return Case(name, num, res, length, frags, pairs, seed)


def lattice_cases():
    return [cube_case("lattice res %d length %.1f" % (res, length), 3, res, length, 120, [(0, 1), (1, 2), (0, 2)], 100, 20 + res)
            for res, length in ((1, 3.0), (2, 3.0), (3, 3.0), (8, 3.0), (3, 2.5))]


def list_cases():
    """num = 2; and num = 5 with a (j, i) list with j > i, a fragment pair listed twice, an empty list between two non-empty ones, a row
    repeated inside a list and a fragment that holds a single point."""
    two = cube_case("two fragments", 2, 3, 3.0, 90, [(0, 1)], 150, 31)
    five = cube_case("five fragments", 5, 3, 3.0, 90, [(0, 1), (3, 1), (0, 1), (1, 2), (2, 3)], 60, 32)
    rng = np.random.default_rng(33)
    five.frags[4] = (five.frags[4][0][:1], five.frags[4][1][:1])                                  # a single point
    p = list(five.pairs)
    p[3] = (1, 2, np.zeros((0, 2), np.int32))                                                     # empty, between two non-empty lists
    rep = p[4][2].copy()
    rep[10:14] = rep[9]                                                                           # one row five times
    p[4] = (2, 3, rep)
    p.append((2, 4, np.stack([rng.integers(0, 90, 25), np.zeros(25, np.int64)], 1).astype(np.int32)))
    five.pairs = p
    return [two, five]


def solve_case(mode, num, res, seed=50):
    """Fragments of 200 points anywhere in the cube, a chain of lists (i, i + 1) plus (0, num - 1), 120 rows each."""
    lists = [(i, i + 1) for i in range(num - 1)] + ([(0, num - 1)] if num > 2 else [])
    return cube_case("%s num %d res %d" % (mode, num, res), num, res, 3.0, 200, lists, 120, seed + 10 * num + res)


# (mode, num, res, unknowns): the sizes at which potrf_rec's arithmetic n1 = ceil(n / 2 / 64) * 64 meets its edges
SOLVE_SIZES = (
    ("slac", 2, 1, 36),          # one diagonal block with jb < 64
    ("slac", 2, 2, 93),          # 64 + 29
    ("slac", 8, 2, 129),         # 64 + 65 -> 64 + (64 + a 1 x 1 trailing block)
    ("slac", 2, 3, 204),         # 128 + 76 -> (64 + 64) + (64 + 12)
    ("nonrigid", 3, 1, 72),      # 64 + 8; block-sparse: three 24 x 24 fragment blocks
    ("nonrigid", 3, 2, 243),     # 128 + 115 -> (64 + 64) + (64 + 51); block-sparse: three 81 x 81 blocks (64 + 17)
)
