"""Seeded clouds that put the voxel-grid, normal and FPFH kernels of csrc/er_fpfh.hip at their shape edges (tests/test_fpfh_cases_cpu.py,
tests/test_fpfh_shapes_gpu.py).  numpy only; the expected values come from tests/fpfh_restatement.py, unchanged.

A Case is one cloud with the two radii it is searched at.  The voxel stage runs on the cloud at LEAF; the normals stage runs on the cloud
ITSELF (so that the point count the wave-per-point kernels see is the count the family names), except in the "-down" variants of `sizes`,
whose cloud is the restatement's voxel-grid output of the case before it; the SPFH / FPFH stage gets the restatement's float32 normals of
the normals stage (feat_normals == "estimated") or, in `star`, the fixture's own random unit normals (feat_normals == "input": the star's
estimated normals are NaN or degenerate by its symmetry).

  sizes   the patch with n at and around the workgroup edges (4 points per workgroup of k_fp_*, 256 per workgroup of k_vox_*), at three
          translations; for n <= 65 most points have fewer than 3 neighbours (the NaN mask, the zero rows)
  clumps  k mutual neighbours: one row range of the candidate walk holds exactly k candidates, ceil(k / 64) trips
  star    one neighbour in each of the 26 cells around the centre's at r (1 - 2^-18), or just outside at r (1 + 2^-18)
  exact   d2 == fl32(r * r) exactly: not a neighbour
  coarse  a radius grid beyond 2^25 cells: the builder doubles the cell
  voxels  cell faces, negative coordinates, one cell, n cells, a segment across the workgroup boundary of k_vox_heads / k_vox_starts
"""
import numpy as np

import fpfh_restatement as fr

LEAF, R_NORMAL, R_FEATURE, CELL = 0.05, 0.1, 0.25, 0.075
F32 = np.float32
GRID_LIMIT = 1 << 25                      # cloud_create_impl doubles the cell until the padded grid has at most this many cells
_cache = {}


class Case:
    def __init__(self, name, xyz, nrm, r_normal=R_NORMAL, r_feature=R_FEATURE, feat_normals="estimated", voxel=True, **facts):
        self.name = name
        self.xyz = np.ascontiguousarray(xyz, F32)
        self.nrm = np.ascontiguousarray(nrm, F32)
        assert self.xyz.shape == self.nrm.shape and self.xyz.shape[1] == 3
        self.r_normal, self.r_feature, self.feat_normals, self.voxel, self.facts = r_normal, r_feature, feat_normals, voxel, facts

    def __repr__(self):
        return "Case(%s, %d points)" % (self.name, len(self.xyz))


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def random_units(g, n):
    return unit(g.normal(size=(n, 3))).astype(F32)


def patch(n, seed):
    """n points with (u, v) uniform in the unit square, z = 0.1 sin(5u) cos(3v), and the normalised (-0.5 cos 5u, 0.3 sin 3v, 1)."""
    g = np.random.default_rng(seed)
    u, v = g.random(n), g.random(n)
    x = np.stack([u, v, 0.1 * np.sin(5 * u) * np.cos(3 * v)], axis=1).astype(F32)
    nrm = unit(np.stack([-0.5 * np.cos(5 * u), 0.3 * np.sin(3 * v), np.ones(n)], axis=1)).astype(F32)
    return x, nrm


def grid_of(xyz, radius):
    """(org float32 [3], cell float32, dim [3], doublings) as cloud_create_impl lays the radius grid out: cell = fl32(radius) * 1.001f, doubled
    while the grid padded by four cells per axis exceeds GRID_LIMIT; dim = floor((hi - lo) / cell) + 1 in float32."""
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    cell = F32(F32(radius) * F32(1.001))
    doublings = 0
    while True:
        dim = np.floor((hi - lo) / cell).astype(np.int64) + 1
        if int(np.prod(dim + 4)) <= GRID_LIMIT:
            return lo, cell, dim, doublings
        cell = F32(cell * F32(2.0))
        doublings += 1


def cells_of(xyz, org, cell, dim):
    """floor((p - org) / cell) in float32, clamped to the grid: the cell k_chunk_cells and fp_for_candidates give a point."""
    q = np.floor((xyz.astype(F32) - org) / cell).astype(np.int64)
    return np.clip(q, 0, dim - 1)


# ---- sizes -------------------------------------------------------------------------------------------------------------------------
SIZES_N = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025)
SIZES_T = (0.0, -3.0, 40.0)


def sizes():
    out = []
    for n in SIZES_N:
        x, nrm = patch(n, [1, n])
        for t in SIZES_T:
            xt = (x + F32(t)).astype(F32)
            raw = Case("sizes-n%d-t%g" % (n, t), xt, nrm, n=n, t=t)
            out.append(raw)
            dx, dn, _ = fr.voxel_grid(xt, nrm, LEAF)
            out.append(Case(raw.name + "-down", dx, dn, voxel=False, n=n, t=t))
    return out


# ---- clumps ------------------------------------------------------------------------------------------------------------------------
CLUMPS_K = (3, 63, 64, 65, 127, 128, 129, 193, 257)


def clumps():
    out = []
    for k in CLUMPS_K:
        g = np.random.default_rng([2, k])
        u, v = 0.05 * g.random(k), 0.05 * g.random(k)
        x = (np.stack([u, v, 0.01 * np.sin(60 * u) * np.cos(40 * v)], axis=1) + np.array([3.0, -1.0, 2.0])).astype(F32)
        # 0.05 x 0.05 x 0.02: the diagonal is 0.073 < both radii, so every point is every other's neighbour
        assert np.linalg.norm(x.astype(np.float64).max(axis=0) - x.astype(np.float64).min(axis=0)) < 0.08
        out.append(Case("clumps-k%d" % k, x, random_units(g, k), k=k))
    return out


# ---- star --------------------------------------------------------------------------------------------------------------------------
STAR_R = (0.25, 0.125, 0.1)
STAR_NORMAL_SHARE = 0.75        # the normals stage of `star` runs at 0.75 r (see star())


def star():
    """28 points: the centre c, 26 points at c + d r (1 -+ 2^-18) for the normalised d in {-1, 0, 1}^3, and an anchor at c - 1.5 cell that is
    the grid's origin, so that c is in the middle of cell (1, 1, 1).  Point 0 is the centre, 1 .. 26 the directions, 27 the anchor.
    The centre's neighbourhood at r has cubic symmetry: its scatter matrix is a multiple of the identity and its normal is not defined.
    The normals stage therefore runs at 0.75 r, where the centre and the six axis points are alone (NaN), an edge point sees its two
    corners and a corner its three edges (nearest spacings: corner-edge 0.60 r, axis-edge 0.77 r); the neighbour COUNT of the normals
    kernel at r itself is pinned separately by the GPU test."""
    out = []
    dirs = unit(np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)], np.float64))
    c = np.array([1.0, -2.0, 0.5])
    for r in STAR_R:
        r32 = F32(r)
        cell = F32(r32 * F32(1.001))
        for twin, scale in (("inner", 1.0 - 2.0 ** -18), ("outer", 1.0 + 2.0 ** -18)):
            g = np.random.default_rng([3, int(r * 1000)])
            x = np.concatenate([c[None, :], c + dirs * float(r32) * scale, (c - 1.5 * float(cell))[None, :]]).astype(F32)
            org, gcell, dim, doublings = grid_of(x, r)
            assert doublings == 0 and gcell == cell and np.array_equal(org, x[27])
            q = np.floor((x[:27] - org) / cell).astype(np.int64)          # the builder's expression, in float32
            assert list(q[0]) == [1, 1, 1] and len({tuple(t) for t in q}) == 27 and q.min() == 0 and q.max() == 2
            count = int((fr.sqdist32(x[:1], x) < r32 * r32).sum())
            assert count == (27 if twin == "inner" else 1), (r, twin, count)
            out.append(Case("star-r%g-%s" % (r, twin), x, random_units(g, 28), r_normal=STAR_NORMAL_SHARE * r, r_feature=r, feat_normals="input",
                            r=r, centre_nn=count))
    return out


# ---- exact -------------------------------------------------------------------------------------------------------------------------
def exact():
    """r = 0.25: fl32(r) * fl32(r) = 0.0625 exactly.  Point 0 = (0, 0, 0), point 1 = (0.25, 0, 0) at d2 == r2 (NOT a neighbour of 0), point 2 =
    (0, nextafter(0.25, 0), 0) at d2 = 0.0625 - 2^-27 (a neighbour of 0).  Twelve patch points in x, y in [-0.07, -0.02]: all neighbours of
    point 0 and of one another (d < 0.11), none of points 1 and 2 (d > 0.27).  So nn = 14, 1, 2 for the named points and 13 for the rest."""
    r = F32(0.25)
    assert float(r) * float(r) == float(r * r) == 0.0625
    below = np.nextafter(r, F32(0))
    m = 12
    g = np.random.default_rng([4, 0])
    u, v = 0.02 + 0.05 * g.random(m), 0.02 + 0.05 * g.random(m)
    p = np.stack([-u, -v, 0.1 * np.sin(5 * u) * np.cos(3 * v)], axis=1)
    pn = unit(np.stack([-0.5 * np.cos(5 * u), 0.3 * np.sin(3 * v), np.ones(m)], axis=1))
    x = np.concatenate([np.array([[0, 0, 0], [r, 0, 0], [0, below, 0]], np.float64), p]).astype(F32)
    nrm = np.concatenate([np.tile([0.0, 0.0, 1.0], (3, 1)), pn]).astype(F32)
    d2 = fr.sqdist32(x[:1], x)
    assert d2[1] == r * r and d2[2] < r * r and float(d2[2]) == 0.0625 - 2.0 ** -27
    nn = [14, 1, 2] + [13] * m
    assert [int((fr.sqdist32(x[i:i + 1], x) < r * r).sum()) for i in range(len(x))] == nn
    return [Case("exact", x, nrm, r_normal=0.25, r_feature=0.25, nn=nn)]


# ---- coarse ------------------------------------------------------------------------------------------------------------------------
def coarse():
    """The 8 corners of a 3.6 m cube, two clumps of 70 points within balls of diameter 0.004 (one beside a corner, which it counts among its
    neighbours), and two points 0.015 apart inside one doubled cell.  Both radii 0.01: at cell 0.01001 the padded grid is 364^3 > 2^25 cells,
    so the builder doubles the cell to 0.02002 (184^3).  Points 0 .. 7 are the corners, 8 .. 77 the corner clump, 78 .. 147 the second clump, 148 and
    149 the close pair."""
    r = 0.01
    g = np.random.default_rng([5, 0])
    lo, side = -1.8, 3.6
    corners = lo + side * np.array([(a, b, c) for c in (0, 1) for b in (0, 1) for a in (0, 1)], np.float64)

    def ball(centre):
        d = g.normal(size=(70, 3))
        d = d / np.linalg.norm(d, axis=1, keepdims=True) * (0.002 * g.random((70, 1)) ** (1.0 / 3.0))
        return centre + d
    clump_a = ball(corners[0] + 0.003)                               # inside the cube, 0.0052 from the corner: the corner is within r of all of it
    clump_b = ball(np.array([0.7, -0.3, 1.1]))
    cell2 = 2.0 * float(F32(F32(r) * F32(1.001)))
    a = np.array([lo + 100.1 * cell2, lo + 50.5 * cell2, lo + 70.5 * cell2])
    pair = np.stack([a, a + np.array([0.015, 0.0, 0.0])])
    x = np.concatenate([corners, clump_a, clump_b, pair]).astype(F32)
    org, cell, dim, doublings = grid_of(x, r)
    first = np.floor((x.max(axis=0) - x.min(axis=0)) / F32(F32(r) * F32(1.001))).astype(np.int64) + 1
    assert list(first) == [360] * 3 and (360 + 4) ** 3 > GRID_LIMIT                    # the cell of the radius: refused
    assert doublings == 1 and cell == F32(cell2) and list(dim) == [180] * 3 and (180 + 4) ** 3 <= GRID_LIMIT
    q = cells_of(x, org, cell, dim)
    assert np.array_equal(q[148], q[149])                                              # the pair shares a doubled cell ...
    r2 = F32(r) * F32(r)
    assert fr.sqdist32(x[148:149], x[149:150])[0] > r2                                  # ... and is no neighbour pair
    assert (fr.sqdist32(x[0:1], x[8:78]) < r2).all()                                    # the corner and its clump
    for s in (slice(8, 78), slice(78, 148)):
        y = x[s].astype(np.float64)
        assert np.linalg.norm(y[:, None, :] - y[None, :, :], axis=2).max() <= 0.004 + 1e-6      # within a ball of diameter 0.004
    nn = [71] + [1] * 7 + [71] * 70 + [70] * 70 + [1, 1]
    return [Case("coarse", x, random_units(g, len(x)), r_normal=r, r_feature=r, nn=nn)]


# ---- voxels ------------------------------------------------------------------------------------------------------------------------
def _faces(ks, other):
    """For every axis and every k: the points whose coordinate on that axis is fl32(k * LEAF) and its two float32 neighbours, the other two
    coordinates = `other` (the middle of a cell)."""
    pts = []
    for axis in range(3):
        for k in ks:
            f = F32(k * LEAF)
            for v in (np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))):
                p = [other] * 3
                p[axis] = v
                pts.append(p)
    return np.array(pts, F32)


def _cell_centres(ijk):
    return ((np.asarray(ijk, np.float64) + 0.5) * LEAF).astype(F32)


def _jitter(g, n):
    return ((g.random((n, 3)) - 0.5) * 0.6 * LEAF).astype(F32)          # stays inside the cell around a centre


def voxels():
    out = []
    g = np.random.default_rng([6, 0])

    def add(name, x, **facts):
        p = g.permutation(len(x))                                    # file order is not cell order: the sort has work to do
        x = np.ascontiguousarray(x[p], F32)
        out.append(Case("voxels-" + name, x, random_units(g, len(x)), **facts))
    a = _faces(range(-3, 4), 0.02)
    add("a-faces", a)
    one = _cell_centres([[2, -1, 3]] * 300) + _jitter(g, 300)
    add("b-one-cell", one, m=1)
    lattice = np.array([(i, j, k) for k in range(7) for j in range(7) for i in range(7)])
    own = _cell_centres(lattice[g.permutation(343)[:257]] - 3) + _jitter(g, 257)
    add("c-own-cells", own, m=257)
    for name, nx in (("d-segment-200", 20), ("d-segment-256", 16)):
        ny = {20: 10, 16: 16}[nx]
        singles = _cell_centres([(i, j, 0) for j in range(ny) for i in range(nx)]) + _jitter(g, nx * ny)
        big = _cell_centres([[0, 0, 1]] * 300) + _jitter(g, 300)     # the highest key: its sorted segment starts behind every single cell
        add(name, np.concatenate([singles, big]), m=nx * ny + 1, segment=(nx * ny, nx * ny + 300))
    col = np.concatenate([(0.005 + 0.04 * g.random((300, 2))), 2.0 * g.random((300, 1))], axis=1)
    col[0, 2], col[1, 2] = 0.001, 1.999                              # the first and the last cell are occupied
    add("e-column", col, div=(1, 1, 40))
    add("f-negative", -_faces(range(1, 8), 0.02))
    for c in out:
        key, _, _, div = fr.voxel_cells(c.xyz, LEAF)
        uk = np.unique(key)
        if "m" in c.facts:
            assert len(uk) == c.facts["m"], (c.name, len(uk))
        if "div" in c.facts:
            assert tuple(div) == c.facts["div"]
        if "segment" in c.facts:
            s0, s1 = c.facts["segment"]
            sk = np.sort(key)
            assert (sk[s0:s1] == sk[s0]).all() and sk[s0 - 1] != sk[s0] and s1 == len(sk) and s0 <= 256 < s1
    assert (out[0].xyz.min() < 0 < out[0].xyz.max()) and out[-1].xyz.max() < 0
    return out


FAMILIES = {"sizes": sizes, "clumps": clumps, "star": star, "exact": exact, "coarse": coarse, "voxels": voxels}
FEATURE_FAMILIES = ("sizes", "clumps", "star", "exact", "coarse")


def cases(family):
    if family not in _cache:
        _cache[family] = FAMILIES[family]()
    return _cache[family]


def case(name):
    return next(c for c in cases(name.split("-")[0]) if c.name == name)


def voxel_key_of(pts, ref_xyz):
    """The voxel key of `pts` in the key space of the cloud ref_xyz."""
    _, _, min_b, div = fr.voxel_cells(ref_xyz, LEAF)
    rel = np.floor(np.asarray(pts, F32) * (F32(1.0) / F32(LEAF))).astype(np.int64) - min_b
    return rel[:, 0] + rel[:, 1] * div[0] + rel[:, 2] * div[0] * div[1]


def restated(c):
    """The restatement's values for a case, computed once and shared (read only): vox = (xyz, nrm, key); normals, n_counts, gap, absdot at
    r_normal; feat_nrm = the normals the feature stage is fed; counts, nn, edge, pairs, feat at r_feature."""
    key = ("restated", c.name)
    if key not in _cache:
        ne, ncnt, gap, absdot = fr.normals(c.xyz, c.nrm, c.r_normal)
        fn = ne if c.feat_normals == "estimated" else c.nrm
        counts, nn, edge, pairs = fr.spfh(c.xyz, fn, c.r_feature)
        d = dict(vox=fr.voxel_grid(c.xyz, c.nrm, LEAF) if c.voxel else None, normals=ne, n_counts=ncnt, gap=gap, absdot=absdot, feat_nrm=fn,
                 counts=counts, nn=nn, edge=edge, pairs=pairs, feat=fr.fpfh(fn, counts, nn, pairs))
        for v in d.values():
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _cache[key] = d
    return _cache[key]
