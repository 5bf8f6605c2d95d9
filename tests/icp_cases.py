"""Inputs that tests/test_icp_restatement_cpu.py and tests/test_icp_shapes_gpu.py share: a corner of three bumpy walls as the target, its
first n points moved by half a degree and 3 mm as sources at the sizes where k_icp_iter / k_icp_final take another path, the guesses, and
the clouds that sit on the data edges (a correspondence at exactly max_dist, non-finite normals, an exact copy, coplanar points, two
correspondences).  tests/test_icp_restatement_cpu.py checks on the restatement that every fixture is where it claims to be."""
import math

import numpy as np

F = np.float32
CELL = 0.03125
MAX_DIST = 0.03125                      # max_dist^2 = 2^-10 exactly, in float32 and in float64
SIZES = (1, 2, 3, 5, 6, 63, 64, 65, 255, 256, 257, 511, 512, 513, 769, 2048, 2049, 4097)
PER_WALL = 1400
SEED = 18
_cache = {}


def rigid(deg, axis, t):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    M[:3, 3] = t
    return M


MOVE = rigid(0.5, (0.3, -0.5, 0.8), (0.0018, -0.0016, 0.0017))          # about 0.5 degrees and 3 mm
GUESSES = {"identity": np.eye(4, dtype=F), "guess": rigid(0.2, (-0.6, 0.2, 0.5), (-0.0008, 0.0007, -0.0006)).astype(F)}


def target(seed=SEED, per_wall=PER_WALL):
    """(xyz, normals) float32: three walls meeting in a corner, a sine relief on each, points in shuffled order."""
    key = ("target", seed, per_wall)
    if key not in _cache:
        g = np.random.default_rng(seed)
        xyz, nrm = [], []
        for wall in range(3):
            u, v = g.uniform(0.06, 0.70, per_wall), g.uniform(0.06, 0.70, per_wall)
            fu, fv, amp = 9.0 + 2 * wall, 7.0 + 3 * wall, 0.012
            h = amp * np.sin(fu * u) * np.cos(fv * v)
            hu, hv = amp * fu * np.cos(fu * u) * np.cos(fv * v), -amp * fv * np.sin(fu * u) * np.sin(fv * v)
            p, n = np.stack([u, v, h], 1), np.stack([-hu, -hv, np.ones_like(u)], 1)
            n /= np.linalg.norm(n, axis=1, keepdims=True)
            xyz.append(np.roll(p, wall, axis=1))
            nrm.append(np.roll(n, wall, axis=1))
        order = g.permutation(3 * per_wall)
        x, n = np.concatenate(xyz)[order].astype(F), np.concatenate(nrm)[order].astype(F)
        x.setflags(write=False)
        n.setflags(write=False)
        _cache[key] = (x, n)
    return _cache[key]


def source(n):
    """The first n target points, moved."""
    x, _ = target()
    return (x[:n].astype(np.float64) @ MOVE[:3, :3].T + MOVE[:3, 3]).astype(F)


def with_edge_point(offset):
    """Target and source for the max_dist edge: the target gains the point (0, 0.5, -0.25), below the floor and away from everything else; the
    source is 64 exact copies of target points plus the point (offset, 0.5, -0.25), so the float32 difference along x is `offset` exactly."""
    x, n = target()
    tx = np.concatenate([x, np.array([[0.0, 0.5, -0.25]], F)])
    tn = np.concatenate([n, np.array([[0, 0, 1]], F)])
    sx = np.concatenate([x[:64], np.array([[F(offset), 0.5, -0.25]], F)]).astype(F)
    return tx, tn, sx


EDGE_EXACT = F(0.03125)                                  # squared: 2^-10 = max_dist^2
EDGE_ABOVE = np.nextafter(F(0.03125), F(1))              # squared: the second float32 above 2^-10


def flat_corner(per_wall=150):
    """Three flat walls with the exact unit normals of the axes.  With a source equal to a target subset the float32 residual
    n . d - n . s is exactly zero (one product is the coordinate itself, the others are zero), which a relief's slanted normals do not give."""
    g = np.random.default_rng(7)
    xyz, nrm = [], []
    for wall in range(3):
        p = np.stack([g.uniform(0.06, 0.7, per_wall), g.uniform(0.06, 0.7, per_wall), np.zeros(per_wall)], 1)
        xyz.append(np.roll(p, wall, axis=1))
        nrm.append(np.roll(np.tile([0.0, 0.0, 1.0], (per_wall, 1)), wall, axis=1))
    order = g.permutation(3 * per_wall)
    return np.concatenate(xyz)[order].astype(F), np.concatenate(nrm)[order].astype(F)


# iterations at which the loop stops on `source(n)` for n >= 6, both guesses: (stop_rule, eps) -> iterations; all converged
KNOWN_STOP = {(0, 1e-6): 2,      # rule 0: the increment's angle and translation fall below eps
              (0, 0.0): 4,       # rule 0 with eps = 0: only the |mse - previous mse| < 1e-12 branch can fire
              (1, 1e-6): 4}      # rule 1: the float32 sum of the increment's change
# slots whose sum is negative on source(n), n >= 63, first iteration, identity guess (14 joins them at some sizes); slot 25 (A^T b, ny) is the
# cancelling one: sum of magnitudes / |sum| = 7.6 to 26
NEGATIVE_SLOTS = (1, 2, 3, 4, 7, 10, 12, 17, 19, 21, 23, 25, 26)


def bad_normal_target():
    """The target with NaN and inf normals on every seventh point."""
    x, n = target()
    n = n.copy()
    n[0::14, 1] = np.nan
    n[7::14, 2] = np.inf
    return x, n


def coplanar(m):
    """m points of the plane z = 0.25 with the normal (0, 0, 1): (target xyz, normals, source = the target moved inside the plane)."""
    g = np.random.default_rng(100 + m)
    x = np.stack([g.uniform(0.1, 0.6, m), g.uniform(0.1, 0.6, m), np.full(m, 0.25)], 1).astype(F)
    n = np.tile(np.array([0, 0, 1], F), (m, 1))
    s = (x + np.array([0.002, -0.001, 0.0], F)).astype(F)
    return x, n, s

# ---- the correspondence chain (k_find_corr / k_ransac_match -> k_count_blocks -> k_scan_blocks -> k_compact) ----------------------------
CHAIN_SIZES = (1, 256, 257, 2048, 2049, 65536 + 1, 262144 + 257)
CHAIN_DIST = 0.015
# blocks of 256 source points that receive crafted matches: the first, both sides of the 8 blocks of one k_count_blocks workgroup, of its 32 strided
# partial vectors (32 x 8 = 256 blocks), of the 1024 blocks of one k_scan_blocks trip, and the last
CHAIN_BLOCKS = (0, 7, 8, 9, 255, 256, 257, 1022, 1023, 1024, 1025)


def chain_source(n, kind="edges"):
    """(xyz, normals, crafted source indices) of n source points for the target(): all of them far outside the target's box except the crafted
    ones -- copies of target points moved by 1 mm, of which every third has its normal flipped (fails the normal test) and every fifth is moved by
    20 mm instead (beyond CHAIN_DIST, inside the search cell).  kind: "edges" = crafted points at the start, the wave edges and the end of
    every block of CHAIN_BLOCKS and of the last block; "last" = in the last, ragged block only; "none" = no crafted point at all."""
    tx, tn = target()
    g = np.random.default_rng(1000 + n)
    xyz = g.uniform(1.5, 1.7, (n, 3)).astype(F)
    nrm = g.standard_normal((n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    nb = (n + 255) // 256
    blocks = {"edges": sorted(set(b for b in CHAIN_BLOCKS if b < nb) | {nb - 1}), "last": [nb - 1], "none": []}[kind]
    where = []
    for b in blocks:
        offs = set([0, 1, 63, 64, 127, 128, 191, 192, 255]) | set(int(v) for v in g.integers(0, 256, 6))
        where += [b * 256 + o for o in sorted(offs) if b * 256 + o < n]
    where = np.array(where, np.int64)
    pick = g.choice(len(tx), len(where), replace=len(where) > len(tx))
    for j, (k, t) in enumerate(zip(where, pick)):
        step = 0.020 if j % 5 == 4 else 0.001
        xyz[k] = (tx[t].astype(np.float64) + step * tn[t].astype(np.float64)).astype(F)
        nrm[k] = -tn[t] if j % 3 == 2 else tn[t]
    return xyz, nrm, where
