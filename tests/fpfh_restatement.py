"""A numpy restatement of the first half of GlobalRegistration's do_all (GlobalRegistration.cpp:59-128): pcl::VoxelGrid, pcl::NormalEstimation
with the sign flip against the input normals, and pcl::FPFHEstimation -- written from the definitions, not from the kernels.  The kernels
of csrc/er_fpfh.hip are compared with this file, never the other way round.

Neighbourhood of point i at radius r: every j whose float32 value ((dx*dx) + dy*dy) + dz*dz is < fl32(r * r); i itself is a member.
Everything behind the float32 inputs is float64.
"""
import numpy as np
from scipy.spatial import cKDTree

DELTA = 1e-9          # a pair within DELTA of an interior bin edge is "near an edge": two float64 evaluations may disagree on its bin


def sqdist32(a, b):
    """float32, ((dx*dx) + dy*dy) + dz*dz -- no FMA."""
    d = a.astype(np.float32) - b.astype(np.float32)
    return ((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def neighbour_pairs(xyz, r):
    """All ordered pairs (i, j), i == j included, with sqdist32 < fl32(r * r): (i [m], j [m], d2 float32 [m]) sorted by (i, j)."""
    x = np.ascontiguousarray(xyz, np.float32)
    r2 = np.float32(r) * np.float32(r)
    tree = cKDTree(x.astype(np.float64))
    p = tree.query_pairs(float(r) * 1.001 + 1e-6, output_type="ndarray")          # a superset; membership is decided in float32 below
    d2 = sqdist32(x[p[:, 0]], x[p[:, 1]])
    p, d2 = p[d2 < r2], d2[d2 < r2]
    n = len(x)
    i = np.concatenate([p[:, 0], p[:, 1], np.arange(n)])
    j = np.concatenate([p[:, 1], p[:, 0], np.arange(n)])
    d = np.concatenate([d2, d2, np.zeros(n, np.float32)])
    o = np.lexsort((j, i))
    return i[o], j[o], d[o]


def neighbours_brute(xyz, r):
    """The O(n^2) float32 loop neighbour_pairs is checked against."""
    x = np.ascontiguousarray(xyz, np.float32)
    r2 = np.float32(r) * np.float32(r)
    ii, jj, dd = [], [], []
    for i in range(len(x)):
        d2 = sqdist32(x[i][None, :], x)
        j = np.nonzero(d2 < r2)[0]
        ii.append(np.full(len(j), i))
        jj.append(j)
        dd.append(d2[j])
    return np.concatenate(ii), np.concatenate(jj), np.concatenate(dd)


# ---- voxel grid ------------------------------------------------------------------------------------------------------------------
def voxel_cells(xyz, leaf):
    """(key int64 [n], ijk int64 [n, 3], min_b, div) of pcl::VoxelGrid: inv = fl32(1 / leaf), ijk = floor(fl32(x * inv))."""
    x = np.ascontiguousarray(xyz, np.float32)
    inv = np.float32(1.0) / np.float32(leaf)
    ijk = np.floor(x * inv).astype(np.int64)
    min_b, max_b = ijk.min(axis=0), ijk.max(axis=0)
    div = max_b - min_b + 1
    rel = ijk - min_b
    return rel[:, 0] + rel[:, 1] * div[0] + rel[:, 2] * div[0] * div[1], ijk, min_b, div


def voxel_grid(xyz, nrm, leaf):
    """One point per occupied cell in ascending key order; each of the six components = float64 sum / count, rounded to float32 once.
    Returns (xyz float32 [m, 3], normals float32 [m, 3], key of every output point int64 [m])."""
    key, _, _, _ = voxel_cells(xyz, leaf)
    uk, inv_idx, cnt = np.unique(key, return_inverse=True, return_counts=True)
    v = np.concatenate([np.asarray(xyz, np.float32), np.asarray(nrm, np.float32)], axis=1).astype(np.float64)
    s = np.zeros((len(uk), 6))
    np.add.at(s, inv_idx, v)                                                     # unbuffered: in file order
    m = (s / cnt[:, None].astype(np.float64)).astype(np.float32)
    return m[:, :3].copy(), m[:, 3:].copy(), uk


# ---- normals ---------------------------------------------------------------------------------------------------------------------
def normals(xyz, nrm_in, r):
    """Per point: float64 centroid and scatter matrix of its neighbourhood, the unit eigenvector of the smallest eigenvalue, negated if its
    float64 dot product with the input normal is < 0, rounded to float32; NaN where the neighbourhood has fewer than 3 points.
    Returns (normals float32 [n, 3], counts int [n], relative gap (l1 - l0) / l2 [n], |n . n_in| [n])."""
    x32 = np.ascontiguousarray(xyz, np.float32)
    x = x32.astype(np.float64)
    n = len(x)
    i, j, _ = neighbour_pairs(x32, r)
    cnt = np.bincount(i, minlength=n)
    c = np.zeros((n, 3))
    np.add.at(c, i, x[j])
    c /= cnt[:, None]
    d = x[j] - c[i]
    S = np.zeros((n, 3, 3))
    np.add.at(S, i, d[:, :, None] * d[:, None, :])
    lam, vec = np.linalg.eigh(S)
    v = vec[:, :, 0]
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    ni = np.asarray(nrm_in, np.float32).astype(np.float64)
    dot = (v[:, 0] * ni[:, 0] + v[:, 1] * ni[:, 1]) + v[:, 2] * ni[:, 2]
    v = np.where((dot < 0.0)[:, None], -v, v)
    out = v.astype(np.float32)
    out[cnt < 3] = np.nan
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
    return out, cnt, gap, np.abs(dot)


# ---- pair features ---------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def pair_features(p1, n1, p2, n2):
    """pcl::computePairFeatures for p1, n1 = the point and p2, n2 = the neighbour (float32 in, float64 behind):
    (ok [m], bin coordinates b [m, 3]) with b1 = 11 (f1 + pi) / (2 pi), b2 = 11 (f2 + 1) / 2, b3 = 11 (f3 + 1) / 2."""
    p1, n1, p2, n2 = (np.asarray(a, np.float32).astype(np.float64).reshape(-1, 3) for a in (p1, n1, p2, n2))
    with np.errstate(all="ignore"):
        d = p2 - p1
        f4 = np.sqrt(_dot(d, d))
        ok = (f4 != 0.0) & np.isfinite(n1).all(axis=1) & np.isfinite(n2).all(axis=1)
        a1, a2 = _dot(n1, d) / f4, _dot(n2, d) / f4
        sw = np.abs(a1) < np.abs(a2)
        na = np.where(sw[:, None], n2, n1)
        nb = np.where(sw[:, None], n1, n2)
        d = np.where(sw[:, None], -d, d)
        f3 = np.where(sw, -a2, a1)
        v = _cross(d, na)
        vn = np.sqrt(_dot(v, v))
        ok &= vn != 0.0
        v = v / vn[:, None]
        w = _cross(na, v)
        f2 = _dot(v, nb)
        f1 = np.arctan2(_dot(w, nb), _dot(na, nb))
        b = np.stack([11.0 * (f1 + np.pi) / (2.0 * np.pi), 11.0 * (f2 + 1.0) / 2.0, 11.0 * (f3 + 1.0) / 2.0], axis=1)
    return ok, b


def bins_of(b):
    return np.clip(np.floor(b), 0, 10).astype(np.int64)


def near_edge(b):
    """True where one of the three coordinates lies within DELTA of an INTERIOR edge 1 .. 10 (the outer edges are clamped away)."""
    e = np.rint(b)
    return ((np.abs(b - e) < DELTA) & (e >= 1) & (e <= 10)).any(axis=1)


# ---- SPFH / FPFH -----------------------------------------------------------------------------------------------------------------
def spfh(xyz, nrm, r):
    """Integer bin counts [n, 33] over every point's neighbours other than itself (failed pairs skipped), the neighbourhood sizes [n]
    (the point included; m_i = size - 1 counts failed pairs too), the near-edge pairs per point [n], and the pair arrays (i, j, d2)."""
    x = np.ascontiguousarray(xyz, np.float32)
    nr = np.ascontiguousarray(nrm, np.float32)
    n = len(x)
    i, j, d2 = neighbour_pairs(x, r)
    nn = np.bincount(i, minlength=n)
    o = i != j
    io, jo = i[o], j[o]
    ok, b = pair_features(x[io], nr[io], x[jo], nr[jo])
    bn = bins_of(b[ok])
    counts = np.zeros((n, 33), np.int64)
    for k in range(3):
        np.add.at(counts, (io[ok], 11 * k + bn[:, k]), 1)
    edge = np.bincount(io[ok], weights=near_edge(b[ok]).astype(np.float64), minlength=n).astype(np.int64)
    return counts, nn, edge, (i, j, d2)


def fpfh(nrm, counts, nn, pairs):
    """Per bin the float64 sum over neighbours j with d2 != 0 of spfh_j[bin] * (1 / (double) d2), spfh_j = count * 100 / m_j; every block of 11
    scaled by 100 / sum when its sum is not 0; float32.  A point whose own normal is not finite gets a zero row."""
    i, j, d2 = pairs
    n = len(nn)
    m = (nn - 1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        row = np.where(m[:, None] > 0, counts.astype(np.float64) * 100.0 / m[:, None], 0.0)
    o = d2 != 0
    w = 1.0 / d2[o].astype(np.float64)
    acc = np.zeros((n, 33))
    np.add.at(acc, i[o], row[j[o]] * w[:, None])
    for k in range(3):
        blk = acc[:, 11 * k:11 * k + 11]
        s = blk.sum(axis=1)
        blk *= np.where(s != 0, 100.0 / np.where(s != 0, s, 1.0), 1.0)[:, None]
    out = acc.astype(np.float32)
    out[~np.isfinite(np.asarray(nrm, np.float32)).all(axis=1)] = 0.0
    return out


def preprocess(xyz, nrm, leaf=0.05, normal_radius=0.1, feature_radius=0.25):
    """The chain on the host: dict(xyz, nrm_down, nrm, n_counts, gap, absdot, counts, nn, edge, feat)."""
    x, nd, _ = voxel_grid(xyz, nrm, leaf)
    ne, ncnt, gap, absdot = normals(x, nd, normal_radius)
    counts, nn, edge, pairs = spfh(x, ne, feature_radius)
    return dict(xyz=x, nrm_down=nd, nrm=ne, n_counts=ncnt, gap=gap, absdot=absdot, counts=counts, nn=nn, edge=edge,
                feat=fpfh(ne, counts, nn, pairs), pairs=pairs)


def match_share(pre_s, pre_t, F_s, F_t, k=2, dist=0.075):
    """Of the (source point, one of its k nearest target descriptors) picks, the share whose target point lies within `dist` of the
    source point once both are in the world frame."""
    fs, ft = pre_s["feat"].astype(np.float64), pre_t["feat"].astype(np.float64)
    idx = cKDTree(ft).query(fs, k=k)[1].reshape(len(fs), k)
    return match_share_of(idx, pre_s["xyz"], pre_t["xyz"], F_s, F_t, dist)


def match_share_of(idx, xs, xt, F_s, F_t, dist=0.075):
    ws = xs.astype(np.float64) @ F_s[:3, :3].T + F_s[:3, 3]
    wt = xt.astype(np.float64) @ F_t[:3, :3].T + F_t[:3, 3]
    d = np.linalg.norm(ws[:, None, :] - wt[idx], axis=2)
    return float((d < dist).mean())
