"""numpy restatement of the RANSAC pose search (er_ransac_align, include/er_hip.h): the counter-based generator, selectSamples
(GlobalRegistration/RansacCurvature.h:319-359), the pick among the k feature matches (:383-386), the polygon test in float32 without
fused multiply-add (PolyRejector.h:262-295), a float64 Kabsch estimate, thresholdNormal (:192-202) and the selection rule (:627-643).
Test infrastructure: the kernels are compared with this, never the other way round."""
import numpy as np

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def draw(seed, it, d):
    """Top 32 bits of splitmix64's output function of the counter (seed << 32) + 16 * iteration + draw.  it: uint64 array."""
    with np.errstate(over="ignore"):
        z = (np.uint64(int(seed) & 0xffffffff) << np.uint64(32)) + it.astype(np.uint64) * np.uint64(16) + np.uint64(d)
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z >> np.uint64(32)


def index_of(r, m):
    """getRandomIndex: floor(m * r / 2^32)."""
    return ((np.uint64(m) * r) >> np.uint64(32)).astype(np.int64)


def select_samples(seed, its, n, ns):
    """selectSamples for an array of iteration numbers: int64 [m, ns], each row ascending and distinct."""
    its = np.asarray(its, np.uint64)
    s = np.zeros((its.shape[0], ns), np.int64)
    for i in range(ns):
        v = index_of(draw(seed, its, i), n - i)
        active = np.ones(its.shape[0], bool)
        for j in range(i):
            ge = active & (v >= s[:, j])
            v = v + ge
            ins = active & ~ge
            if ins.any():
                s[ins, j + 1:i + 1] = s[ins, j:i]
                s[ins, j] = v[ins]
            active &= ~ins
        s[active, i] = v[active]
    return s


def pick_matches(seed, its, s, knn):
    """The matched target index of every sample: knn int [n_src, k]."""
    its = np.asarray(its, np.uint64)
    k = knn.shape[1]
    c = np.zeros_like(s)
    for i in range(s.shape[1]):
        col = index_of(draw(seed, its, 8 + i), k) if k > 1 else np.zeros(its.shape[0], np.int64)
        c[:, i] = knn[s[:, i], col]
    return c


def _sqdist32(a, b):
    d = b - a                                                     # float32
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def edge_ok(ds, dt, simsq):
    """thresholdEdgeLength on float32 squared lengths: the shorter over the longer >= simsq.  0 / 0 is NaN and fails."""
    ds, dt = np.asarray(ds, np.float32), np.asarray(dt, np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sim = np.where(ds < dt, ds / dt, dt / ds)
    assert sim.dtype == np.float32
    return sim >= np.float32(simsq)


def polygon_ok(src_xyz, tgt_xyz, s, c, similarity):
    """thresholdPolygon over all pairs of edges, float32."""
    sx, tx = np.asarray(src_xyz, np.float32), np.asarray(tgt_xyz, np.float32)
    simsq = np.float32(similarity) * np.float32(similarity)
    ok = np.ones(s.shape[0], bool)
    ns = s.shape[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(ns):
            for j in range(i + 1, ns):
                ds = _sqdist32(sx[s[:, i]], sx[s[:, j]])
                dt = _sqdist32(tx[c[:, i]], tx[c[:, j]])
                ok &= edge_ok(ds, dt, simsq)
    return ok


def kabsch(P, Q):
    """Least-squares rigid transforms of point sets P -> Q (float64 [m, ns, 3]): (M float64 [m, 4, 4], singular values [m, 3])."""
    cp, cq = P.mean(axis=1), Q.mean(axis=1)
    H = np.einsum("mia,mib->mab", P - cp[:, None], Q - cq[:, None])
    U, sv, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(np.einsum("mab,mbc->mac", U, Vt)))
    D = np.zeros((P.shape[0], 3, 3))
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = np.where(d < 0, -1.0, 1.0)
    R = np.einsum("mba,mbc,mdc->mad", Vt, D, U)                   # V D U^T
    M = np.zeros((P.shape[0], 4, 4))
    M[:, :3, :3] = R
    M[:, :3, 3] = cq - np.einsum("mab,mb->ma", R, cp)
    M[:, 3, 3] = 1.0
    return M, sv


def estimate(src_xyz, tgt_xyz, s, c):
    """(M float32 [m, 4, 4] = float64 Kabsch rounded once, singular values of the cross-covariance)."""
    P = np.asarray(src_xyz, np.float32)[s].astype(np.float64)
    Q = np.asarray(tgt_xyz, np.float32)[c].astype(np.float64)
    M, sv = kabsch(P, Q)
    return M.astype(np.float32), sv


def normal_dots(M32, src_nrm, tgt_nrm, s, c):
    """n_t . (R n_s) of every sample of every hypothesis: float32 [m, ns], float32 arithmetic in the library's order."""
    sn, tn = np.asarray(src_nrm, np.float32)[s], np.asarray(tgt_nrm, np.float32)[c]          # [m, ns, 3]
    M = np.asarray(M32, np.float32)
    out = np.zeros(s.shape, np.float32)
    with np.errstate(invalid="ignore"):
        for i in range(s.shape[1]):
            a = sn[:, i]
            nn = [(M[:, r, 0] * a[:, 0] + M[:, r, 1] * a[:, 1]) + M[:, r, 2] * a[:, 2] for r in range(3)]
            d = (tn[:, i, 0] * nn[0] + tn[:, i, 1] * nn[1]) + tn[:, i, 2] * nn[2]
            assert d.dtype == np.float32
            out[:, i] = d
    return out


def normal_min_dot(M32, src_nrm, tgt_nrm, s, c):
    """The smallest n_t . (R n_s) of each hypothesis (for printing margins; NaN as soon as one sample's is -- normal_ok is the test)."""
    d = normal_dots(M32, src_nrm, tgt_nrm, s, c)
    out = np.full(s.shape[0], np.inf, np.float32)
    for i in range(s.shape[1]):
        out = np.minimum(out, d[:, i])
    return out


def normal_ok(M32, src_nrm, tgt_nrm, s, c, cos_a):
    """thresholdNormal sample by sample: a hypothesis is rejected if and only if some sample has n_t . (R n_s) < cos_a, compared in
    float64.  A NaN dot product is not below anything, so a sample with a NaN normal never rejects -- and never hides another that does."""
    d = normal_dots(M32, src_nrm, tgt_nrm, s, c).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return ~(d < cos_a).any(axis=1)


def propose(seed, it0, it1, n_src, ns, knn, src_xyz, tgt_xyz, similarity, block=250000):
    """The iterations of [it0, it1) that pass the polygon test: (iterations int64 [m], samples [m, ns], matches [m, ns])."""
    I, S, Cc = [], [], []
    for a in range(it0, it1, block):
        its = np.arange(a, min(it1, a + block), dtype=np.uint64)
        s = select_samples(seed, its, n_src, ns)
        c = pick_matches(seed, its, s, knn)
        ok = polygon_ok(src_xyz, tgt_xyz, s, c, similarity)
        I.append(its[ok].astype(np.int64)); S.append(s[ok]); Cc.append(c[ok])
    return np.concatenate(I), np.concatenate(S), np.concatenate(Cc)


def acceptable(count, n_src, inlier_fraction, inlier_number):
    count = np.asarray(count)
    frac = count.astype(np.float32) / np.float32(n_src)
    return (count > 0) & ((frac >= np.float32(inlier_fraction)) | (count > inlier_number))


def select(iterations, count, error, n_src, inlier_fraction, inlier_number):
    """Index of the winning row (lowest error among the acceptable ones, the earliest iteration on equal error) or -1."""
    ok = acceptable(count, n_src, inlier_fraction, inlier_number)
    if not ok.any():
        return -1
    idx = np.flatnonzero(ok)
    order = np.lexsort((np.asarray(iterations)[idx], np.asarray(error)[idx]))
    return int(idx[order[0]])


def align(src_xyz, src_nrm, tgt_xyz, tgt_nrm, knn, scorer, max_iterations, nr_samples=4, similarity=0.9, inlier_fraction=0.33,
          inlier_number=30000, angle_diff=0.52359878, seed=0, chunk=1 << 20):
    """The whole loop, in chunks of `chunk` iterations carried like the library carries them.  scorer(M float32 4x4) -> (count, error).
    Returns dict(T, converged, n_inliers, error, stats, aux=(iterations, counts, errors, Ms))."""
    cos_a = np.cos(np.float64(np.float32(angle_diff)))
    best = None
    aux_i, aux_c, aux_e, aux_M = [], [], [], []
    surv = 0
    for it0 in range(0, max_iterations, chunk):
        its, s, c = propose(seed, it0, min(max_iterations, it0 + chunk), len(src_xyz), nr_samples, knn, src_xyz, tgt_xyz, similarity)
        surv += len(its)
        if not len(its):
            continue
        M32, _ = estimate(src_xyz, tgt_xyz, s, c)
        keep = normal_ok(M32, src_nrm, tgt_nrm, s, c, cos_a) & ~np.isnan(M32[:, :3, :]).any(axis=(1, 2))
        its, M32 = its[keep], M32[keep]
        sc = [scorer(M) for M in M32]
        cnt = np.array([x[0] for x in sc], np.int64)
        err = np.array([x[1] for x in sc], np.float64)
        aux_i += list(its); aux_c += list(cnt); aux_e += list(err); aux_M += list(M32)
        w = select(its, cnt, err, len(src_xyz), inlier_fraction, inlier_number)
        if w >= 0 and (best is None or (err[w], its[w]) < (best[0], best[1])):
            best = (err[w], its[w], cnt[w], M32[w])
    stats = dict(iterations=max_iterations, polygon_rejections=max_iterations - surv, normal_rejections=surv - len(aux_i), scored=len(aux_i))
    return dict(T=best[3] if best else np.eye(4, dtype=np.float32), converged=best is not None, n_inliers=int(best[2]) if best else 0,
                error=float(best[0]) if best else float(np.finfo(np.float32).max), stats=stats,
                aux=(np.array(aux_i, np.int64), np.array(aux_c, np.int64), np.array(aux_e), np.array(aux_M, np.float32).reshape(-1, 4, 4)))


def feature_knn(src_f, tgt_f, k, block=512):
    """float64 brute force: (indices [n, k], squared distances [n, k]); candidates from the expanded form, ranked by the difference form;
    equal distances go to the lower index, also where more targets tie than a row has places."""
    a, b = np.asarray(src_f, np.float64), np.asarray(tgt_f, np.float64)
    kk = min(b.shape[0], k + 8)
    bb = (b * b).sum(axis=1)
    idx = np.zeros((a.shape[0], k), np.int64)
    dist = np.zeros((a.shape[0], k))
    for r0 in range(0, a.shape[0], block):
        x = a[r0:r0 + block]
        d2 = (x * x).sum(axis=1)[:, None] + bb[None] - 2.0 * (x @ b.T)
        thr = np.partition(d2, kk - 1, axis=1)[:, kk - 1:kk]                                # every target as close as the kk-th, however many tie with it
        far = d2 > thr + 1e-9 * (np.abs(thr) + (x * x).sum(axis=1)[:, None] + bb.max())
        m = int((~far).sum(axis=1).max())
        cand = np.sort(np.argsort(far, axis=1, kind="stable")[:, :m], axis=1)             # ascending index: a stable sort then breaks ties downwards
        dd = ((x[:, None, :] - b[cand]) ** 2).sum(axis=2)
        o = np.argsort(dd, axis=1, kind="stable")[:, :k]
        idx[r0:r0 + block] = np.take_along_axis(cand, o, axis=1)
        dist[r0:r0 + block] = np.take_along_axis(dd, o, axis=1)
    return idx, dist


def common_scene(n_frag=4, points=8000, noise=0.15, outlier_frac=0.7, frs=None):
    """synth.fragment_set(n_frag, points) with landmark_features of the world positions: [(xyz, nrm, F, features)]."""
    from elasticreconstruction_amd import synth
    frs = frs if frs is not None else synth.fragment_set(n_frag, target_points=points)
    g = np.random.default_rng(5)
    out = []
    for x, n, F in frs:
        w = x.astype(np.float64) @ F[:3, :3].T + F[:3, 3]
        out.append((x, n, F, synth.landmark_features(w, seed=11, noise=noise, outlier_frac=outlier_frac, rng=g)))
    return out
