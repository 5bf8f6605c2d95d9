"""The RANSAC pose search of GlobalRegistration on the GPU (er_feature_knn, er_ransac_hypotheses, er_ransac_align; icp.global_registration)
against the numpy restatement of tests/ransac_restatement.py and the CPU oracle's getFitness.  Common scene: synth.fragment_set(4, 8000),
grid cell 0.075, landmark_features(noise 0.15, 70 % outlier rows), alignment.config's parameters, 1 000 000 iterations."""
import os

import numpy as np
import pytest

import ransac_restatement as rr
from elasticreconstruction_amd import _ffi, formats, synth
from elasticreconstruction_amd.icp import (Cloud, Features, feature_knn, global_registration, icp_align, ransac_align, ransac_hypotheses,
                                           ransac_inliers)

pytestmark = pytest.mark.gpu
ITER = 1000000
FMAX = float(np.finfo(np.float32).max)
_cache = {}


def scene():
    if "sc" not in _cache:
        sc = rr.common_scene(4)
        _cache["sc"] = sc
        _cache["clouds"] = [Cloud(x, n, 0.075) for x, n, _, _ in sc]
        _cache["feats"] = [Features(f) for _, _, _, f in sc]
    return _cache["sc"], _cache["clouds"], _cache["feats"]


def run10(seed=1, **kw):
    """fragment 1 onto fragment 0 with every scored hypothesis returned (cached per argument set)."""
    key = ("run", seed, tuple(sorted(kw.items())))
    if key not in _cache:
        _, cl, ft = scene()
        _cache[key] = ransac_align(cl[1], cl[0], ft[1], ft[0], max_iterations=ITER, seed=seed, aux_capacity=200000, **kw)
    return _cache[key]


def oracle_pair(s, t):
    from oracle.pyoracle import IcpOracle
    sc, _, _ = scene()
    return IcpOracle(sc[s][0], sc[s][1], 0.075), IcpOracle(sc[t][0], sc[t][1], 0.075)


def test_ransac_feature_knn_matches_float64_brute_force(gpu):
    g = np.random.default_rng(2)
    for ns, nt, dim in ((1000, 777, 33), (333, 2500, 20), (70, 64, 64), (1, 9, 1)):
        a, b = g.normal(size=(ns, dim)).astype(np.float32), g.normal(size=(nt, dim)).astype(np.float32)
        fa, fb = Features(a), Features(b)
        for k in (1, 2, 8):
            idx, d = feature_knn(fa, fb, k)
            ridx, rd = rr.feature_knn(a, b, k)
            assert idx.min() >= 0 and idx.max() < nt
            d64 = ((a.astype(np.float64)[:, None, :] - b.astype(np.float64)[idx]) ** 2).sum(axis=2)       # float64 distance of what the GPU chose
            bad = idx != ridx
            near = np.abs(d64 - rd) <= 1e-5 * rd
            assert (near | ~bad).all(), "a wrong neighbour (%d x %d x %d, k = %d)" % (ns, nt, dim, k)
            share = bad.any(axis=1).mean()
            print("feature_knn %d x %d x %d k=%d: %.4f %% rows with a near-tie" % (ns, nt, dim, k, 100 * share))
            assert share <= 1e-3
            assert np.allclose(d, d64, rtol=1e-5, atol=0) and (np.diff(d, axis=1) >= 0).all()
    # ties go to the lower index: duplicated target rows
    b2 = np.concatenate([b[:5], b[:5]])
    idx, _ = feature_knn(Features(b[:5]), Features(b2), 2)
    assert np.array_equal(idx, np.stack([np.arange(5), np.arange(5) + 5], axis=1))


def test_ransac_proposals_are_exact(gpu):
    sc, cl, ft = scene()
    r = run10()
    knn, _ = feature_knn(ft[1], ft[0], 2)
    its, s, c = rr.propose(1, 0, ITER, len(sc[1][0]), 4, knn, sc[1][0], sc[0][0], 0.9)
    print("proposals: %d polygon survivors of %d, stats %s" % (len(its), ITER, r.stats))
    assert r.stats["iterations"] == ITER and len(its) == ITER - r.stats["polygon_rejections"] and len(its) >= 100
    status, M = ransac_hypotheses(cl[1], cl[0], s, c)
    assert (status != 1).all()                                                               # the explicit-sample entry point agrees on every survivor
    acc = status == 0
    assert r.stats["scored"] == int(acc.sum()) == len(r.aux) and r.stats["normal_rejections"] == int((status == 2).sum())
    assert np.array_equal(r.aux["iteration"], its[acc])                                      # the same iterations, in iteration order
    assert np.array_equal(r.aux["M"].view(np.uint32), M[acc].view(np.uint32))                # from the same samples and matches
    # and iterations the restatement rejects are rejected there too
    rej = np.setdiff1d(np.arange(5000), its)[:2000].astype(np.uint64)
    s2 = rr.select_samples(1, rej, len(sc[1][0]), 4)
    st2, M2 = ransac_hypotheses(cl[1], cl[0], s2, rr.pick_matches(1, rej, s2, knn))
    assert (st2 == 1).all() and not M2.any()


def test_ransac_estimates_match_float64_kabsch(gpu):
    sc, cl, ft = scene()
    knn, _ = feature_knn(ft[1], ft[0], 2)
    its, s, c = rr.propose(1, 0, ITER, len(sc[1][0]), 4, knn, sc[1][0], sc[0][0], 0.9)
    status, M = ransac_hypotheses(cl[1], cl[0], s, c)
    R, sv = rr.estimate(sc[1][0], sc[0][0], s, c)
    ok = sv[:, 1] >= 1e-6 * sv[:, 0]
    assert (~ok).mean() <= 0.01
    tol = np.spacing(np.maximum(np.abs(R), np.float32(1.0)).astype(np.float32))
    diff = np.abs(M.astype(np.float64) - R.astype(np.float64))
    print("estimates: %d sample sets, %d left out, worst |dM| / ulp = %.3f" % (len(its), int((~ok).sum()), float((diff[ok] / tol[ok]).max())))
    assert (diff[ok] <= tol[ok]).all()
    cos_a = np.cos(np.float64(np.float32(0.52359878)))
    md = rr.normal_min_dot(R, sc[1][1], sc[0][1], s, c).astype(np.float64)
    close = np.abs(md - cos_a) <= 1e-5
    assert close.mean() <= 0.01
    assert np.array_equal((status == 0)[~close], (md >= cos_a)[~close])
    # three and six samples through the same entry point
    for ns in (3, 6):
        q = np.arange(400, dtype=np.uint64)
        s3 = rr.select_samples(9, q, len(sc[1][0]), ns)
        t3 = (s3 * 7 + 3) % len(sc[0][0])
        st3, M3 = ransac_hypotheses(cl[1], cl[0], s3, t3, similarity=0.0)
        R3, sv3 = rr.estimate(sc[1][0], sc[0][0], s3, t3)
        ok3 = sv3[:, 1] >= 1e-6 * sv3[:, 0]
        tol3 = np.spacing(np.maximum(np.abs(R3), np.float32(1.0)).astype(np.float32))
        assert (st3 != 1).all() and ok3.mean() >= 0.99
        assert (np.abs(M3.astype(np.float64) - R3.astype(np.float64))[ok3] <= tol3[ok3]).all()


def test_ransac_scores_and_selection(gpu):
    sc, cl, ft = scene()
    r = run10()
    osrc, otgt = oracle_pair(1, 0)
    assert len(r.aux) >= 50
    for row in r.aux:
        c, _, s64 = osrc.ransac_fitness(otgt, row["M"], 0.075)
        assert int(row["count"]) == c
        assert row["error"] == (pytest.approx(s64 / c, rel=1e-9) if c else FMAX)
    ok = rr.acceptable(r.aux["count"], len(sc[1][0]), 0.33, 30000)
    assert r.converged and ok.any()
    w = rr.select(r.aux["iteration"], r.aux["count"], r.aux["error"], len(sc[1][0]), 0.33, 30000)
    win = r.aux[w]
    assert ok[w] and r.n_inliers == int(win["count"]) and r.error == win["error"] and np.array_equal(r.T.view(np.uint32), win["M"].view(np.uint32))
    assert not (r.aux["error"][ok] < r.error * (1 - 1e-9)).any()
    assert not ((r.aux["error"][ok] == r.error) & (r.aux["iteration"][ok] < win["iteration"])).any()
    print("selection: %d scored, %d acceptable, winner iteration %d with %d inliers, error %.6g" % (len(r.aux), int(ok.sum()), win["iteration"], r.n_inliers, r.error))


def test_ransac_reproducible_whatever_the_chunking(gpu):
    _, cl, ft = scene()
    a = run10()
    _cache.pop(("run", 1, ()), None)
    for kw in ({}, {"chunk_iterations": 1 << 18}, {"chunk_iterations": 300007}):
        b = ransac_align(cl[1], cl[0], ft[1], ft[0], max_iterations=ITER, seed=1, aux_capacity=200000, **kw)
        assert np.array_equal(a.T.view(np.uint32), b.T.view(np.uint32)) and (a.converged, a.n_inliers, a.error, a.stats) == (b.converged, b.n_inliers, b.error, b.stats)
        assert a.aux.tobytes() == b.aux.tobytes(), kw
    o = run10(seed=2)
    assert o.aux.tobytes() != a.aux.tobytes() and o.converged
    _cache[("run", 1, ())] = a


def test_ransac_registers_the_fragments(gpu):
    """RANSAC on the thinned clouds (the first 8000 rows of the 250 000-point fragments), then ICP on the full ones from its pose."""
    big = synth.fragment_set(4, 250000, device="cuda:0")
    sc = rr.common_scene(frs=[(x[:8000], n[:8000], F) for x, n, F in big])
    cl = [Cloud(x, n, 0.075) for x, n, _, _ in sc]
    ft = [Features(f) for _, _, _, f in sc]
    full = [Cloud(x, n, 0.03) for x, n, _ in big]
    from oracle.pyoracle import IcpOracle
    oc = [IcpOracle(x, n, 0.075) for x, n, _, _ in sc]
    for s, t in ((1, 0), (2, 1), (3, 0)):
        gt = np.linalg.inv(sc[t][2]) @ sc[s][2]
        r = ransac_align(cl[s], cl[t], ft[s], ft[t], max_iterations=ITER, seed=1)
        c_gt = oc[s].ransac_fitness(oc[t], gt.astype(np.float32), 0.075)[0]
        c_r = oc[s].ransac_fitness(oc[t], r.T, 0.075)[0]
        T, it, conv, _ = icp_align(full[s], full[t], r.T, 0.03, 20, 1e-6)
        e_r, e_i = float(np.abs(r.T.astype(np.float64) - gt).max()), float(np.abs(T.astype(np.float64) - gt).max())
        print("pair %d -> %d: %d inliers against %d for the ground truth (%.4f); |T - gt|max RANSAC %.4f, after ICP (%d iterations) %.5f"
              % (s, t, c_r, c_gt, c_r / c_gt, e_r, it, e_i))
        assert r.converged and c_r == r.n_inliers and c_r >= 0.95 * c_gt
        assert e_i < 2e-3


def test_ransac_refusals_and_the_empty_result(gpu):
    sc, cl, ft = scene()
    r = ransac_align(cl[1], cl[0], ft[1], ft[0], max_iterations=200000, seed=1, inlier_fraction=0.99)
    assert not r.converged and np.array_equal(r.T, np.eye(4, dtype=np.float32)) and r.n_inliers == 0
    assert r.stats["iterations"] == 200000 and r.stats["scored"] > 0 and r.stats["polygon_rejections"] + r.stats["normal_rejections"] + r.stats["scored"] == 200000
    for kw, msg in ((dict(nr_samples=2), "two-point branch"), (dict(k_correspondences=0), "must be 1 .. 8"), (dict(similarity=1.0), "similarity"),
                    (dict(max_corr_dist=0.08), "grid cell"), (dict(inlier_fraction=1.5), "inlier fraction"), (dict(nr_samples=7), "3 .. 6")):
        with pytest.raises(_ffi.ErError, match=msg):
            ransac_align(cl[1], cl[0], ft[1], ft[0], max_iterations=1000, **kw)
    with pytest.raises(_ffi.ErError, match="one-to-one"):
        ransac_align(cl[1], cl[0], Features(sc[1][3][:-1]), ft[0], max_iterations=1000)
    with pytest.raises(_ffi.ErError, match="dimensions"):
        ransac_align(cl[1], cl[0], Features(sc[1][3][:, :20]), ft[0], max_iterations=1000)
    with pytest.raises(_ffi.ErError, match="outside its cloud"):
        ransac_hypotheses(cl[1], cl[0], [[0, 1, 2, len(sc[1][0])]], [[0, 1, 2, 3]])
    with pytest.raises(_ffi.ErError, match="not finite"):
        Features(np.full((4, 33), np.nan, np.float32))


def test_ransac_global_registration_with_smart_swap(gpu, tmp_path):
    sc, _, _ = scene()
    sub = [sc[0], sc[1], (sc[2][0][:6000], sc[2][1][:6000], sc[2][2], sc[2][3][:6000])]       # fragment 2 is the smallest: (0, 2) and (1, 2) keep it as the object
    sub = [sub[2], sub[0], sub[1]]                                                           # ... put first, it is the scene of (0, 1) and (0, 2): both swap
    cl = [Cloud(x, n, 0.075) for x, n, _, _ in sub]
    ft = [Features(f) for _, _, _, f in sub]
    kw = dict(max_iterations=500000, seed=3)
    traj, info = global_registration(cl, ft, **kw)
    assert [(t.id1, t.id2, t.frame) for t in traj] == [(0, 1, 3), (0, 2, 3), (1, 2, 3)] == [(t.id1, t.id2, t.frame) for t in info]
    r = ransac_align(cl[0], cl[1], ft[0], ft[1], **kw)                                       # the swapped pair (0, 1): the smaller cloud 0 is the source
    assert np.array_equal(traj[0].T, np.linalg.inv(r.T).astype(np.float32).astype(np.float64))
    assert np.array_equal(info[0].info, ransac_inliers(cl[0], cl[1], r.T, 0.075)[4])         # information_target_
    r12 = ransac_align(cl[2], cl[1], ft[2], ft[1], **kw)                                     # not swapped: object 2 onto scene 1
    assert np.array_equal(traj[2].T, r12.T.astype(np.float64)) and np.array_equal(info[2].info, ransac_inliers(cl[2], cl[1], r12.T, 0.075)[3])
    for t, (i, j) in zip(traj, ((0, 1), (0, 2), (1, 2))):
        gt = np.linalg.inv(sub[i][2]) @ sub[j][2]
        assert np.abs(t.T - gt).max() < 0.1
    formats.save_log(str(tmp_path / "result.txt"), traj)
    formats.save_info(str(tmp_path / "result.info"), info)
    back, iback = formats.load_log(str(tmp_path / "result.txt")), formats.load_info(str(tmp_path / "result.info"))
    assert len(back) == 3 and all(np.allclose(a.T, b.T, atol=1e-8) and (a.id1, a.id2) == (b.id1, b.id2) for a, b in zip(traj, back))
    assert len(iback) == 3 and all(np.allclose(a.info, b.info, atol=1e-7, rtol=1e-9) for a, b in zip(info, iback))
