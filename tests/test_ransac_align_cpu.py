"""The RANSAC pose search (er_ransac_align and its parts), the part that needs no GPU: the entry points at the C ABI, the seeded
descriptor of the tests, and the numpy restatement of the search (tests/ransac_restatement.py) on its own -- on the common scene it must
converge and reach 0.95 of the ground-truth pose's inlier count, the bar tests/test_ransac_align_gpu.py sets for the kernels, so that
the bar is shown to be one the method meets without them."""
import ctypes as C
import os

import numpy as np

import ransac_restatement as rr
from elasticreconstruction_amd import _ffi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("er_features_create", "er_features_destroy", "er_features_size", "er_feature_knn", "er_ransac_hypotheses", "er_ransac_params_default",
       "er_ransac_align")


def test_ransac_entry_points_are_declared_bound_and_refuse_to_run_without_a_device():
    hdr = open(os.path.join(ROOT, "include", "er_hip.h")).read()
    L = _ffi.lib()
    for name in NEW:
        assert name + "(" in hdr and name in _ffi.SYMBOLS and hasattr(L, name), name
    p = _ffi.ErRansacParams()
    assert L.er_ransac_params_default(C.byref(p)) == 0
    assert (p.max_iterations, p.nr_samples, p.k_correspondences, p.inlier_number, p.chunk_iterations) == (4000000, 4, 2, 30000, 0)
    assert abs(p.similarity - 0.9) < 1e-6 and abs(p.max_corr_dist - 0.075) < 1e-6 and abs(p.inlier_fraction - 0.33) < 1e-6 and abs(p.angle_diff - 0.52359878) < 1e-6
    import pytest
    import torch
    if torch.cuda.is_available():
        return
    from elasticreconstruction_amd.icp import Features
    with pytest.raises(_ffi.ErError, match="no HIP device"):
        Features(np.zeros((10, 33), np.float32))
    for call in (lambda: L.er_feature_knn(None, None, 1, None, None),
                 lambda: L.er_ransac_hypotheses(None, None, 0, 4, None, None, C.c_float(0.9), C.c_float(0.5), None, None),
                 lambda: L.er_ransac_align(None, None, None, None, C.byref(p), None, None, None, None, None, None, 0, None)):
        assert call() != 0 and "no HIP device" in L.er_last_error().decode()


def test_landmark_features_are_deterministic_and_shared_between_fragments():
    x = np.random.default_rng(0).random((500, 3)) * 3
    a = synth.landmark_features(x, seed=11, noise=0.15, outlier_frac=0.7, rng=5)
    b = synth.landmark_features(x, seed=11, noise=0.15, outlier_frac=0.7, rng=np.random.default_rng(5))
    assert a.dtype == np.float32 and a.shape == (500, 33) and np.array_equal(a, b)
    clean = synth.landmark_features(x, seed=11, noise=0.0, outlier_frac=0.0, rng=1)
    assert np.array_equal(clean, synth.landmark_features(x, seed=11, noise=0.0, outlier_frac=0.0, rng=2))       # the world position alone
    assert not np.array_equal(clean, synth.landmark_features(x, seed=12, noise=0.0, outlier_frac=0.0, rng=1))
    inl = np.abs(a - clean).max(axis=1) < 1.0                                                # rows that are the signal plus 0.15 noise
    assert 0.2 < inl.mean() < 0.4


def test_generator_and_select_samples_restatement():
    its = np.arange(20000, dtype=np.uint64)
    s = rr.select_samples(7, its, 50, 6)
    assert (np.diff(s, axis=1) > 0).all() and s.min() == 0 and s.max() == 49                 # distinct, ascending, the whole range
    # the scalar procedure of RansacCurvature.h:334-358, literally, for a few rows
    for r in (0, 1, 77, 19999):
        out = []
        for i in range(6):
            v = int(rr.index_of(rr.draw(7, its[r:r + 1], i), 50 - i)[0])
            out.append(v)
            for j in range(i):
                if out[i] >= out[j]:
                    out[i] += 1
                else:
                    t = out[i]
                    for k in range(i, j, -1):
                        out[k] = out[k - 1]
                    out[j] = t
                    break
        assert out == list(s[r])
    assert int(rr.draw(0, np.zeros(1, np.uint64), 0)[0]) == 0xE220A8397B1DCDAF >> 32       # splitmix64's first output for state 0
    u = rr.draw(3, its, 1).astype(np.float64) / 2.0 ** 32
    assert abs(u.mean() - 0.5) < 0.01 and abs(np.corrcoef(u[:-1], u[1:])[0, 1]) < 0.03


def test_normal_test_is_per_sample_and_a_nan_normal_never_rejects():
    """thresholdNormal (RansacCurvature.h:192-202) tests each sample on its own: `nt.dot(nn) < cos` is false for a NaN, so a NaN normal
    neither rejects nor shields a bad sample next to it.  Folding the dot products with a NaN-propagating minimum first, as the
    restatement once did, keeps the first case below."""
    nan = np.float32(np.nan)
    c30 = np.cos(np.float64(np.float32(0.52359878)))
    good, bad = [0.0, 0.0, 1.0], [0.0, np.sin(1.0), np.cos(1.0)]                             # against a target normal z: dot 1 and cos(1 rad) = 0.54
    for ns in (3, 4, 6):
        src = np.array([[nan] * 3, bad, good, [nan, 0.0, 1.0]] + [good] * 4, np.float32)
        tgt = np.zeros((8, 3), np.float32)
        tgt[:, 2] = 1.0
        tgt_nan = tgt.copy()
        tgt_nan[:] = nan
        M = np.broadcast_to(np.eye(4, dtype=np.float32), (5, 4, 4))
        rest = [2, 4, 5, 6, 7]
        s = np.array([[0, 1] + rest[:ns - 2],                                                # one NaN sample and one below the cosine
                      [1, 0] + rest[:ns - 2],                                                # the same, the bad one first
                      [0] + rest[:ns - 1],                                                   # one NaN sample, the others above
                      [3] + rest[:ns - 1],                                                   # (one NaN component is a NaN sample)
                      rest[:ns - 1] + [1]])                                                  # no NaN, one below
        c = np.broadcast_to(np.arange(ns), s.shape)
        new = rr.normal_ok(M, src, tgt, s, c, c30)
        with np.errstate(invalid="ignore"):
            old = ~(rr.normal_min_dot(M, src, tgt, s, c).astype(np.float64) < c30)
        assert list(new) == [False, False, True, True, False]
        assert list(old) == [True, True, True, True, False]                                  # what the folded minimum gave: it differs in the first kind
        assert rr.normal_ok(M, np.full_like(src, nan), tgt, s, c, c30).all()                 # all samples NaN: kept
        assert rr.normal_ok(M, src, tgt_nan, s, c, c30).all()


def test_restatement_alone_registers_the_common_scene():
    from oracle.pyoracle import IcpOracle
    sc = rr.common_scene(2)
    (x0, n0, F0, f0), (x1, n1, F1, f1) = sc
    knn, _ = rr.feature_knn(f1, f0, 2)
    src, tgt = IcpOracle(x1, n1, 0.075), IcpOracle(x0, n0, 0.075)

    def scorer(M):
        c, _, s64 = src.ransac_fitness(tgt, M, 0.075)
        return c, (s64 / c if c else float(np.finfo(np.float32).max))

    kw = dict(max_iterations=100000, seed=1)
    a = rr.align(x1, n1, x0, n0, knn, scorer, chunk=100000, **kw)
    b = rr.align(x1, n1, x0, n0, knn, scorer, chunk=30000, **kw)
    assert a["converged"] and a["stats"] == b["stats"] and a["n_inliers"] == b["n_inliers"] and a["error"] == b["error"]
    assert np.array_equal(a["T"], b["T"]) and all(np.array_equal(p, q) for p, q in zip(a["aux"], b["aux"]))
    gt = (np.linalg.inv(F0) @ F1).astype(np.float32)
    c_gt, _ = scorer(gt)
    print("restatement alone: %s, %d inliers against %d for the ground truth (%.4f)" % (a["stats"], a["n_inliers"], c_gt, a["n_inliers"] / c_gt))
    assert a["stats"]["scored"] >= 5
    assert a["n_inliers"] >= 0.95 * c_gt
