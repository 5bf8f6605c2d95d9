"""CPU checks of the path-B oracle (oracle/icp_oracle.cpp).  PCL/FLANN are absent, so parity of the ICP
step is UNPINNED; these are the pins that exist: an independent exact-NN implementation
(scipy cKDTree), ground-truth recovery on synthetic pairs, the known-answer structure of the information
matrix (also visible in the reference's Matlab example data), and the file formats."""
import os

import numpy as np
import pytest
from scipy.spatial import cKDTree

from elasticreconstruction_amd import formats, synth
from oracle.pyoracle import IcpOracle

import helpers


def make_pair(n=60000, seed=11, rot=1.5, trans=0.015):
    frag = synth.look_at((1.5, 1.5, 1.5), (0, 0, 1)) @ np.linalg.inv(synth.basepose())
    xyz0, nrm0 = synth.sample_fragment(frag, n, seed=seed)
    xyz1, nrm1 = synth.sample_fragment(frag, n, seed=seed + 1)          # a DIFFERENT sampling of the same surfaces
    P = synth.perturbation(seed + 2, rot, trans)                        # pcd1 lives in a perturbed frame
    Pi = np.linalg.inv(P)
    xyz1 = (xyz1 @ Pi[:3, :3].T + Pi[:3, 3]).astype(np.float32)
    nrm1 = (nrm1 @ Pi[:3, :3].T).astype(np.float32)
    return (xyz0, nrm0), (xyz1, nrm1), P                                # P maps pcd1 into pcd0's frame (ground truth)


def test_exact_nn_against_ckdtree():
    (x0, n0), (x1, n1), P = make_pair()
    tgt, src = IcpOracle(x0, n0, 0.03), IcpOracle(x1, n1, 0.03)
    for T, r in ((np.eye(4), 0.03), (P, 0.03), (P, 0.015)):
        idx, sqd = src.nn_pass(tgt, T, r)
        q = (x1.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32).astype(np.float64)
        d, j = cKDTree(x0.astype(np.float64)).query(q)
        clear_in = d < r * (1 - 1e-4)
        clear_out = d > r * (1 + 1e-4)
        assert (idx[clear_out] < 0).all()
        assert (idx[clear_in] >= 0).all()
        same = idx[clear_in] == j[clear_in]
        # disagreements may only be float32-vs-float64 near-ties
        dd = np.linalg.norm(q[clear_in][~same] - x0[idx[clear_in][~same]].astype(np.float64), axis=1)
        assert np.allclose(dd, d[clear_in][~same], rtol=1e-5, atol=1e-7)
        assert same.mean() > 0.999


def test_icp_recovers_ground_truth_and_counts():
    (x0, n0), (x1, n1), P = make_pair()
    tgt, src = IcpOracle(x0, n0, 0.03), IcpOracle(x1, n1, 0.03)
    cnt = src.count_inliers(tgt, np.eye(4), 0.03)
    assert 0 < cnt <= src.n
    T, it, conv, fit = src.align(tgt, np.eye(4, dtype=np.float32), want_fitness=True)
    assert conv and 1 <= it <= 20
    R_err = np.abs(T[:3, :3].astype(np.float64) - P[:3, :3]).max()
    t_err = np.abs(T[:3, 3].astype(np.float64) - P[:3, 3]).max()
    assert R_err < 1e-3 and t_err < 1e-3, (R_err, t_err)
    assert src.count_inliers(tgt, T.astype(np.float64), 0.03) > cnt
    # both PCL stop rules end at the same place on an easy pair
    T6, it6, conv6, _ = src.align(tgt, np.eye(4, dtype=np.float32), stop_rule=1)
    assert conv6 and np.abs(T6 - T).max() < 1e-3


def test_information_matrix_known_answer_structure():
    (x0, n0), (x1, n1), P = make_pair(20000)
    tgt, src = IcpOracle(x0, n0, 0.03), IcpOracle(x1, n1, 0.03)
    pairs, info = src.find_correspondence(tgt, P, 0.015, want_info=True)
    m = pairs.shape[0]
    assert m > 1000 and (np.diff(pairs[:, 1]) > 0).all()                # ascending source index
    s = x1[pairs[:, 1]].astype(np.float64)
    assert np.array_equal(info[:3, :3], m * np.eye(3))
    S = 2 * s.sum(0)
    B = np.array([[0, S[2], -S[1]], [-S[2], 0, S[0]], [S[1], -S[0], 0]])
    assert np.allclose(info[:3, 3:], B, rtol=1e-12) and np.allclose(info[3:, :3], B.T, rtol=1e-12)
    # full formula, float64 numpy
    A = np.zeros((m, 3, 6))
    A[:, 0, 0] = A[:, 1, 1] = A[:, 2, 2] = 1
    A[:, 0, 4], A[:, 0, 5] = 2 * s[:, 2], -2 * s[:, 1]
    A[:, 1, 3], A[:, 1, 5] = -2 * s[:, 2], 2 * s[:, 0]
    A[:, 2, 3], A[:, 2, 4] = 2 * s[:, 1], -2 * s[:, 0]
    assert np.allclose(info, np.einsum("kri,krj->ij", A, A), rtol=1e-10)


def test_reference_example_files_parse_and_roundtrip(tmp_path):
    """The only real data files of the reference: format fixtures for RGBDTrajectory / RGBDInformation,
    and the known-answer structure of gt.info (N*I3 block, antisymmetric off-diagonal blocks)."""
    REF_DATA = helpers.reference_example_data(tmp_path / "ref_data")
    traj = formats.load_log(os.path.join(REF_DATA, "Trajectory", "traj_gt.log"))
    assert len(traj) == 2538 and traj[0].frame == 1
    assert np.allclose(traj[10].T[3], [0, 0, 0, 1])
    p = str(tmp_path / "t.log")
    formats.save_log(p, traj[:50])
    back = formats.load_log(p)
    assert all(np.abs(a.T - b.T).max() < 1e-8 and (a.id1, a.id2, a.frame) == (b.id1, b.id2, b.frame) for a, b in zip(traj[:50], back))
    scene = os.path.join(REF_DATA, "RegistrationEvaluation", "livingroom1")
    log, info = formats.load_log(os.path.join(scene, "gt.log")), formats.load_info(os.path.join(scene, "gt.info"))
    assert len(log) == len(info) and len(info) > 10
    for fi in info[:40]:
        N = fi.info[0, 0]
        assert N > 0 and np.array_equal(fi.info[:3, :3], N * np.eye(3))
        assert np.allclose(fi.info[:3, 3:], -fi.info[:3, 3:].T, atol=1e-6 * N)      # antisymmetric +-2*sum(s)
        assert np.allclose(fi.info, fi.info.T, atol=1e-6 * N)
    p2 = str(tmp_path / "t.info")
    formats.save_info(p2, info[:5])
    assert all(np.allclose(a.info, b.info, atol=1e-8) for a, b in zip(info[:5], formats.load_info(p2)))


def test_ransac_fitness_restatement_against_ckdtree():
    """RansacCurvature::getFitness (GlobalRegistration/RansacCurvature.h:661-704), SURVEY.md 8f-3: inlier count and
    mean squared NN distance of one hypothesis against an independent exact NN (float64 cKDTree)."""
    (x0, n0), (x1, n1), P = make_pair(n=20000)
    tgt, src = IcpOracle(x0, n0, 0.05), IcpOracle(x1, n1, 0.05)
    for M, thr in ((P.astype(np.float32), 0.05), (np.eye(4, dtype=np.float32), 0.03), (synth.perturbation(5, 60, 2.0).astype(np.float32), 0.05)):
        cnt, fit32, s64 = src.ransac_fitness(tgt, M, thr)
        q = ((M[:3, 0] * x1[:, :1] + M[:3, 1] * x1[:, 1:2]) + M[:3, 2] * x1[:, 2:3]) + M[:3, 3]      # float32, same order
        d, _ = cKDTree(x0.astype(np.float64)).query(q.astype(np.float64))
        d2 = d * d
        lim = float(np.float32(thr) * np.float32(thr))
        clear = np.abs(d2 - lim) > 1e-6 * lim
        assert abs(cnt - int((d2 < lim).sum())) <= int((~clear).sum())
        if cnt:
            assert fit32 == pytest.approx(s64 / cnt, rel=1e-4)
            assert s64 / cnt == pytest.approx(d2[d2 < lim].mean(), rel=1e-3)
        else:
            assert fit32 == np.finfo(np.float32).max


def test_ransac_inlier_lists_and_information_restatement():
    """getFitness's `inliers` / `inliers_target` and getInformation (RansacCurvature.h:680-695, :707-733) against an
    independent statement: cKDTree matches and sum A^T A built with numpy from the float32 coordinates."""
    (x0, n0), (x1, n1), P = make_pair(n=20000)
    tgt, src = IcpOracle(x0, n0, 0.05), IcpOracle(x1, n1, 0.05)

    def information(p):
        A = np.zeros((len(p), 3, 6))
        A[:, 0, 0] = A[:, 1, 1] = A[:, 2, 2] = 1.0
        two = (np.float32(2) * p).astype(np.float64)                     # 2 * sz is a float product in the reference
        A[:, 0, 4], A[:, 0, 5] = two[:, 2], -two[:, 1]
        A[:, 1, 3], A[:, 1, 5] = -two[:, 2], two[:, 0]
        A[:, 2, 3], A[:, 2, 4] = two[:, 1], -two[:, 0]
        return np.einsum("nki,nkj->ij", A, A)

    for M, thr in ((P.astype(np.float32), 0.05), (np.eye(4, dtype=np.float32), 0.02)):
        ins, int_, info_s, info_t = src.ransac_inliers(tgt, M, thr)
        cnt, _, _ = src.ransac_fitness(tgt, M, thr)
        assert len(ins) == cnt and np.all(np.diff(ins) > 0)
        q = ((M[:3, 0] * x1[:, :1] + M[:3, 1] * x1[:, 1:2]) + M[:3, 2] * x1[:, 2:3]) + M[:3, 3]
        d, nn = cKDTree(x0.astype(np.float64)).query(q.astype(np.float64))
        lim = float(np.float32(thr) * np.float32(thr))
        sure = np.abs(d * d - lim) > 1e-6 * lim
        mine = np.zeros(len(x1), bool)
        mine[ins] = True
        assert np.array_equal(mine[sure], (d * d < lim)[sure])
        dd = np.linalg.norm(q[ins].astype(np.float64) - x0[int_].astype(np.float64), axis=1)
        assert np.all(dd <= d[ins] * (1 + 1e-5) + 1e-7)                   # the listed target IS a nearest neighbour
        assert np.allclose(info_s, information(x1[ins]), rtol=1e-12, atol=1e-9)
        assert np.allclose(info_t, information(x0[int_]), rtol=1e-12, atol=1e-9)
        assert info_s[0, 0] == cnt and np.allclose(info_s, info_s.T)


def test_single_icp_step_equals_an_independent_point_to_plane_least_squares():
    """One iteration of the restated ICP (max_iter = 1) against an independent statement of the published step (Low 2004 /
    PCL's TransformationEstimationPointToPlaneLLS): cKDTree correspondences within max_dist, rows [s x n, n] and right-hand
    sides n . (d - s), numpy's least-squares solution, and the rotation Rz(gamma) Ry(beta) Rx(alpha) of the six parameters."""
    (x0, n0), (x1, n1), P = make_pair(n=30000, rot=1.0, trans=0.01)
    tgt, src = IcpOracle(x0, n0, 0.03), IcpOracle(x1, n1, 0.03)
    for guess in (np.eye(4), P @ synth.perturbation(3, 0.3, 0.003)):
        g32 = guess.astype(np.float32)
        T1, it, conv, _ = src.align(tgt, g32, max_dist=0.03, max_iter=1)
        assert it == 1
        s = ((g32[:3, 0] * x1[:, :1] + g32[:3, 1] * x1[:, 1:2]) + g32[:3, 2] * x1[:, 2:3]) + g32[:3, 3] if not np.array_equal(g32, np.eye(4, dtype=np.float32)) else x1
        s = s.astype(np.float64)
        d, j = cKDTree(x0.astype(np.float64)).query(s)
        keep = d <= 0.03 * (1 - 1e-6)
        s, q, nn = s[keep], x0[j[keep]].astype(np.float64), n0[j[keep]].astype(np.float64)
        A = np.concatenate([np.cross(s, nn), nn], axis=1)
        b = np.einsum("ij,ij->i", nn, q - s)
        x = np.linalg.lstsq(A, b, rcond=None)[0]
        ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
        Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
        Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
        Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
        D = np.eye(4)
        D[:3, :3], D[:3, 3] = Rz @ Ry @ Rx, x[3:]
        want = D @ guess
        assert np.abs(T1.astype(np.float64) - want).max() < 2e-6, np.abs(T1 - want).max()
        # and the step goes the right way
        assert np.abs((D @ guess)[:3, 3] - P[:3, 3]).max() <= np.abs(guess[:3, 3] - P[:3, 3]).max() + 1e-9


def test_pcl_golden_cases_are_reproducible_and_tie_rich(tmp_path):
    """The inputs of the real-PCL pin (tests/golden/make_golden_pcl.py): deterministic, and the lattice case really is a tie case -- every query has FOUR
    target points at bit-identical float32 distance, of which the restatements pick the lowest index (FLANN's rule is the ASSUMPTION the golden file would
    settle)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_pcl as mg
    a, b = mg.write_cases(str(tmp_path / "a")), mg.write_cases(str(tmp_path / "b"))
    assert a == b and set(a) == {"easy", "hard", "limit", "lattice"}
    name, (x0, n0), (x1, n1), G, r = mg.cases()[3]
    d = ((x1[:50, None, :] - x0[None, :, :]) ** 2)
    d = (d[..., 0] + d[..., 1]) + d[..., 2]
    best = d.min(1, keepdims=True)
    assert ((d == best).sum(1) == 4).all()
    tgt, src = IcpOracle(x0, n0, 0.03), IcpOracle(x1, n1, 0.03)
    idx, _ = src.nn_pass(tgt, np.eye(4), 0.03)
    assert np.array_equal(idx[:50], np.argmax(d == best, axis=1))           # ties -> the lowest index
    assert os.path.exists(os.path.join(tmp_path, "a", "cases.txt"))


def test_restatements_equal_real_pcl_when_its_golden_file_is_present():
    """Self-activating (missing 4): tests/golden/pcl_golden.json is written by tests/golden/make_golden_pcl.py --driver on a machine that
    HAS PCL 1.7 + FLANN (oracle/pcl_driver.cpp runs the calls of CorresApp.cpp:236-312 on the committed cases).  When it exists, both restatements of this
    repository are held against it: the nearest-neighbour indices of every query (FLANN's tie rule on the lattice case), the pre-check count, and the ICP's
    transform / iteration count / convergence flag."""
    import json
    import sys
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcl_golden.json")
    if not os.path.exists(path):
        pytest.skip("no tests/golden/pcl_golden.json: real PCL has never been run on the committed cases (INTEGRATION.md, 'Closing the PCL pin')")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_pcl as mg
    with open(path) as f:
        g = json.load(f)
    gold = {c["name"]: c for c in g["cases"]}
    import hashlib
    for name, (x0, n0), (x1, n1), G, r in mg.cases():
        c = gold[name]
        assert hashlib.sha256(x0.tobytes() + n0.tobytes() + x1.tobytes() + n1.tobytes()).hexdigest() == g["inputs_sha256"][name], "inputs of case %s do not reproduce here" % name
        tgt, src = IcpOracle(x0, n0, r), IcpOracle(x1, n1, r)
        idx, _ = src.nn_pass(tgt, G, 1e9 if False else r)
        # FLANN answers for every query, the restatement only inside the radius: compare where both answer
        inside = idx >= 0
        assert np.array_equal(idx[:64][inside[:64]], np.asarray(c["nn_first"])[: len(idx[:64])][inside[:64]]), "case %s: nearest neighbours (tie rule?)" % name
        assert src.count_inliers(tgt, G, r) == c["precheck_count"], "case %s: pre-check count" % name
        T, it, conv, _ = src.align(tgt, G.astype(np.float32), r, 20, 1e-6, 0)
        Tg = np.array([int(h, 16) for h in c["T_hex"]], np.uint32).view(np.float32).reshape(4, 4)
        assert (it, bool(conv)) == (c["iterations"], bool(c["converged"])), "case %s: iterations / converged %s vs PCL %s" % (name, (it, conv), (c["iterations"], c["converged"]))
        assert np.abs(T - Tg).max() <= 1e-6, "case %s: |T_restatement - T_pcl| = %.3g" % (name, np.abs(T - Tg).max())
