"""Path B after the search (er_icp.hip): the 29 sums of an ICP iteration, the solve, the increment, the composition and the stop rule, row by row
through er_icp_align_trace; and the correspondence chain (k_count_blocks, k_scan_blocks, k_compact) at the edges of its blocks.

Every iteration row is restated in numpy (tests/icp_restatement.py, held to the oracle by tests/test_icp_restatement_cpu.py) from the device's own
previous increment, so no row inherits another's error.  With S the exact sum of a slot's float64 row values, A the sum of their magnitudes,
u = 2^-53, nb = blocks of 256 source points:

    |device - S| <= 7 u A + 2 u |S| + (4 nb + 2) / fx_scale
        7 u A            a wave's butterfly is six additions deep (seven with the final pair add): (1 + u)^7 - 1 on the 64 values of a wave;
        (4 nb) / scale   one truncation towards zero per wave and slice on the way to 128-bit fixed point (below one unit each); everything after
                         that is integer addition, exact;  + 2 units of slack for the read-out's split into a high and a low word;
        2 u |S|          the two roundings of the read-out (h 2^64 + l, then the multiplication by 1 / scale is exact).
    slot 28 is the correspondence count exactly; with one source point slot 27 is the squared distance bit for bit.

Slots 1, 2, 3, 4, 7, 10, 12, 17, 19, 21, 23, 25 and 26 are negative on these fixtures and slot 25 cancels (A / |S| = 7.6 to 26), so the
negation in the fixed-point conversion and its carries are on the path of every case.

The information sums of the chain are float64 all the way: |device - S| <= D u A with D the longest addition path read off the kernels:
8 blocks added per thread in k_count_blocks + 6 levels of the wave tree + 3 additions of the 4 wave totals + ceil(parts / 32) strided partial
vectors per slice in k_scan_blocks + its 32 slices, parts = ceil(nb / 8).

What the branches looked like before this file: the synthetic fragments of the suite have 250 000 points = 977 blocks, so the second trip of
k_scan_blocks (from 1025 blocks) and its `carry` never ran; 262 401 points here give 1026 blocks.

Measured on one MI355X (each test prints its own; profiles/icp_shapes.txt): worst |device - S| / bound over every row of every case 0.244 for
the ICP sums (guess, 2049 points, row 3, slot 10; 0.1 to 0.2 is typical), 0.046 for the information sums (D = 50 to 54)."""
from fractions import Fraction

import numpy as np
import pytest

import icp_cases as cases
import icp_restatement as R
from elasticreconstruction_amd import _ffi
from elasticreconstruction_amd.icp import (Cloud, count_inliers, find_correspondence, icp_align, icp_align_batch, icp_align_trace,
                                           ransac_inliers)

pytestmark = pytest.mark.gpu

F = np.float32
U = Fraction(1, 2 ** 53)
_cache = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if np.asarray(a).dtype == F else np.uint64)


def cloud(key, make):
    if key not in _cache:
        x, n = make()
        _cache[key] = Cloud(x, n, cases.CELL)
    return _cache[key]


def target_cloud():
    return cloud("target", cases.target)


def source_cloud(n):
    return cloud(("source", n), lambda: (cases.source(n), np.zeros((n, 3), F)))


def check_rows(tr, src_xyz, tx, tn, guess, max_iter, eps, stop_rule, label):
    """Every row of a trace against the restatement of that iteration, started from the device's previous row.  Returns the worst
    error / bound of the sums."""
    n = len(src_xyz)
    nb = (n + 255) // 256
    fx = tr["fx_scale"]
    m, e = np.frexp(fx)
    assert (m == 0.5).all() and (fx > 0).all(), "scales must be powers of two"
    X = R.start_points(src_xyz, guess)
    st = R.State(guess)
    worst = (0.0, -1, -1)
    assert tr["n_rows"] == len(tr["totals"]) >= 1
    for r in range(tr["n_rows"]):
        assert not st.done, "%s: a row after the loop had ended" % label
        tot = tr["totals"][r]
        W, _, _ = R.row_values(X, tx, tn, cases.MAX_DIST)
        S, A = R.exact_sums(W)
        for t in range(29):
            assert abs(S[t]) * Fraction(float(fx[t])) < 2 ** 121
            err = abs(Fraction(float(tot[t])) - S[t])
            bound = 7 * U * A[t] + 2 * U * abs(S[t]) + Fraction(4 * nb + 2) / Fraction(float(fx[t]))
            ratio = float(err / bound)
            if ratio > worst[0]:
                worst = (ratio, r, t)
            assert err <= bound, "%s row %d slot %d: |device - S| = %.3g, bound %.3g" % (label, r, t, float(err), float(bound))
        assert tot[28] == len(W)
        if n == 1 and len(W) == 1:
            assert bits(tot[27:28])[0] == bits(W[0, 27:28])[0]
        # the decision, restated on the device's own sums
        prev_fin, prev_delta, prev_iter = st.fin.copy(), st.delta.copy(), st.iter
        dev_delta, dev_fin = tr["delta"][r], tr["fin"][r]
        A6, b = R.system(tot)
        x = None if tot[28] < 3.0 else R.solve6(A6, b)
        cond = np.linalg.cond(A6) if x is not None else np.inf
        advanced = int(tr["iter"][r]) == prev_iter + 1
        if x is None:
            assert not advanced, "%s row %d: the device solved a system the restatement refuses" % (label, r)
        elif cond * 2.0 ** -53 <= 2.0 ** -40:
            assert advanced
        else:
            assert n < 6, "%s row %d: cond %.3g skips the increment check at %d points" % (label, r, cond, n)
        if not advanced:
            assert int(tr["iter"][r]) == prev_iter and tr["done"][r] == 1 and tr["conv"][r] == 0
            assert np.array_equal(bits(dev_fin), bits(prev_fin)) and np.array_equal(bits(dev_delta), bits(prev_delta))
            st.done, st.conv = True, False
            continue
        if cond * 2.0 ** -53 <= 2.0 ** -40:
            xr = np.linalg.solve(A6, b)
            D_ref = R.increment_f64(xr)
            tol = 2.0 ** -23 * np.abs(D_ref) + 4 * cond * 2.0 ** -53 * np.abs(xr).max()
            assert (np.abs(dev_delta.astype(np.float64) - D_ref) <= tol).all(), "%s row %d: increment" % (label, r)
        assert np.array_equal(bits(dev_fin), bits(R.compose(dev_delta, prev_fin))), "%s row %d: final != increment * final" % (label, r)
        st.prev_delta, st.delta, st.fin, st.iter = prev_delta, dev_delta.copy(), dev_fin.copy(), prev_iter + 1
        stop, conv = R.stop_after(st, dev_delta, prev_delta, tot, max_iter, eps, stop_rule)
        assert (bool(tr["done"][r]), bool(tr["conv"][r])) == (stop, conv), "%s row %d: stop rule" % (label, r)
        if stop_rule == 0 and st.iter < max_iter:
            assert bits(tr["prev_mse"][r:r + 1])[0] == bits(np.array([st.prev_mse]))[0]
        st.done, st.conv = stop, conv
        X = R.apply_f32(dev_delta, X)
    assert st.done
    assert (tr["iterations"], tr["converged"]) == (st.iter, st.conv) and np.array_equal(bits(tr["T"]), bits(st.fin))
    print("%s: %d rows, worst |device - S| / bound = %.3f (row %d, slot %d)" % (label, tr["n_rows"], worst[0], worst[1], worst[2]))
    return worst[0]


def same_trace(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("totals", "fin", "delta", "T")) and all(
        np.array_equal(a[k], b[k]) for k in ("iter", "done", "conv")) and (a["iterations"], a["converged"], a["n_rows"]) == (
        b["iterations"], b["converged"], b["n_rows"]) and np.array_equal(bits(a["prev_mse"]), bits(b["prev_mse"]))


@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("gname,stop_rule,eps", [("identity", 0, 1e-6), ("guess", 1, 1e-6), ("guess", 0, 0.0)])
def test_every_iteration_row_at_every_shape(gname, stop_rule, eps, n):
    tx, tn = cases.target()
    src, g = cases.source(n), cases.GUESSES[gname]
    s, t = source_cloud(n), target_cloud()
    tr1 = icp_align_trace(s, t, g, cases.MAX_DIST, 20, eps, stop_rule, pts=1)
    tr2 = icp_align_trace(s, t, g, cases.MAX_DIST, 20, eps, stop_rule, pts=2)
    assert same_trace(tr1, tr2), "pts = 1 and pts = 2 disagree"
    check_rows(tr1, src, tx, tn, g, 20, eps, stop_rule, "%s rule %d eps %g n %d" % (gname, stop_rule, eps, n))
    if n >= 6:
        assert (tr1["iterations"], tr1["converged"]) == (cases.KNOWN_STOP[(stop_rule, eps)], True)
    T, it, cv, _ = icp_align(s, t, g, cases.MAX_DIST, 20, eps, stop_rule)
    assert (it, cv) == (tr1["iterations"], tr1["converged"]) and np.array_equal(bits(T), bits(tr1["T"]))


def test_trace_refuses_other_slice_counts():
    s, t = source_cloud(65), target_cloud()
    for pts in (0, 3, -1):
        with pytest.raises(_ffi.ErError):
            icp_align_trace(s, t, np.eye(4, dtype=F), cases.MAX_DIST, pts=pts)


def test_a_batch_of_1024_blocks_takes_two_slices_per_workgroup_and_changes_no_bit(monkeypatch):
    """675 small pairs in ONE group hold 1035 blocks, so the library itself picks two slices per workgroup for the first chunk."""
    monkeypatch.setenv("ER_ICP_GROUP", "1024")
    sizes = [n for n in cases.SIZES if n <= 769]
    reps = 45
    assert reps * sum((n + 255) // 256 for n in sizes) >= 1024 and reps * len(sizes) <= 1024
    t = target_cloud()
    srcs = [source_cloud(n) for n in sizes] * reps
    g = cases.GUESSES["guess"]
    T, it, cv, _ = icp_align_batch(srcs, [t] * len(srcs), [g] * len(srcs), cases.MAX_DIST, 20, 1e-6, 1)
    for k, n in enumerate(sizes):
        tr = icp_align_trace(source_cloud(n), t, g, cases.MAX_DIST, 20, 1e-6, 1, pts=2)
        for q in range(k, len(srcs), len(sizes)):
            assert (it[q], cv[q]) == (tr["iterations"], tr["converged"]) and np.array_equal(bits(T[q]), bits(tr["T"])), (n, q)


@pytest.mark.parametrize("max_iter", [0, 1])
def test_iteration_limit_zero_and_one(max_iter):
    tx, tn = cases.target()
    g = cases.GUESSES["identity"]
    tr = icp_align_trace(source_cloud(65), target_cloud(), g, cases.MAX_DIST, max_iter, 1e-6, 0)
    check_rows(tr, cases.source(65), tx, tn, g, max_iter, 1e-6, 0, "max_iter %d" % max_iter)
    assert (tr["n_rows"], tr["iterations"], tr["converged"]) == (1, 1, True)


def test_a_correspondence_at_exactly_max_dist_is_kept_by_icp_alone():
    g = np.eye(4, dtype=F)
    for off, cnt in ((cases.EDGE_EXACT, 65), (cases.EDGE_ABOVE, 64)):
        tx, tn, sx = cases.with_edge_point(off)
        t, s = Cloud(tx, tn, cases.CELL), Cloud(sx, np.tile(np.array([0, 0, 1], F), (65, 1)), cases.CELL)
        tr = icp_align_trace(s, t, g, cases.MAX_DIST, 20, 1e-6, 0)
        check_rows(tr, sx, tx, tn, g, 20, 1e-6, 0, "edge point %s" % ("on" if cnt == 65 else "above"))
        assert tr["totals"][0][28] == cnt
        assert count_inliers(s, t, np.eye(4), cases.MAX_DIST) == 64
        pairs, _ = find_correspondence(s, t, np.eye(4), cases.MAX_DIST, normal_cos=-2.0)
        assert len(pairs) == 64 and (pairs[:, 1] == np.arange(64)).all()


def test_non_finite_target_normals_count_and_add_no_row():
    tx, tn = cases.bad_normal_target()
    t = Cloud(tx, tn, cases.CELL)
    for gname in ("identity", "guess"):
        g = cases.GUESSES[gname]
        tr = icp_align_trace(source_cloud(513), t, g, cases.MAX_DIST, 20, 1e-6, 0)
        assert np.isfinite(tr["totals"]).all() and tr["totals"][0][28] == 513
        check_rows(tr, cases.source(513), tx, tn, g, 20, 1e-6, 0, "bad normals, %s" % gname)


def test_an_exact_copy_has_zero_residual_sums_and_an_identity_increment():
    x, nr = cases.flat_corner()
    t, s = Cloud(x, nr, cases.CELL), Cloud(x[:300], nr[:300], cases.CELL)
    g = np.eye(4, dtype=F)
    tr = icp_align_trace(s, t, g, cases.MAX_DIST, 20, 1e-6, 0)
    check_rows(tr, x[:300], x, nr, g, 20, 1e-6, 0, "exact copy")
    assert (tr["n_rows"], tr["iterations"], tr["converged"]) == (1, 1, True)
    assert (tr["totals"][0][21:28] == 0).all() and tr["totals"][0][28] == 300
    assert np.array_equal(bits(tr["T"]), bits(g))
    assert np.array_equal(bits(tr["delta"][0]), bits(R.construct_increment(np.zeros(6))))      # the identity, with -sin(0) stored as -0.0
    assert (tr["delta"][0] == g).all()


@pytest.mark.parametrize("m", [2, 3, 300])
def test_no_solution_and_too_few_correspondences_return_the_guess(m):
    """Coplanar points under one normal: three columns of the system are exactly zero, LDL^T refuses, the pivoting fallback refuses.
    m = 2: the minimum of 3 correspondences ends the loop before the solve; the count row says 2."""
    x, nr, s = cases.coplanar(max(m, 3))
    x, nr, s = x[:m], nr[:m], s[:m]
    t, sc = Cloud(x, nr, cases.CELL), Cloud(s, nr, cases.CELL)
    for gname in ("identity", "guess"):
        g = cases.GUESSES[gname]
        if gname == "guess":                                  # a guess that keeps the points in the plane's neighbourhood
            g = np.eye(4, dtype=F)
            g[0, 3] = F(0.001)
        tr = icp_align_trace(sc, t, g, cases.MAX_DIST, 20, 1e-6, 0)
        check_rows(tr, s, x, nr, g, 20, 1e-6, 0, "coplanar %d, %s" % (m, gname))
        assert (tr["n_rows"], tr["iterations"], tr["converged"]) == (1, 0, False) and tr["totals"][0][28] == m
        assert np.array_equal(bits(tr["T"]), bits(g))
        T, it, cv, _ = icp_align(sc, t, g, cases.MAX_DIST)
        assert (it, cv) == (0, False) and np.array_equal(bits(T), bits(g))


# ---- the correspondence chain ----------------------------------------------------------------------------------------------------------

def info_terms(p):
    """The ten float64 values one matched point adds to the information sums: 2x, 2y, 2z (float32 products, widened), the three diagonal and
    the three off-diagonal entries of the rotation block, one."""
    p = np.asarray(p, F).reshape(-1, 3)
    ax, ay, az = ((F(2) * p[:, a]).astype(np.float64) for a in range(3))
    return np.stack([ax, ay, az, az * az + ay * ay, az * az + ax * ax, ay * ay + ax * ax, ay * (-ax), (-az) * ax, az * (-ay), np.ones(len(p))], axis=1)


def check_information(info, pts, nb, label):
    """info 6x6 against the exact sums of info_terms(pts): counts exact, structural zeros exact, every sum within D u A."""
    parts = (nb + 7) // 8
    D = 8 + 6 + 3 + (parts + 31) // 32 + 32
    S, A = R.exact_sums(info_terms(pts))
    place = {0: [(1, 5, 1), (2, 4, -1)], 1: [(2, 3, 1), (0, 5, -1)], 2: [(0, 4, 1), (1, 3, -1)], 3: [(3, 3, 1)], 4: [(4, 4, 1)], 5: [(5, 5, 1)],
             6: [(3, 4, 1)], 7: [(3, 5, 1)], 8: [(4, 5, 1)]}
    assert np.array_equal(info, info.T)
    assert info[0, 0] == info[1, 1] == info[2, 2] == len(pts)
    seen = {(0, 0), (1, 1), (2, 2)}
    worst = 0.0
    for k, cells in place.items():
        for r, c, sign in cells:
            seen |= {(r, c), (c, r)}
            err, bound = abs(Fraction(float(info[r, c])) - sign * S[k]), D * U * A[k]
            assert err <= bound, "%s: information (%d, %d) off by %.3g, bound %.3g" % (label, r, c, float(err), float(bound))
            if bound:
                worst = max(worst, float(err / bound))
    assert all(info[r, c] == 0 for r in range(6) for c in range(6) if (r, c) not in seen)
    return worst, D


def near_target(xyz, tx, margin=0.05):
    lo, hi = tx.min(axis=0) - margin, tx.max(axis=0) + margin
    return np.nonzero(((xyz >= lo) & (xyz <= hi)).all(axis=1))[0]


CHAIN_CASES = [(n, "edges") for n in cases.CHAIN_SIZES] + [(2049, "none"), (65537, "none"), (257, "last"), (2049, "last"), (65537, "last")]


@pytest.mark.parametrize("n,kind", CHAIN_CASES)
def test_correspondence_chain_at_block_edges(n, kind):
    tx, tn = cases.target()
    xyz, nrm, where = cases.chain_source(n, kind)
    near = near_target(xyz, tx)
    assert np.array_equal(near, np.sort(where)), "only the crafted points lie near the target"
    nb = (n + 255) // 256
    s, t = Cloud(xyz, nrm, cases.CELL), target_cloud()
    idx, d = R.nearest(xyz[near], tx)
    d64 = d.astype(np.float64)
    # FindCorrespondence at the identity: distance, then the float32 normal product compared as a double
    r = float(F(cases.CHAIN_DIST))
    nn, sn = tn[idx], nrm[near]
    dot = (nn[:, 0] * sn[:, 0] + nn[:, 1] * sn[:, 1]) + nn[:, 2] * sn[:, 2]
    ok = (d64 <= r * r) & (d64 < cases.CHAIN_DIST * cases.CHAIN_DIST) & (dot.astype(np.float64) > 0.8660)
    want = np.stack([idx[ok], near[ok]], axis=1).astype(np.int32)
    pairs, info = find_correspondence(s, t, np.eye(4), cases.CHAIN_DIST, 0.8660, want_info=True)
    assert np.array_equal(pairs, want)
    w1, D = check_information(info, xyz[near[ok]], nb, "FindCorrespondence n %d %s" % (n, kind))
    # getFitness's inlier list at the identity: d < threshold^2 as floats
    thr = F(cases.CHAIN_DIST)
    hit = d < thr * thr
    inl, inl_t, fit, info_s, info_t = ransac_inliers(s, t, np.eye(4, dtype=F), cases.CHAIN_DIST)
    assert np.array_equal(inl, near[hit]) and np.array_equal(inl_t, idx[hit])
    w2, _ = check_information(info_s, xyz[near[hit]], nb, "ransac source n %d %s" % (n, kind))
    w3, _ = check_information(info_t, tx[idx[hit]], nb, "ransac target n %d %s" % (n, kind))
    if hit.any():
        Sd, Ad = R.exact_column_sum(d64[hit]), R.exact_column_sum(d64[hit])
        assert abs(Fraction(fit) * int(hit.sum()) - Sd) <= (6 + 3 + nb + 2) * U * Ad          # wave tree, 4 waves, one atomic per block, the division
    if kind == "none":
        assert len(pairs) == 0 and len(inl) == 0 and not info.any() and not info_s.any() and not info_t.any()
    else:
        assert ok.sum() >= 1 and (~ok).sum() >= (1 if len(near) >= 3 else 0)
    if kind == "last":
        assert near.min() >= (nb - 1) * 256
    print("chain n %d %s: %d of %d crafted points matched, D = %d, worst information error / bound %.3f %.3f %.3f" % (
        n, kind, ok.sum(), len(near), D, w1, w2, w3))
