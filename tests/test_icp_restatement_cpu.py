"""tests/icp_restatement.py is not its own judge: its loop must reproduce oracle/icp_oracle.cpp (the CPU statement of PCL's loop that
tests/test_icp_oracle.py holds the library to) on the fixtures of tests/icp_cases.py -- iteration counts and `converged` equal, every
entry of T within 2 float32 ulp -- and the fixtures must be where tests/test_icp_shapes_gpu.py needs them.  No device.

One difference is measured here rather than hidden: the oracle forms the six products of two normal components (slots 15..20) as float32
products and widens them (nx * nx of two floats), the kernel -- and therefore the restatement the GPU tests use -- multiplies the widened
components in float64.  With float32 normal products the restatement equals the oracle bit for bit at every size from 6 points up; with
float64 products T moves by up to 4 ulp of an entry (identity guess, rule 1, 512 points).  The two row sets differ in those six slots
only, by at most 2^-24 of each value (test_the_kernels_normal_products_differ_from_the_oracles_only_in_six_slots)."""
from fractions import Fraction

import numpy as np
import pytest

import icp_cases as cases
import icp_restatement as R
from oracle.pyoracle import IcpOracle

F = np.float32
_cache = {}


def oracle_target():
    if "t" not in _cache:
        x, n = cases.target()
        _cache["t"] = IcpOracle(x, n, cases.CELL)
    return _cache["t"]


def ulps(T, ref):
    ref = np.asarray(ref, F)
    return np.abs(np.asarray(T, np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)


@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("gname,stop_rule,eps", [("identity", 0, 1e-6), ("guess", 1, 1e-6), ("guess", 0, 0.0)])
def test_restated_loop_equals_the_oracle(gname, stop_rule, eps, n):
    x, nr = cases.target()
    s, g = cases.source(n), cases.GUESSES[gname]
    trace = []
    T, it, cv = R.align(s, x, nr, g, cases.MAX_DIST, 20, eps, stop_rule, trace=trace, normal_products=F)
    To, ito, cvo, _ = IcpOracle(s, np.zeros_like(s), cases.CELL).align(oracle_target(), g, cases.MAX_DIST, 20, eps, stop_rule)
    assert (it, cv) == (ito, cvo)
    if n >= 6:
        assert (it, cv) == (cases.KNOWN_STOP[(stop_rule, eps)], True)
        assert ulps(T, To).max() <= 2
        for row in trace:                                     # the conditions the GPU test's increment check relies on
            assert row["totals"][28] == n
            cond = np.linalg.cond(R.system(row["totals"])[0])
            assert cond <= 200 and cond * R.U <= 2.0 ** -40
    elif n < 3:
        assert it == 0 and not cv and np.array_equal(T, g) and len(trace) == 1 and trace[0]["totals"][28] == n
    # n = 3, 5: fewer rows than unknowns -- the solve divides rounding noise by rounding noise, T is not comparable


def test_the_kernels_normal_products_differ_from_the_oracles_only_in_six_slots():
    x, nr = cases.target()
    W64, k64, _ = R.row_values(cases.source(2049), x, nr, cases.MAX_DIST)
    W32, k32, _ = R.row_values(cases.source(2049), x, nr, cases.MAX_DIST, normal_products=F)
    assert np.array_equal(k64, k32)
    same = [t for t in range(29) if np.array_equal(W64[:, t], W32[:, t])]
    assert same == [t for t in range(29) if not 15 <= t <= 20]
    assert (np.abs(W64[:, 15:21] - W32[:, 15:21]) <= 2.0 ** -24 * np.abs(W64[:, 15:21])).all()


def test_exact_sums_are_exact():
    g = np.random.default_rng(3)
    v = g.standard_normal(3000) * np.exp2(g.integers(-40, 40, 3000))
    v[::7] = 0.0
    want = sum((Fraction(float(q)) for q in v), Fraction(0))
    assert R.exact_column_sum(v) == want
    assert R.exact_column_sum(np.zeros(5)) == 0 and R.exact_column_sum(np.zeros(0)) == 0
    assert R.exact_column_sum(np.array([1e300, -1e300, 2.0 ** -1000])) == Fraction(2) ** -1000


def test_negative_and_cancelling_slots_come_with_the_fixtures():
    x, nr = cases.target()
    for n in (63, 257, 4097):
        S, A = R.exact_sums(R.row_values(cases.source(n), x, nr, cases.MAX_DIST)[0])
        assert all(S[t] < 0 for t in cases.NEGATIVE_SLOTS)
        assert 7 <= A[25] / abs(S[25]) <= 27


def test_edge_point_sits_exactly_on_max_dist():
    for off, d_want, n_kept in ((cases.EDGE_EXACT, 2.0 ** -10, 65), (cases.EDGE_ABOVE, 2.0 ** -10 + 2.0 ** -32, 64)):
        tx, _, sx = cases.with_edge_point(off)
        idx, d = R.nearest(sx, tx)
        assert idx[-1] == len(tx) - 1 and float(d[-1]) == d_want
        assert (d[:-1] == 0).all() and (idx[:-1] == np.arange(64)).all()
        assert R.kept(d, cases.MAX_DIST).sum() == n_kept
        assert (d.astype(np.float64) < cases.MAX_DIST ** 2).sum() == 64            # what the pre-check and FindCorrespondence keep


def test_bad_normals_are_matched_and_leave_only_distance_and_count():
    x, nr = cases.bad_normal_target()
    W, k, i = R.row_values(cases.source(513), x, nr, cases.MAX_DIST)
    bad = ~np.isfinite(nr[i]).all(axis=1)
    assert len(k) == 513 and 50 <= bad.sum() <= 100
    assert np.isnan(nr[i][bad]).any() and np.isinf(nr[i][bad]).any()
    assert (W[bad, :27] == 0).all() and (W[bad, 28] == 1).all() and (W[bad, 27] > 0).all() and np.isfinite(W).all()


def test_flat_corner_copy_has_exactly_zero_residuals():
    x, nr = cases.flat_corner()
    W, k, i = R.row_values(x[:300], x, nr, cases.MAX_DIST)
    assert len(k) == 300 and (i == np.arange(300)).all() and (W[:, 21:28] == 0).all()
    T, it, cv = R.align(x[:300], x, nr, np.eye(4, dtype=F), cases.MAX_DIST)
    assert it == 1 and cv and np.array_equal(T.view(np.uint32), np.eye(4, dtype=F).view(np.uint32))
    D = R.construct_increment(np.zeros(6))
    assert (D == np.eye(4, dtype=F)).all() and np.signbit(D[2, 0])                  # -sin(0) is stored as -0.0


@pytest.mark.parametrize("m", [3, 300])
def test_coplanar_points_leave_three_zero_columns_and_no_solution(m):
    x, nr, s = cases.coplanar(m)
    W, k, _ = R.row_values(s, x, nr, cases.MAX_DIST)
    assert len(k) == m
    A, b = R.system(W.sum(axis=0))
    assert [c for c in range(6) if not A[:, c].any()] == [2, 3, 4]
    assert R.solve6(A, b) is None
    g = cases.GUESSES["identity"]
    T, it, cv = R.align(s, x, nr, g, cases.MAX_DIST)
    assert it == 0 and not cv and np.array_equal(T, g)


@pytest.mark.parametrize("max_iter", [0, 1])
def test_iteration_limit_of_zero_and_one_both_run_one_iteration(max_iter):
    x, nr = cases.target()
    s, g = cases.source(65), cases.GUESSES["identity"]
    T, it, cv = R.align(s, x, nr, g, cases.MAX_DIST, max_iter, normal_products=F)
    To, ito, cvo, _ = IcpOracle(s, np.zeros_like(s), cases.CELL).align(oracle_target(), g, cases.MAX_DIST, max_iter)
    assert (it, cv) == (1, True) == (ito, cvo) and ulps(T, To).max() <= 2
