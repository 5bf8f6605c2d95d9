"""High-precision restatement of the sums the FragmentOptimizer assembly forms (helper, no tests in here).

The bucket ARITHMETIC -- one correspondence's values and matrix indices -- is taken from oracle/fopt_oracle.cpp through
FoptOracle.rigid_bucket / slac_bucket / nonrigid_bucket (pinned to the reference header by tests/test_fopt_oracle.py).  Only the
PLACEMENT rule is restated here, and every entry of every system is summed in np.longdouble (64-bit mantissa on x86) together with
the sum of the absolute values of its addends and their number.  That is what an entry-wise bound needs:

    n additions and n rounded products, each with relative error u = 2^-53, move an entry by at most 2 n u A to first order,
    A = sum |addend| -- whatever the order of the sum, whether the products were rounded (the CPU oracle) or fused into the
    accumulation (the FP64 matrix cores), and however many atomics the chunks of a group add with.

An entry with ONE addend must be that float64 product bit for bit; an entry with none must be exactly 0.0.  (The longdouble products
are themselves rounded to 64 bits: 2^-64 A per addend, 2^-11 of the bound.)
"""
import numpy as np

U = 2.0 ** -53


def require_longdouble():
    """np.longdouble has to be the x87 80-bit type; anything narrower cannot referee float64 sums."""
    import pytest
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("np.longdouble has a %d-bit mantissa here, the reference sums need 64" % (np.finfo(np.longdouble).nmant + 1))
    assert np.finfo(np.longdouble).nmant >= 63


def _segment_sum(v, order, starts):
    return np.add.reduceat(v[order], starts) if v.size else v[:0]


class Sums:
    """Per-entry sums of one system, kept for the touched entries only (a dense non-rigid matrix does not fit at resolution 8):
    keys = flat index row * shape[1] + col, ascending;  S = sum, A = sum |addend| (np.longdouble), n = number of addends,
    P = the float64 sum of the float64 addends in list order -- at n == 1 the single float64 product."""

    def __init__(self, shape, keys, a, b, factor=None):
        """addend = factor * a * b (factor: exact powers of two, or None); a, b float64 arrays of the shape of keys."""
        self.shape = tuple(int(s) for s in shape)
        keys = np.asarray(keys, np.int64).reshape(-1)
        a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
        p64 = a * b
        pld = a.astype(np.longdouble) * b.astype(np.longdouble)
        if factor is not None:
            f = np.asarray(factor, np.float64).reshape(-1)
            p64, pld = f * p64, f.astype(np.longdouble) * pld
        order = np.argsort(keys, kind="stable")
        sk = keys[order]
        starts = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]])) if sk.size else np.zeros(0, np.int64)
        self.keys = sk[starts]
        self.S = _segment_sum(pld, order, starts)
        self.A = _segment_sum(np.abs(pld), order, starts)
        self.n = np.diff(np.concatenate([starts, [sk.size]])).astype(np.int64)
        self.P = np.zeros(self.keys.size)
        np.add.at(self.P, np.searchsorted(self.keys, keys), p64)

    def dense(self):
        """(S, A, n) as arrays of the matrix's shape."""
        size = int(np.prod(self.shape))
        S, A, n = np.zeros(size, np.longdouble), np.zeros(size, np.longdouble), np.zeros(size, np.int64)
        S[self.keys], A[self.keys], n[self.keys] = self.S, self.A, self.n
        return S.reshape(self.shape), A.reshape(self.shape), n.reshape(self.shape)


def reference_sums(o, pairs, pose_rot_t, weight):
    """o: FoptOracle with the clouds set (and posed); pairs: [(i, j, int32 [m, 2])] as given to set_pairs / SetCorrespondences.
    Returns {"rigid": {JJ, Jb, score}, "slac": {JJ, Jb, score}, "nonrigid": {AA}} of Sums."""
    num, nper = o.num, o.nper
    N0, N1, M = 6 * num, 6 * num + nper, num * nper
    rv, rb, ri, sv, sb, si, a1, v1, a2, v2 = ([] for _ in range(10))
    for i, j, pr in pairs:
        for ii, jj in np.asarray(pr, np.int64).reshape(-1, 2):
            val, b = o.rigid_bucket(i, int(ii), j, int(jj))
            rv.append(val); rb.append(b); ri.append(np.concatenate([i * 6 + np.arange(6), j * 6 + np.arange(6)]))
            idx, val, b = o.slac_bucket(i, int(ii), j, int(jj), pose_rot_t)
            sv.append(val); sb.append(b); si.append(idx.astype(np.int64))
            i1, w1, i2, w2 = o.nonrigid_bucket(i, int(ii), j, int(jj), weight)
            a1.append(i * nper + i1.astype(np.int64)); v1.append(w1); a2.append(j * nper + i2.astype(np.int64)); v2.append(w2)
    T = len(rb)
    arr = lambda x, w, dt: np.asarray(x, dt).reshape(T, w)
    rv, ri, rb = arr(rv, 12, np.float64), arr(ri, 12, np.int64), np.asarray(rb, np.float64).reshape(T)
    sv, si, sb = arr(sv, 60, np.float64), arr(si, 60, np.int64), np.asarray(sb, np.float64).reshape(T)
    a1, v1, a2, v2 = arr(a1, 24, np.int64), arr(v1, 24, np.float64), arr(a2, 24, np.int64), arr(v2, 24, np.float64)
    full = lambda x, y: (np.broadcast_to(x[:, :, None], (T, x.shape[1], y.shape[1])), np.broadcast_to(y[:, None, :], (T, x.shape[1], y.shape[1])))
    out = {}
    # rigid: AddHessian puts val[a] val[c] on BOTH triangles; every listed pair (an empty one too) adds 1 to the first six diagonal entries
    ra, rc = full(ri, ri)
    va, vc = full(rv, rv)
    gauge = np.tile(np.arange(6) * (N0 + 1), len(pairs))
    out["rigid"] = dict(
        JJ=Sums((N0, N0), np.concatenate([(ra * N0 + rc).reshape(-1), gauge]), np.concatenate([va.reshape(-1), np.ones(gauge.size)]),
                np.concatenate([vc.reshape(-1), np.ones(gauge.size)])),
        Jb=Sums((N0,), ri, rv, np.broadcast_to(rb[:, None], rv.shape)),
        score=Sums((1,), np.zeros(T, np.int64), rb, rb))
    # SLAC: upper triangle; a == c on the diagonal, coinciding indices fold 2 v_a v_c onto the diagonal, the rest goes to (min, max)
    ua, uc = np.triu_indices(60, 1)
    ia, ic = si[:, ua], si[:, uc]
    lo, hi = np.minimum(ia, ic), np.maximum(ia, ic)
    out["slac"] = dict(
        JJ=Sums((N1, N1), np.concatenate([(si * N1 + si).reshape(-1), (lo * N1 + hi).reshape(-1)]),
                np.concatenate([sv.reshape(-1), sv[:, ua].reshape(-1)]), np.concatenate([sv.reshape(-1), sv[:, uc].reshape(-1)]),
                np.concatenate([np.ones(sv.size), np.where(ia == ic, 2.0, 1.0).reshape(-1)])),
        Jb=Sums((N1,), si, sv, np.broadcast_to(sb[:, None], sv.shape)),
        score=Sums((1,), np.zeros(T, np.int64), sb, sb))
    # non-rigid: idx1 x idx1 and idx2 x idx2 on both triangles of the fragments' diagonal blocks, idx1 x idx2 on one side
    k, a, b = [], [], []
    for x, vx, y, vy in ((a1, v1, a1, v1), (a2, v2, a2, v2), (a1, v1, a2, v2)):
        r, c = full(x, y)
        p, q = full(vx, vy)
        k.append((r * M + c).reshape(-1)); a.append(p.reshape(-1)); b.append(q.reshape(-1))
    out["nonrigid"] = dict(AA=Sums((M, M), np.concatenate(k), np.concatenate(a), np.concatenate(b)))
    return out


def compare(sums, keys, vals, what, single_exact=True):
    """(keys, vals): the NON-ZERO entries of a computed system, flat indices into sums.shape, duplicates allowed (they are added in
    longdouble: the 24 x 24 blocks of the non-rigid mode overlap).  Asserts, entry by entry: no addend -> exactly 0.0; one addend ->
    the float64 product bit for bit; every entry |value - S| <= 2 n u A.  Returns the worst error / bound over the entries that are sums."""
    keys, vals = np.asarray(keys, np.int64).reshape(-1), np.asarray(vals, np.float64).reshape(-1)
    assert np.isfinite(vals).all(), what
    nz = vals != 0.0
    keys, vals = keys[nz], vals[nz]
    pos = np.searchsorted(sums.keys, keys)
    hit = (pos < sums.keys.size)
    hit[hit] = sums.keys[pos[hit]] == keys[hit]
    assert hit.all(), "%s: %d non-zero entries where the reference has no addend, first at flat index %d (value %r)" % (
        what, (~hit).sum(), keys[~hit][0], vals[~hit][0])
    got = np.zeros(sums.keys.size, np.longdouble)
    np.add.at(got, pos, vals.astype(np.longdouble))
    cnt = np.bincount(pos, minlength=sums.keys.size)
    bound = 2.0 * sums.n.astype(np.longdouble) * np.longdouble(U) * sums.A
    err = np.abs(got - sums.S)
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, "%s: %d entries outside 2 n u A; worst at flat index %d: got %r, sum %r, n = %d, error %.3g against %.3g" % (
        what, bad.size, sums.keys[bad[np.argmax((err - bound)[bad])]], float(got[bad[0]]), float(sums.S[bad[0]]), sums.n[bad[0]],
        float(err[bad].max()), float(bound[bad].max()))
    if single_exact:
        one = np.flatnonzero((sums.n == 1) & (cnt <= 1))
        g64 = got[one].astype(np.float64)
        same = (g64.view(np.uint64) == sums.P[one].view(np.uint64)) | ((g64 == 0.0) & (sums.P[one] == 0.0))
        assert same.all(), "%s: %d single-addend entries are not the float64 product; first at flat index %d: got %r, product %r" % (
            what, (~same).sum(), sums.keys[one[~same][0]], g64[~same][0], sums.P[one[~same][0]])
        assert ((sums.n != 1) | (cnt <= 1)).all(), what + ": a single-addend entry came from several non-zero parts"
    ok = (bound > 0) & ((sums.n > 1) | (not single_exact))        # (a single addend was just compared for equality: nothing to measure)
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


def compare_dense(sums, M, what, single_exact=True):
    M = np.ascontiguousarray(M, np.float64).reshape(-1)
    assert M.size == int(np.prod(sums.shape)), what
    k = np.flatnonzero(M)
    return compare(sums, k, M[k], what, single_exact)


def zero_pattern_matches(sums, keys, vals):
    """The computed non-zero set equals the reference's set of entries with A != 0."""
    keys, vals = np.asarray(keys, np.int64).reshape(-1), np.asarray(vals, np.float64).reshape(-1)
    return np.array_equal(np.unique(keys[vals != 0.0]), sums.keys[sums.A != 0])


# ---- the regularised systems -----------------------------------------------------------------------------------------------
def lattice_laplacian(res):
    """Every ORDERED pair (vertex, 6-neighbour) of the (res+1)^3 grid adds, per xyz component, +1 to both diagonal entries and -1 to
    the coupling (both triangles of the symmetric matrix).  Vertex (i, j, k) has index i + j (res+1) + k (res+1)^2, xyz interleaved."""
    n1 = res + 1
    L = np.zeros((3 * n1 ** 3, 3 * n1 ** 3))
    at = lambda i, j, k: i + j * n1 + k * n1 * n1
    for k in range(n1):
        for j in range(n1):
            for i in range(n1):
                for di, dj, dk in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)):
                    ii, jj, kk = i + di, j + dj, k + dk
                    if min(ii, jj, kk) < 0 or max(ii, jj, kk) > res:
                        continue
                    for c in range(3):
                        a, b = at(i, j, k) * 3 + c, at(ii, jj, kk) * 3 + c
                        L[a, a] += 1.0
                        L[b, b] += 1.0
                        L[a, b] -= 1.0
                        L[b, a] -= 1.0
    return L


def slac_system(JJ, num, res, default_weight):
    """thisJJ of OptimizeSLAC as a full symmetric float64 matrix: the data term JJ (Sums, upper triangle) + default_weight * (lattice
    Laplacian + 1 on the three entries of the anchor vertex (res/2, res/2, 0)) + 1 on the first six diagonal entries."""
    D = JJ.dense()[0].astype(np.float64)
    assert np.count_nonzero(np.tril(D, -1)) == 0
    A = D + np.triu(D, 1).T
    L = lattice_laplacian(res)
    anchor = (res // 2 + (res // 2) * (res + 1)) * 3
    for c in range(3):
        L[anchor + c, anchor + c] += 1.0
    A[6 * num:, 6 * num:] += default_weight * L
    A[np.arange(6), np.arange(6)] += 1.0
    return A


def nonrigid_system(AA, num, res):
    """thisAA of OptimizeNonrigid: the data term AA (Sums; lists with i < j, so the couplings sit above the diagonal blocks) + the
    Laplacian of scale 1 on every fragment block + 1 on the first three diagonal entries."""
    D = AA.dense()[0].astype(np.float64)
    nper = 3 * (res + 1) ** 3
    A = np.zeros_like(D)
    L = lattice_laplacian(res)
    for f in range(num):
        s = slice(f * nper, (f + 1) * nper)
        A[s, s] = D[s, s] + L
        assert np.count_nonzero(D[s, :f * nper]) == 0, "a list with i > j: its couplings lie below the diagonal blocks"
        A[s, (f + 1) * nper:] = D[s, (f + 1) * nper:]
        A[(f + 1) * nper:, s] = D[s, (f + 1) * nper:].T
    A[np.arange(3), np.arange(3)] += 1.0
    return A


def scaled_residual(A, x, b):
    """eta(x) = |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf), evaluated in longdouble."""
    Al, xl, bl = A.astype(np.longdouble), np.asarray(x).astype(np.longdouble), np.asarray(b).astype(np.longdouble)
    r = bl - Al @ xl
    return float(np.abs(r).max() / (np.abs(Al).sum(1).max() * np.abs(xl).max() + np.abs(bl).max()))
