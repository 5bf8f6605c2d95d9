"""Plain numpy restatement of one iteration of path B's ICP loop (er_icp.hip: k_icp_iter, k_icp_final, dev_icp_decide), written from the
kernels' comments and the oracle's definition, not from their code paths:

  correspondences   brute-force float32 nearest neighbour, d = ((dx*dx) + dy*dy) + dz*dz with dx = q - t, ties to the lower index; kept iff
                    d <= float(max_dist)^2 as doubles and not d > max_dist^2;
  rows              a, b, c and e are float32 expressions evaluated left to right and widened; the 29 values of a correspondence are float64
                    products of those (0..20 upper triangle of A^T A row by row over [a b c nx ny nz], 21..26 A^T b, 27 d, 28 one); a
                    correspondence with a non-finite coordinate or normal has slots 27 and 28 only;
  sums              per slot the EXACT sum S of the float64 values (fractions.Fraction) and the sum A of their magnitudes;
  update            X <- M X in float32, ((m0 x + m1 y) + m2 z) + m3 per row;
  increment         Rz(gamma) Ry(beta) Rx(alpha) in float64, stored as float32; final = increment * final in float32, each entry
                    ((d0 f0 + d1 f1) + d2 f2) + d3 f3;
  stop rules        0: iteration limit, then the increment's angle and translation against eps, then |mse - previous mse| < 1e-12;
                    1: iteration limit, then |float32 sum of (increment - previous increment)| < eps.

The library is built without floating-point contraction, so every float32 expression here has the bits the kernel computes."""
from fractions import Fraction

import numpy as np

F = np.float32
U = 2.0 ** -53
IDENT = np.eye(4, dtype=F)


def nearest(Q, P, chunk=512):
    """(index of the nearest row of P, float32 squared distance) for every row of Q; ties to the lower index."""
    Q, P = np.asarray(Q, F).reshape(-1, 3), np.asarray(P, F).reshape(-1, 3)
    idx, dist = np.zeros(len(Q), np.int64), np.zeros(len(Q), F)
    for s in range(0, len(Q), chunk):
        q = Q[s:s + chunk]
        dx, dy, dz = (q[:, None, a] - P[None, :, a] for a in range(3))
        d = ((dx * dx) + dy * dy) + dz * dz
        assert d.dtype == F
        d = np.where(np.isnan(d), F(np.inf), d)
        i = np.argmin(d, axis=1)
        idx[s:s + chunk], dist[s:s + chunk] = i, d[np.arange(len(q)), i]
    return idx, dist


def kept(d, max_dist):
    """ICP's correspondence filter on float32 squared distances."""
    r = float(F(max_dist))
    d = d.astype(np.float64)
    return (d <= r * r) & ~(d > float(max_dist) * float(max_dist))


def row_values(X, tgt_xyz, tgt_nrm, max_dist, normal_products=np.float64):
    """The 29 float64 values of every kept correspondence of the points X (float32 [n, 3]), in the order of X: float64 [m, 29]; also the
    kept source rows and their target indices.  normal_products: the type in which the six products of two normal components (slots
    15..20) are formed -- float64 in the kernel, float32 in oracle/icp_oracle.cpp (nx * nx of two floats, widened afterwards)."""
    X = np.asarray(X, F).reshape(-1, 3)
    idx, d = nearest(X, tgt_xyz)
    k = np.nonzero(kept(d, max_dist))[0]
    i = idx[k]
    s, t, n = X[k], np.asarray(tgt_xyz, F)[i], np.asarray(tgt_nrm, F)[i]
    sx, sy, sz = s[:, 0], s[:, 1], s[:, 2]
    dx, dy, dz = t[:, 0], t[:, 1], t[:, 2]
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        a = nz * sy - ny * sz
        b = nx * sz - nz * sx
        c = ny * sx - nx * sy
        e = nx * dx + ny * dy + nz * dz - nx * sx - ny * sy - nz * sz
        assert a.dtype == F and e.dtype == F
        v = [q.astype(np.float64) for q in (a, b, c, nx, ny, nz)]
        e = e.astype(np.float64)
        W = np.zeros((len(k), 29), np.float64)
        t_ = 0
        for r in range(6):
            for q in range(r, 6):
                W[:, t_] = v[r] * v[q]
                t_ += 1
        if normal_products is not np.float64:
            t_ = 15
            for r in range(3, 6):
                for q in range(r, 6):
                    W[:, t_] = (n[:, r - 3] * n[:, q - 3]).astype(np.float64)
                    t_ += 1
        for r in range(6):
            W[:, 21 + r] = v[r] * e
    fin = np.isfinite(s).all(axis=1) & np.isfinite(n).all(axis=1)
    W[~fin, :27] = 0.0
    W[:, 27] = d[k].astype(np.float64)
    W[:, 28] = 1.0
    return W, k, i


def exact_column_sum(v):
    """The exact sum of finite float64 values as a Fraction (mantissas added as integers, exponent by exponent)."""
    v = np.asarray(v, np.float64)
    v = v[v != 0.0]
    if len(v) == 0:
        return Fraction(0)
    m, e = np.frexp(v)
    mi = np.ldexp(m, 53).astype(np.int64)                     # exact: |m| 2^53 is an integer below 2^53
    e = e.astype(np.int64) - 53
    total, emin = 0, int(e.min())
    for ex in np.unique(e):
        q = mi[e == ex]
        hi, lo = q >> 27, q & ((1 << 27) - 1)                 # two halves: neither sum can overflow 64 bits
        total += ((int(hi.sum()) << 27) + int(lo.sum())) << (int(ex) - emin)
    return Fraction(total) * Fraction(2) ** emin


def exact_sums(W):
    """Per slot (S exact as a Fraction, A = exact sum of magnitudes as a Fraction)."""
    return [exact_column_sum(W[:, t]) for t in range(W.shape[1])], [exact_column_sum(np.abs(W[:, t])) for t in range(W.shape[1])]


def apply_f32(M, X):
    """X <- M X in float32 (IterativeClosestPoint::transformCloud)."""
    M, X = np.asarray(M, F).reshape(4, 4), np.asarray(X, F).reshape(-1, 3)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    out = np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], axis=1)
    assert out.dtype == F
    return out


def is_identity(M):
    return bool((np.asarray(M, F).reshape(4, 4) == IDENT).all())


def start_points(src_xyz, guess):
    """The source as iteration 0 sees it: the guess applied in float32 unless it is the identity."""
    X = np.asarray(src_xyz, F).reshape(-1, 3)
    return X.copy() if is_identity(guess) else apply_f32(guess, X)


def increment_f64(x):
    """constructTransformationMatrix before its float32 storage: float64 4x4."""
    sa, ca, sb, cb, sg, cg = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    M = np.zeros((4, 4))
    M[0, :3] = [cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca]
    M[1, :3] = [sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca]
    M[2, :3] = [-sb, cb * sa, cb * ca]
    M[:3, 3] = x[3:6]
    M[3, 3] = 1.0
    return M


def construct_increment(x):
    return increment_f64(x).astype(F)


def compose(D, Fin):
    """final = increment * final in float32 with the kernel's association."""
    D, Fin = np.asarray(D, F).reshape(4, 4), np.asarray(Fin, F).reshape(4, 4)
    out = np.zeros((4, 4), F)
    for r in range(4):
        for c in range(4):
            out[r, c] = ((D[r, 0] * Fin[0, c] + D[r, 1] * Fin[1, c]) + D[r, 2] * Fin[2, c]) + D[r, 3] * Fin[3, c]
    return out


def system(tot):
    """(A^T A 6x6, A^T b) from the 29 totals."""
    A, t = np.zeros((6, 6)), 0
    for r in range(6):
        for c in range(r, 6):
            A[r, c] = A[c, r] = tot[t]
            t += 1
    return A, np.array(tot[21:27], np.float64)


def solve6(A, b):
    """Gaussian elimination with partial pivoting; None when a pivot is zero or not finite (what the library's fallback refuses; its
    LDL^T refuses earlier, on a pivot that is not safely positive, and then asks the fallback)."""
    A, b = np.array(A, np.float64), np.array(b, np.float64)
    for c in range(6):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if A[p, c] == 0.0 or not np.isfinite(A[p, c]):
            return None
        if p != c:
            A[[p, c]], b[[p, c]] = A[[c, p]], b[[c, p]]
        for r in range(c + 1, 6):
            f = A[r, c] / A[c, c]
            A[r, c:] -= f * A[c, c:]
            b[r] -= f * b[c]
    x = np.zeros(6)
    for r in range(5, -1, -1):
        x[r] = (b[r] - A[r, r + 1:] @ x[r + 1:]) / A[r, r]
    return x if np.isfinite(x).all() else None


class State:
    """The loop variables of IterativeClosestPoint::align."""

    def __init__(self, guess):
        self.fin = np.asarray(guess, F).reshape(4, 4).copy()
        self.delta, self.prev_delta = IDENT.copy(), IDENT.copy()
        self.prev_mse = np.finfo(np.float64).max
        self.iter, self.done, self.conv = 0, False, False


def stop_after(st, D, prev_D, tot, max_iter, eps, stop_rule):
    """The stop rules after an accepted increment D (st.iter already counts it).  Returns (stop, converged); updates st.prev_mse."""
    D = np.asarray(D, F).reshape(4, 4)
    if st.iter >= max_iter:
        return True, True
    if stop_rule == 0:
        cos_angle = 0.5 * float((D[0, 0] + D[1, 1]) + D[2, 2] - F(1))
        tr2 = float((D[0, 3] * D[0, 3] + D[1, 3] * D[1, 3]) + D[2, 3] * D[2, 3])
        cur = tot[27] / tot[28]
        stop = (cos_angle >= 1.0 - eps and tr2 <= eps) or abs(cur - st.prev_mse) < 1e-12
        st.prev_mse = cur
        return stop, stop
    s = F(0)
    for v, w in zip(D.reshape(16), np.asarray(prev_D, F).reshape(16)):
        s = s + (v - w)
    stop = abs(float(s)) < eps
    return stop, stop


def decide(st, tot, max_iter, eps, stop_rule):
    """One decision from the iteration's 29 totals: the minimum of 3 correspondences, the solve, the increment, the composition, the stop
    rule.  Returns the increment or None."""
    if tot[28] < 3.0:
        st.done, st.conv = True, False
        return None
    x = solve6(*system(tot))
    if x is None:
        st.done, st.conv = True, False
        return None
    D = construct_increment(x)
    st.prev_delta, st.delta = st.delta, D
    st.fin = compose(D, st.fin)
    st.iter += 1
    stop, conv = stop_after(st, D, st.prev_delta, tot, max_iter, eps, stop_rule)
    if stop:
        st.done, st.conv = True, conv
    return D


def align(src_xyz, tgt_xyz, tgt_nrm, guess, max_dist, max_iter=20, eps=1e-6, stop_rule=0, trace=None, normal_products=np.float64):
    """The whole loop on the restatement: (T float32 4x4, iterations, converged).  Sums are the exact sums rounded once."""
    st = State(guess)
    X = start_points(src_xyz, guess)
    if len(X) == 0 or len(tgt_xyz) == 0:
        return st.fin, 0, False
    while not st.done:
        W, _, _ = row_values(X, tgt_xyz, tgt_nrm, max_dist, normal_products)
        S, _ = exact_sums(W)
        tot = np.array([float(s) for s in S])
        D = decide(st, tot, max_iter, eps, stop_rule)
        if trace is not None:
            trace.append(dict(totals=tot, delta=None if D is None else D.copy(), fin=st.fin.copy(), iter=st.iter, done=st.done, conv=st.conv))
        if D is not None:
            X = apply_f32(D, X)
    return st.fin, st.iter, st.conv
