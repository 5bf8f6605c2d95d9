"""A numpy statement of the pose graph model of DESIGN.md 7.12 (GraphOptimizer's switchable-constraint and EM modes): what
csrc/er_pgo_math.h and csrc/er_pgo.hip are pinned to.  It restates the reference's MODEL (GraphOptimizer/OptApp.cpp over g2o's VertexSE3 /
EdgeSE3 and vertigo's switchable edge); it is not g2o, and the Levenberg-Marquardt schedule below is this project's own.

    pose       4 x 4 isometry; X_0 fixed; initial poses X_{i+1} = X_i odo_i
    minimal    (t, qx, qy, qz), qw = sqrt(1 - |q|^2) >= 0;  X <- X fromMQT(delta);  r = toMQT(Z^-1 X_i^-1 X_j)
    costs      odometry r^T Om r;  loop (s r)^T Om (s r) + w (1 - s)^2;  s <- clamp(s + ds, 0, 1)
    switches   eliminated inside the edge (an exact 1 x 1 Schur complement): the system that is factored is 6 (N - 1) square
    LM         lambda_0 = 1e-5 max diag(H) (H linearised with lambda = 0 in the switches' H_ss); a trial solves (H + lambda I) d = -b, applies it
               and re-evaluates F; rho = (F - F_new) / (d^T (lambda d - b)) over poses and switches; rho > 0 and F_new finite: accept,
               lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)), nu = 2; otherwise lambda *= nu, nu *= 2; a failed factorisation is a
               rejected trial; an iteration is up to 10 trials; the run ends after max_iteration iterations or after an iteration without an
               accepted trial.
    EM         per round: l_k = w^2 / (w^2 + r^T Om r), the edge uses sqrt(l_k) Om, then one LM iteration with a fresh lambda_0.
"""
import numpy as np

TRIALS = 10


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def inverse(X):
    Y = np.eye(4)
    Y[:3, :3] = X[:3, :3].T
    Y[:3, 3] = -(X[:3, :3].T @ X[:3, 3])
    return Y


def product(A, B):
    C = np.eye(4)
    C[:3, :3] = A[:3, :3] @ B[:3, :3]
    C[:3, 3] = A[:3, :3] @ B[:3, 3] + A[:3, 3]
    return C


def quaternion(E):
    """(x, y, z, w), w >= 0, unit: the branch with the largest divisor."""
    m = E
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0.0:
        s = np.sqrt(tr + 1.0) * 2.0
        q = [(m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, 0.25 * s]
    elif m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        s = np.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2]) * 2.0
        q = [0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s, (m[2, 1] - m[1, 2]) / s]
    elif m[1, 1] > m[2, 2]:
        s = np.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2]) * 2.0
        q = [(m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s, (m[0, 2] - m[2, 0]) / s]
    else:
        s = np.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1]) * 2.0
        q = [(m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s, (m[1, 0] - m[0, 1]) / s]
    q = np.array(q)
    q = q / np.linalg.norm(q)
    return -q if q[3] < 0.0 else q


def to_mqt(E):
    q = quaternion(E)
    return np.concatenate([E[:3, 3], q[:3]]), q[3]


def from_mqt(d):
    x, y, z = d[3:6]
    n2 = x * x + y * y + z * z
    if n2 < 1.0:
        w = np.sqrt(1.0 - n2)
    else:
        n = np.sqrt(n2)
        x, y, z, w = x / n, y / n, z / n, 0.0
    D = np.eye(4)
    D[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    D[:3, 3] = d[:3]
    return D


def residual(Z, Xi, Xj):
    return to_mqt(product(inverse(Z), product(inverse(Xi), Xj)))[0]


def jacobians(Z, Xi, Xj):
    """(r, Ji, Jj): the closed forms of DESIGN.md 7.12."""
    A, B = inverse(Z), product(inverse(Xi), Xj)
    E = product(A, B)
    r, wE = to_mqt(E)
    qa, qb = quaternion(A), quaternion(B)
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    Jj[:3, :3] = E[:3, :3]
    Jj[3:, 3:] = wE * np.eye(3) + skew(r[3:])
    Ji[:3, :3] = -A[:3, :3]
    Ji[:3, 3:] = A[:3, :3] @ (2.0 * skew(B[:3, 3]))
    va, wa, vb, wb = qa[:3], qa[3], qb[:3], qb[3]
    p = np.concatenate([wa * vb + wb * va + np.cross(va, vb), [wa * wb - va @ vb]])          # q_A q_B
    sg = 1.0 if p @ np.concatenate([r[3:], [wE]]) >= 0.0 else -1.0
    Ji[3:, 3:] = -sg * ((wa * np.eye(3) + skew(va)) @ (wb * np.eye(3) - skew(vb)) - np.outer(va, vb))
    return r, Ji, Jj


def numeric_jacobians(Z, Xi, Xj, h=1e-7):
    """central differences of residual() along X <- X fromMQT(delta)"""
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        Ji[:, k] = (residual(Z, product(Xi, from_mqt(d)), Xj) - residual(Z, product(Xi, from_mqt(-d)), Xj)) / (2 * h)
        Jj[:, k] = (residual(Z, Xi, product(Xj, from_mqt(d))) - residual(Z, Xi, product(Xj, from_mqt(-d)))) / (2 * h)
    return Ji, Jj


def edge_record(Om, r, Ji, Jj, switchable, s, w, lam):
    """dict(H 12 x 12, g 12, hps 12, hss, bs, chi2): the edge's contribution with its switch eliminated; Hfull, gfull: before the elimination."""
    J = np.hstack([Ji, Jj]) * (s if switchable else 1.0)
    chi2 = r @ Om @ r
    if not switchable:
        return dict(H=J.T @ Om @ J, g=J.T @ Om @ r, hps=np.zeros(12), hss=1.0, bs=0.0, chi2=chi2, Hfull=J.T @ Om @ J, gfull=J.T @ Om @ r)
    hss = chi2 + w + lam
    bs = s * chi2 - w * (1.0 - s)
    hps = J.T @ Om @ r
    Hf, gf = J.T @ Om @ J, s * hps
    return dict(H=Hf - np.outer(hps, hps) / hss, g=gf - hps * bs / hss, hps=hps, hss=hss, bs=bs, chi2=chi2, Hfull=Hf, gfull=gf)


class Graph:
    """poses [N, 4, 4]; odometry edge i = (i, i + 1); loops: ids [K, 2], T [K, 4, 4]; information [.., 6, 6] or None (identity)."""

    def __init__(self, odo_T, loop_ids, loop_T, odo_info=None, loop_info=None):
        self.odo_T = np.asarray(odo_T, np.float64).reshape(-1, 4, 4)
        self.n_odo = len(self.odo_T)
        self.N = self.n_odo + 1
        self.loop_ids = np.asarray(loop_ids, np.int64).reshape(-1, 2)
        self.K = len(self.loop_ids)
        self.loop_T = np.asarray(loop_T, np.float64).reshape(-1, 4, 4)
        eye = np.eye(6)
        oi = np.tile(eye, (self.n_odo, 1, 1)) if odo_info is None else np.asarray(odo_info, np.float64).reshape(-1, 6, 6)
        li = np.tile(eye, (self.K, 1, 1)) if loop_info is None else np.asarray(loop_info, np.float64).reshape(-1, 6, 6)
        self.Z = np.concatenate([self.odo_T, self.loop_T]) if self.K else self.odo_T.copy()
        self.Om = np.concatenate([oi, li]) if self.K else oi.copy()
        self.ids = np.concatenate([np.stack([np.arange(self.n_odo), np.arange(self.n_odo) + 1], axis=1), self.loop_ids])
        self.E = self.n_odo + self.K
        self.n = 6 * self.n_odo
        self.reset()

    def reset(self):
        P = [np.eye(4)]
        for T in self.odo_T:
            P.append(P[-1] @ T)
        self.poses = np.stack(P)
        self.sw = np.ones(self.K)
        self.scale = np.ones(self.E)

    # ---- one linearisation ------------------------------------------------------------------------------------------------------------
    def records(self, switchable, w, lam):
        out = []
        for e in range(self.E):
            i, j = self.ids[e]
            r, Ji, Jj = jacobians(self.Z[e], self.poses[i], self.poses[j])
            is_sw = switchable and e >= self.n_odo
            out.append(edge_record(self.scale[e] * self.Om[e], r, Ji, Jj, is_sw, self.sw[e - self.n_odo] if is_sw else 1.0, w, lam))
        return out

    def assemble(self, recs, key_H="H", key_g="g"):
        """dense H, b of the pose unknowns (vertex v >= 1 at 6 (v - 1)) from per-edge 12 x 12 / 12 entries"""
        H, b = np.zeros((self.n, self.n)), np.zeros(self.n)
        for e, R in enumerate(recs):
            v = [self.ids[e][0] - 1, self.ids[e][1] - 1]
            for p in range(2):
                if v[p] < 0:
                    continue
                b[6 * v[p]:6 * v[p] + 6] += R[key_g][6 * p:6 * p + 6]
                for q in range(2):
                    if v[q] >= 0:
                        H[6 * v[p]:6 * v[p] + 6, 6 * v[q]:6 * v[q] + 6] += R[key_H][6 * p:6 * p + 6, 6 * q:6 * q + 6]
        return H, b

    def linearize(self, w, lam, switchable=True):
        """(H, b, chi2 per edge, the edge records)"""
        recs = self.records(switchable, w, lam)
        return self.assemble(recs) + (np.array([R["chi2"] for R in recs]), recs)

    def full_system(self, w):
        """the undamped (6 (N - 1) + K)-dimensional Gauss-Newton system of the switchable mode, switches last"""
        recs = self.records(True, w, 0.0)
        Hp, bp = self.assemble(recs, "Hfull", "gfull")
        n, K = self.n, self.K
        H, b = np.zeros((n + K, n + K)), np.zeros(n + K)
        H[:n, :n], b[:n] = Hp, bp
        for k in range(K):
            R = recs[self.n_odo + k]
            H[n + k, n + k] = R["hss"]
            b[n + k] = R["bs"]
            for p in range(2):
                v = self.ids[self.n_odo + k][p] - 1
                if v >= 0:
                    H[6 * v:6 * v + 6, n + k] += R["hps"][6 * p:6 * p + 6]
                    H[n + k, 6 * v:6 * v + 6] += R["hps"][6 * p:6 * p + 6]
        return H, b

    def cost(self, poses, sw, switchable, w):
        F = 0.0
        for e in range(self.E):
            i, j = self.ids[e]
            r = residual(self.Z[e], poses[i], poses[j])
            chi2 = r @ (self.scale[e] * self.Om[e]) @ r
            if switchable and e >= self.n_odo:
                s = sw[e - self.n_odo]
                F += s * s * chi2 + w * (1.0 - s) ** 2
            else:
                F += chi2
        return F

    # ---- one trial: (dx, ds, poses_c, sw_c, F_new, denom, ok) ---------------------------------------------------------------------------
    def trial(self, w, lam, switchable=True, lin=None):
        """lin: a linearize() result to use instead of a new one (without switches it does not depend on lambda)"""
        H, b, _, recs = lin if lin is not None else self.linearize(w, lam, switchable)
        try:
            with np.errstate(all="ignore"):
                if not np.isfinite(H).all():
                    raise np.linalg.LinAlgError
                L = np.linalg.cholesky(H + lam * np.eye(self.n))
            dx = np.linalg.solve(L.T, np.linalg.solve(L, -b))
        except np.linalg.LinAlgError:
            return None
        poses = self.poses.copy()
        for v in range(1, self.N):
            poses[v] = product(self.poses[v], from_mqt(dx[6 * (v - 1):6 * v]))
        ds, sw = np.zeros(self.K), self.sw.copy()
        denom = dx @ (lam * dx - b)
        if switchable:
            for k in range(self.K):
                R = recs[self.n_odo + k]
                d12 = np.concatenate([dx[6 * (v - 1):6 * v] if v > 0 else np.zeros(6) for v in self.ids[self.n_odo + k]])
                hd = R["hps"] @ d12
                ds[k] = (-R["bs"] - hd) / R["hss"]
                # the edge's part of delta^T (lambda delta - b) over poses and switches: b_pose = b_reduced + sum hps bs / hss
                denom += lam * ds[k] ** 2 - R["bs"] * ds[k] - hd * R["bs"] / R["hss"]
            sw = np.clip(self.sw + ds, 0.0, 1.0)
        with np.errstate(all="ignore"):
            F_new = self.cost(poses, sw, switchable, w)
        return dx, ds, poses, sw, F_new, denom

    def lm_iteration(self, w, switchable, st, trace, lin=None):
        """up to TRIALS trials; st = dict(lam, nu, F).  True if one was accepted."""
        if not switchable and lin is None:
            lin = self.linearize(w, 0.0, False)                            # the same for every trial of the iteration: nothing in it has a lambda
        for _ in range(TRIALS):
            t = self.trial(w, st["lam"], switchable, lin)
            F_new = np.nan if t is None else t[4]
            with np.errstate(all="ignore"):
                rho = np.nan if t is None else (st["F"] - F_new) / t[5]
            ok = t is not None and np.isfinite(F_new) and rho > 0.0
            trace.append((st["lam"], st["F"], F_new, bool(ok)))
            if ok:
                self.poses, self.sw = t[2], t[3]
                st["lam"] *= max(1.0 / 3.0, min(1.0 - (2.0 * rho - 1.0) ** 3, 2.0 / 3.0))
                st["nu"] = 2.0
                st["F"] = F_new
                return True
            st["lam"] *= st["nu"]
            st["nu"] *= 2.0
        return False

    def lambda0(self, w, switchable):
        H = self.linearize(w, 0.0, switchable)[0]
        return 1e-5 * max(0.0, np.max(np.diag(H)))

    def optimize(self, method="switchable", w=1.0, max_iteration=100):
        """dict(poses, values (switches or EM weights), kept, iterations, trials, trace [(lambda, F, F_new, accepted)])"""
        self.reset()
        trace, its = [], 0
        lk = np.zeros(self.K)
        if method == "switchable":
            if max_iteration > 0:
                st = dict(lam=self.lambda0(w, True), nu=2.0, F=self.cost(self.poses, self.sw, True, w))
            for _ in range(max_iteration):
                its += 1
                if not self.lm_iteration(w, True, st, trace):
                    break
            values, kept = self.sw.copy(), self.sw > 0.5
        else:
            for _ in range(max_iteration):
                for k in range(self.K):
                    e = self.n_odo + k
                    r = residual(self.Z[e], self.poses[self.ids[e][0]], self.poses[self.ids[e][1]])
                    lk[k] = (w * w) / (w * w + r @ self.Om[e] @ r)
                    self.scale[e] = np.sqrt(lk[k])
                lin = self.linearize(w, 0.0, False)
                st = dict(lam=1e-5 * max(0.0, np.max(np.diag(lin[0]))), nu=2.0, F=self.cost(self.poses, self.sw, False, w))
                its += 1
                self.lm_iteration(w, False, st, trace, lin)
            values, kept = lk.copy(), lk > 0.25
        return dict(poses=self.poses.copy(), values=values, kept=kept, iterations=its, trials=len(trace), trace=trace)
