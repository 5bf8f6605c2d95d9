"""The numpy statement of the depth odometry (csrc/er_odom_math.h and csrc/er_odom.hip restate it): KinFu-style
projective point-to-plane ICP between depth frames.  The reference tree does not contain KinFu; this file is the pin, and nothing here is
PCL's text or is checked against PCL.

Everything per pixel is float32, elementwise, in the operation order of er_odom_math.h (numpy never fuses a multiply with an add; its '/'
and sqrt are correctly rounded).  The sums are float64 sums of exact products; the 6 x 6 solve is numpy.linalg.cholesky."""
import math

import numpy as np

F = np.float32
SIGMA_SPACE, SIGMA_DEPTH = 4.5, 30.0
RADIUS = 6                    # 13 x 13
PYR_SPAN = 90                 # 3 sigma_depth, millimetres
DEPTH_W_MAX = 512
DEFAULTS = dict(levels=3, iterations=(10, 5, 4, 4), bilateral=1, max_depth_mm=0, min_valid=50, dist_thresh=F(0.10),
                angle_thresh=F(0.3420201433256687))
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]     # the upper triangle of J^T J, row by row


def tables():
    """(space[73], depth_w[n]): float64 exp rounded to float32.  The depth table ends where its weight times the smallest space weight would
    no longer be a normal float32."""
    space = np.exp(-np.arange(73, dtype=np.float64) / (2.0 * SIGMA_SPACE * SIGMA_SPACE)).astype(F)
    d = np.arange(DEPTH_W_MAX, dtype=np.float64)
    w = np.exp(-d * d / (2.0 * SIGMA_DEPTH * SIGMA_DEPTH)).astype(F)
    under = w.astype(np.float64) * np.float64(space[72]) < np.float64(np.finfo(F).tiny)
    n = int(np.argmax(under)) if under.any() else DEPTH_W_MAX
    return space, w[:n].copy()


def bilateral(img, space, depth_w):
    """uint16 [rows, cols] -> uint16: 169 shifted-array passes in row-major tap order; taps outside the image or with depth 0 are skipped
    (a weight of +0 added to a non-negative sum is the same bits)."""
    rows, cols = img.shape
    c = img.astype(np.int32)
    n = len(depth_w)
    dw = np.zeros(65536, F)
    dw[:n] = depth_w
    pad = np.zeros((rows + 2 * RADIUS, cols + 2 * RADIUS), np.int32)
    pad[RADIUS:RADIUS + rows, RADIUS:RADIUS + cols] = c
    wsum = np.zeros((rows, cols), F)
    s = np.zeros((rows, cols), F)
    for dy in range(-RADIUS, RADIUS + 1):
        for dx in range(-RADIUS, RADIUS + 1):
            tap = pad[RADIUS + dy:RADIUS + dy + rows, RADIUS + dx:RADIUS + dx + cols]
            delta = np.abs(tap - c)
            valid = (tap != 0) & (c != 0) & (delta < n)
            w = np.where(valid, space[dx * dx + dy * dy] * dw[delta], F(0))
            wsum = wsum + w
            s = s + w * tap.astype(F)
    with np.errstate(all="ignore"):
        out = np.rint(s / wsum)
    return np.where(c != 0, out, F(0)).astype(np.uint16)


def pyr_down(src):
    """Level l -> l + 1: the integer mean of the taps of the 5 x 5 window around (2x, 2y) inside the image and within PYR_SPAN of the centre."""
    rows, cols = src.shape
    s32 = src.astype(np.int64)
    c = s32[0::2, 0::2]
    pad = np.full((rows + 4, cols + 4), -10 ** 9, np.int64)
    pad[2:2 + rows, 2:2 + cols] = s32
    total = np.zeros_like(c)
    count = np.zeros_like(c)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            tap = pad[2 + dy:2 + dy + rows:2, 2 + dx:2 + dx + cols:2]
            ok = np.abs(tap - c) < PYR_SPAN
            total += np.where(ok, tap, 0)
            count += ok
    return np.where(c != 0, total // np.maximum(count, 1), 0).astype(np.uint16)


def vertex_map(depth, K):
    fx, fy, cx, cy = (F(k) for k in K)
    rows, cols = depth.shape
    u = np.arange(cols, dtype=F)[None, :]
    v = np.arange(rows, dtype=F)[:, None]
    z = depth.astype(F) / F(1000.0)
    V = np.empty((rows, cols, 3), F)
    V[..., 0] = (z * (u - cx)) / fx
    V[..., 1] = (z * (v - cy)) / fy
    V[..., 2] = z
    V[depth == 0] = np.nan
    return V


def normals_of(V):
    """normalize(cross(v(x+1, y) - v, v(x, y+1) - v)) of a vertex map; NaN where one of the three vertices is not valid (NaN) and on the
    last row and the last column."""
    rows, cols = V.shape[:2]
    N = np.full((rows, cols, 3), np.nan, F)
    p = V[:-1, :-1]
    a = V[:-1, 1:] - p
    b = V[1:, :-1] - p
    with np.errstate(all="ignore"):
        cx = a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
        cy = a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
        cz = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
        ln = np.sqrt((cx * cx + cy * cy) + cz * cz)
        n = np.stack([cx / ln, cy / ln, cz / ln], -1)
    ok = ~(np.isnan(p).any(-1) | np.isnan(V[:-1, 1:]).any(-1) | np.isnan(V[1:, :-1]).any(-1))
    n[~ok] = np.nan
    N[:-1, :-1] = n
    return N


def normal_map(depth, K):
    return normals_of(vertex_map(depth, K))


def rotation(alpha, beta, gamma):
    """Rz(gamma) Ry(beta) Rx(alpha)."""
    sa, ca, sb, cb, sg, cg = math.sin(alpha), math.cos(alpha), math.sin(beta), math.cos(beta), math.sin(gamma), math.cos(gamma)
    return np.array([[cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca],
                     [sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca],
                     [-sb, cb * sa, cb * ca]], np.float64)


class Odometry:
    def __init__(self, cols, rows, cam, tables_=None, **params):
        self.cols, self.rows, self.cam = cols, rows, tuple(F(k) for k in cam)
        p = dict(DEFAULTS)
        p.update(params)
        self.p = p
        self.levels = int(p["levels"])
        assert 1 <= self.levels <= 4 and cols % (1 << (self.levels - 1)) == 0 and rows % (1 << (self.levels - 1)) == 0
        self.space, self.depth_w = tables_ if tables_ is not None else tables()
        self.total_iters = sum(int(p["iterations"][l]) for l in range(self.levels))

    def K(self, level):
        return tuple(k / F(1 << level) for k in self.cam)

    def depth_pyramid(self, frame):
        img = np.asarray(frame, np.uint16).reshape(self.rows, self.cols)
        d0 = bilateral(img, self.space, self.depth_w) if self.p["bilateral"] else img.copy()
        if self.p["max_depth_mm"] > 0:
            d0 = np.where(d0 > self.p["max_depth_mm"], 0, d0).astype(np.uint16)
        out = [d0]
        for _ in range(1, self.levels):
            out.append(pyr_down(out[-1]))
        return out

    def maps(self, frame):
        """Per level (depth uint16 [r, c], vertex float32 [r, c, 3], normal float32 [r, c, 3])."""
        return [(d, vertex_map(d, self.K(l)), normal_map(d, self.K(l))) for l, d in enumerate(self.depth_pyramid(frame))]

    def rows_of(self, model, cur, level, T, mask=False):
        """The rows (a [m, 6] float32, b [m] float32) of the pixels of `cur` that find a match in `model` under m_T_c = T (float64 4x4);
        mask: also which pixels those are."""
        _, Vm, Nm = model[level]
        _, Vc, Nc = cur[level]
        rows, cols = Vm.shape[:2]
        fx, fy, cx, cy = self.K(level)
        T = np.asarray(T, np.float64).reshape(4, 4)
        R, t = T[:3, :3].astype(F), T[:3, 3].astype(F)           # the float64 state cast to float32 once
        v, n = Vc.reshape(-1, 3), Nc.reshape(-1, 3)
        vx, vy, vz, nx, ny, nz = v[:, 0], v[:, 1], v[:, 2], n[:, 0], n[:, 1], n[:, 2]
        with np.errstate(all="ignore"):
            ok = np.isfinite(v).all(1) & np.isfinite(n).all(1)
            gx = ((R[0, 0] * vx + R[0, 1] * vy) + R[0, 2] * vz) + t[0]
            gy = ((R[1, 0] * vx + R[1, 1] * vy) + R[1, 2] * vz) + t[1]
            gz = ((R[2, 0] * vx + R[2, 1] * vy) + R[2, 2] * vz) + t[2]
            hx = (R[0, 0] * nx + R[0, 1] * ny) + R[0, 2] * nz
            hy = (R[1, 0] * nx + R[1, 1] * ny) + R[1, 2] * nz
            hz = (R[2, 0] * nx + R[2, 1] * ny) + R[2, 2] * nz
            ok &= np.isfinite(gx) & np.isfinite(gy) & np.isfinite(gz) & (gz > 0)
            pu = np.rint((gx * fx) / gz + cx)
            pv = np.rint((gy * fy) / gz + cy)
            ok &= (pu >= 0) & (pu <= F(cols - 1)) & (pv >= 0) & (pv <= F(rows - 1))          # tested in float, before any conversion
            idx = np.where(ok, pv, F(0)).astype(np.int64) * cols + np.where(ok, pu, F(0)).astype(np.int64)
            vm, nm = Vm.reshape(-1, 3)[idx], Nm.reshape(-1, 3)[idx]
            ok &= np.isfinite(vm).all(1) & np.isfinite(nm).all(1)
            mx, my, mz = nm[:, 0], nm[:, 1], nm[:, 2]
            dx, dy, dz = vm[:, 0] - gx, vm[:, 1] - gy, vm[:, 2] - gz
            dist = np.sqrt((dx * dx + dy * dy) + dz * dz)
            ok &= dist <= F(self.p["dist_thresh"])
            sx, sy, sz = hy * mz - hz * my, hz * mx - hx * mz, hx * my - hy * mx
            sine = np.sqrt((sx * sx + sy * sy) + sz * sz)
            ok &= sine < F(self.p["angle_thresh"])
            a = np.stack([gy * mz - gz * my, gz * mx - gx * mz, gx * my - gy * mx, mx, my, mz], 1)
            b = (mx * dx + my * dy) + mz * dz
        return (a[ok], b[ok], ok) if mask else (a[ok], b[ok])

    def linearize(self, model, cur, level, T, with_abs=False):
        """(sums[27], count): 21 entries of the upper triangle of J^T J row by row, then J^T r; every product of two float32 values is taken
        in float64 (exact).  with_abs: also the sums of the absolute terms (what bounds the difference of two summation orders)."""
        a, b = self.rows_of(model, cur, level, T)
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        terms = [a64[:, i] * a64[:, j] for i, j in PAIRS] + [a64[:, i] * b64 for i in range(6)]
        sums = np.array([np.sum(x) for x in terms], np.float64)
        if with_abs:
            return sums, len(b), np.array([np.sum(np.abs(x)) for x in terms], np.float64)
        return sums, len(b)

    def step(self, sums, count, T):
        """One pose update from an iteration's sums.  Returns (T_new, lost); a lost pair keeps T."""
        T = np.asarray(T, np.float64).reshape(4, 4)
        if count < self.p["min_valid"] or not np.isfinite(sums).all():
            return T.copy(), True
        A = np.zeros((6, 6))
        for k, (i, j) in enumerate(PAIRS):
            A[i, j] = A[j, i] = sums[k]
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            return T.copy(), True
        x = np.linalg.solve(L.T, np.linalg.solve(L, sums[21:27]))
        if not np.isfinite(x).all():
            return T.copy(), True
        Rinc = rotation(x[0], x[1], x[2])
        out = np.eye(4)
        out[:3, :3] = Rinc @ T[:3, :3]
        out[:3, 3] = Rinc @ T[:3, 3] + x[3:6]
        if not np.isfinite(out).all():
            return T.copy(), True
        return out, False

    def schedule(self):
        """The (level) of every iteration, coarse to fine."""
        return [l for l in range(self.levels - 1, -1, -1) for _ in range(int(self.p["iterations"][l]))]

    def align_maps(self, model, cur, guess=None):
        """(T, lost, trace): trace[k] = (pose after iteration k, that iteration's count)."""
        T = np.eye(4) if guess is None else np.asarray(guess, np.float64).reshape(4, 4).copy()
        lost, trace = False, []
        for level in self.schedule():
            count = 0
            if not lost:
                sums, count = self.linearize(model, cur, level, T)
                T, lost = self.step(sums, count, T)
            trace.append((T.copy(), count))
        return T, lost, trace

    def align(self, model_frame, cur_frame, guess=None):
        return self.align_maps(self.maps(model_frame), self.maps(cur_frame), guess)

    def track(self, frames):
        """T_rel[i] = frame i <- frame i + 1, and the lost flags."""
        m = [self.maps(f) for f in frames]
        out = [self.align_maps(m[i], m[i + 1]) for i in range(len(m) - 1)]
        return np.stack([o[0] for o in out]), np.array([o[1] for o in out])


def accumulate(T_rel, first=None):
    W = [np.eye(4) if first is None else np.asarray(first, np.float64)]
    for T in T_rel:
        W.append(W[-1] @ T)
    return np.stack(W)


def pose_error(T, G):
    """(rotation error in degrees, translation error in metres) of T against G."""
    D = np.linalg.inv(G) @ T
    c = min(1.0, max(-1.0, (np.trace(D[:3, :3]) - 1.0) / 2.0))
    return math.degrees(math.acos(c)), float(np.linalg.norm(D[:3, 3]))
