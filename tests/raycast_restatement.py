"""The ray caster (csrc/er_raycast_math.h) in numpy: the brute-force march, one numpy operation per rounded float32
operation, no empty-space skip.  The host-compiled header (tests/test_raycast_cpu.py) and the device (tests/test_raycast_gpu.py) are held
to this file bit for bit; that equality is also what proves the kernel's skip.

A volume is a dict {unit key: (sdf float32[64^3], weight float32[64^3])} as TSDFVolume.read_unit / OracleVolume.read_unit return it.
"""
import math

import numpy as np

F = np.float32
UL = 3.0 / 512.0
ULF = F(UL)
HALF = 256 * 64
LATTICE = 512 * 64
MAX_STEPS = 65536
BRACKETS = 4
DEFAULT_PARAMS = (F(0.0), F(4.0), F(0.8) * F(0.03))


class Refused(ValueError):
    pass


def count_steps(t_min, t_max, step):
    t_min, t_max, step = F(t_min), F(t_max), F(step)
    if not (np.isfinite(t_min) and np.isfinite(t_max) and np.isfinite(step)) or not step > 0:
        raise Refused("t_min, t_max and step must be finite and step positive")
    if t_max <= t_min:
        return 0
    n = math.ceil((float(t_max) - float(t_min)) / float(step))
    if n > MAX_STEPS:
        raise Refused("more than %d steps" % MAX_STEPS)
    return int(n)


class Volume:
    """The dict as arrays: fetch() answers (observed, sdf) for arrays of 0-based lattice indices."""

    def __init__(self, units):
        self.keys = np.array(sorted(units), np.int64)
        n = len(self.keys)
        self.sdf = np.zeros((max(n, 1), 64 ** 3), np.float32)
        self.w = np.zeros((max(n, 1), 64 ** 3), np.float32)
        for i, k in enumerate(self.keys):
            self.sdf[i] = np.asarray(units[int(k)][0], np.float32).reshape(-1)
            self.w[i] = np.asarray(units[int(k)][1], np.float32).reshape(-1)

    def fetch(self, gx, gy, gz):
        inl = (gx >= 0) & (gx < LATTICE) & (gy >= 0) & (gy < LATTICE) & (gz >= 0) & (gz < LATTICE)
        gx, gy, gz = np.where(inl, gx, 0), np.where(inl, gy, 0), np.where(inl, gz, 0)
        key = (gx >> 6) << 18 | (gy >> 6) << 9 | (gz >> 6)
        vox = (gx & 63) * 4096 + (gy & 63) * 64 + (gz & 63)
        if len(self.keys) == 0:
            return np.zeros(gx.shape, bool), np.zeros(gx.shape, np.float32)
        pos = np.minimum(np.searchsorted(self.keys, key), len(self.keys) - 1)
        have = inl & (self.keys[pos] == key)
        pos = np.where(have, pos, 0)
        return have & (self.w[pos, vox] != 0), self.sdf[pos, vox]


def nearest_index(p):
    """-> (on the lattice, index): rint((double)p / unit length), tested as a double before it becomes an integer."""
    with np.errstate(invalid="ignore"):
        q = np.rint(p.astype(np.float64) / UL)
        ok = (q >= -HALF) & (q <= HALF - 1)
    return ok, np.where(ok, q, 0).astype(np.int64) + HALF


def sample_nearest(vol, px, py, pz):
    ox, gx = nearest_index(px)
    oy, gy = nearest_index(py)
    oz, gz = nearest_index(pz)
    obs, Fv = vol.fetch(gx, gy, gz)
    return obs & ox & oy & oz, Fv


def cell_index(p):
    with np.errstate(invalid="ignore"):
        q = p.astype(np.float64) / UL
        fl = np.floor(q)
        ok = (fl >= -HALF) & (fl <= HALF - 1)
        f = (q - fl).astype(np.float32)
    return ok, np.where(ok, fl, 0).astype(np.int64) + HALF, f


def trilinear(vol, px, py, pz):
    """-> (valid, value): eight fetches, z innermost, c = F0 + f (F1 - F0), then y, then x; valid iff all eight corners are observed."""
    ox, ix, fx = cell_index(px)
    oy, iy, fy = cell_index(py)
    oz, iz, fz = cell_index(pz)
    ok = ox & oy & oz
    c = {}
    for a in (0, 1):
        for b in (0, 1):
            for d in (0, 1):
                o, c[a, b, d] = vol.fetch(ix + a, iy + b, iz + d)
                ok = ok & o
    with np.errstate(invalid="ignore", over="ignore"):
        c00 = c[0, 0, 0] + fz * (c[0, 0, 1] - c[0, 0, 0])
        c01 = c[0, 1, 0] + fz * (c[0, 1, 1] - c[0, 1, 0])
        c10 = c[1, 0, 0] + fz * (c[1, 0, 1] - c[1, 0, 0])
        c11 = c[1, 1, 0] + fz * (c[1, 1, 1] - c[1, 1, 0])
        c0 = c00 + fy * (c01 - c00)
        c1 = c10 + fy * (c11 - c10)
        return ok, c0 + fx * (c1 - c0)


def raycast(units, cols, rows, cam4, T, params=None, stats=None):
    """-> (depth uint16[rows, cols], vmap float32[rows, cols, 3], nmap float32[rows, cols, 3]); camera frame, NaN / 0 where there is no hit.
    stats (a dict): receives 'samples' = the samples the plain march takes, summed over the image, and 'hits'."""
    t_min, t_max, step = [F(x) for x in (DEFAULT_PARAMS if params is None else params)]
    n_steps = count_steps(t_min, t_max, step)
    vol = units if isinstance(units, Volume) else Volume(units)
    fx, fy, cx, cy = [F(x) for x in cam4]
    T = np.asarray(T, np.float64).reshape(4, 4)
    R = T[:3, :3].astype(np.float32)
    o = T[:3, 3].astype(np.float32)
    n = cols * rows
    err = lambda: np.errstate(invalid="ignore", over="ignore", divide="ignore")      # noqa: E731
    with err():
        u = np.tile(np.arange(cols, dtype=np.float32), rows)
        v = np.repeat(np.arange(rows, dtype=np.float32), cols)
        x = (u - cx) / fx
        y = (v - cy) / fy
        ln = np.sqrt((x * x + y * y) + F(1.0))
        dc = [x / ln, y / ln, F(1.0) / ln]
        dw = [(R[a, 0] * dc[0] + R[a, 1] * dc[1]) + R[a, 2] * dc[2] for a in range(3)]
    active = np.arange(n)
    prev_obs = np.zeros(n, bool)
    Fp = np.zeros(n, np.float32)
    Fc = np.zeros(n, np.float32)
    hit_k = np.full(n, -1, np.int64)
    samples = 0
    for k in range(n_steps):
        if active.size == 0:
            break
        samples += active.size
        with err():
            t = t_min + F(k) * step
            p = [dw[a][active] * t + o[a] for a in range(3)]
        obs, Fv = sample_nearest(vol, *p)
        with err():
            front = obs & prev_obs[active] & (Fp[active] >= 0) & (Fv < 0)
            back = obs & prev_obs[active] & (Fp[active] < 0) & (Fv >= 0)
        hit_k[active[front]] = k
        Fc[active[front]] = Fv[front]
        go = ~(front | back)
        upd = go & obs
        Fp[active[upd]] = Fv[upd]
        prev_obs[active[go]] = obs[go]
        active = active[go]
    depth = np.zeros(n, np.uint16)
    vmap = np.full((n, 3), np.nan, np.float32)
    nmap = np.full((n, 3), np.nan, np.float32)
    h = np.nonzero(hit_k >= 0)[0]
    if stats is not None:
        stats["samples"], stats["hits"] = samples, int(h.size)
    if h.size:
        with err():
            d = [dw[a][h] for a in range(3)]

            def tri_at(jj):
                tq = t_min + jj.astype(np.float32) * step
                return trilinear(vol, *[d[a] * tq + o[a] for a in range(3)])

            # the bracket (t_j, t_j+1) starts at j = k - 1 and moves one step at a time towards the surface until the trilinear pair encloses it
            j = hit_k[h] - 1
            vA, A = tri_at(j)
            vB, B = tri_at(j + 1)
            found = np.zeros(h.size, bool)
            alive = np.ones(h.size, bool)
            for s_ in range(BRACKETS):
                alive &= vA & vB
                found |= alive & (A >= 0) & (B < 0)
                alive &= ~found
                fwd = B >= 0
                alive &= ~np.where(fwd, j + 2 >= n_steps, j < 1)
                if s_ == BRACKETS - 1 or not alive.any():
                    break
                j = np.where(alive, j + np.where(fwd, 1, -1), j)
                vC, Cq = tri_at(np.where(fwd, j + 1, j))
                mf, mb = alive & fwd, alive & ~fwd
                A, vA, B, vB = (np.where(mf, B, np.where(mb, Cq, A)), np.where(mf, vB, np.where(mb, vC, vA)),
                                np.where(mf, Cq, np.where(mb, A, B)), np.where(mf, vC, np.where(mb, vA, vB)))
            j = np.where(found, j, hit_k[h] - 1)
            Ft = np.where(found, A, Fp[h])
            Ftdt = np.where(found, B, Fc[h])
            t0 = t_min + j.astype(np.float32) * step
            Ts = t0 - (step * Ft) / (Ftdt - Ft)
            vert = np.stack([Ts * dc[a][h] for a in range(3)], axis=1)
            mm = np.rint(vert[:, 2] * F(1000.0))
            okd = (mm >= 1) & (mm <= 65535)
            depth[h] = np.where(okd, mm, 0).astype(np.uint16)
            vmap[h] = vert
            hp = [d[a] * Ts + o[a] for a in range(3)]
            ok = np.ones(h.size, bool)
            g = []
            for a in range(3):
                hi = list(hp)
                lo = list(hp)
                hi[a] = hp[a] + ULF
                lo[a] = hp[a] - ULF
                va, A = trilinear(vol, *hi)
                vb, B = trilinear(vol, *lo)
                ok = ok & va & vb
                g.append(A - B)
            gl = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            ok = ok & (gl > 0)
            nw = [-g[a] / gl for a in range(3)]
            nc = np.stack([(R[0, a] * nw[0] + R[1, a] * nw[1]) + R[2, a] * nw[2] for a in range(3)], axis=1)
            nmap[h[ok]] = nc[ok]
    return depth.reshape(rows, cols), vmap.reshape(rows, cols, 3), nmap.reshape(rows, cols, 3)


def raycast_levels(units, cols, rows, cam4, T, levels, params=None):
    """Level l: cols / 2^l x rows / 2^l with cam4 / 2^l, the intrinsics odometry_restatement.Odometry.K(l) uses."""
    vol = units if isinstance(units, Volume) else Volume(units)
    cam = np.asarray(cam4, np.float32)
    return [raycast(vol, cols >> l, rows >> l, cam / F(2 ** l), T, params) for l in range(levels)]


def align_model(od, units, T_model, cur_frame, params=None, guess=None):
    """The frame-to-model route on restatements only: odometry_restatement.Odometry.align_maps with the ray-cast maps as the model."""
    model = raycast_levels(units, od.cols, od.rows, od.cam, T_model, od.levels, params)     # per level (depth, V, N), as Odometry.maps
    return od.align_maps(model, od.maps(cur_frame), guess)
