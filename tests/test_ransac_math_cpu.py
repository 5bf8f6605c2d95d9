"""csrc/er_ransac_math.h compiled for the host (tests/hostcheck/ransac_math_check.cpp) against the numpy restatement of
tests/ransac_restatement.py: the generator, selectSamples at every NS and at the smallest clouds, the polygon edge test at its edges,
the rigid estimate against a float64 Kabsch, and the terms of thresholdNormal.  The kernels of er_ransac.hip compile this text."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ransac_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def hostlib():
    if "lib" not in _cache:
        src = os.path.join(ROOT, "tests", "hostcheck", "ransac_math_check.cpp")
        inc = os.path.join(ROOT, "elasticreconstruction_amd", "csrc")
        out = os.path.join(ROOT, "tests", "hostcheck", "_build", "libransac_math_check.so")
        deps = [src, os.path.join(inc, "er_ransac_math.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I" + inc, src, "-o", out], check=True)
        _cache["lib"] = C.CDLL(out)
    return _cache["lib"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def h_draw(seed, it, d):
    seed, it, d = (np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.uint32), np.broadcast(seed, it, d).shape)).ravel() for x in (seed, it, d))
    out = np.zeros(seed.shape[0], np.uint32)
    hostlib().rs_draw(int(out.shape[0]), _p(seed), _p(it), _p(d), _p(out))
    return out


def h_select(seed, its, n, ns):
    its = np.ascontiguousarray(its, np.uint32)
    out = np.zeros((its.shape[0], ns), np.int32)
    assert hostlib().rs_select_samples(ns, C.c_uint(seed), int(its.shape[0]), _p(its), int(n), _p(out)) == 0
    return out


def h_estimate(P, Q):
    P, Q = np.ascontiguousarray(P, np.float64), np.ascontiguousarray(Q, np.float64)
    M = np.zeros((P.shape[0], 16), np.float32)
    hostlib().rs_rigid_estimate(int(P.shape[0]), int(P.shape[1]), _p(P), _p(Q), _p(M))
    return M.reshape(-1, 4, 4)


SEEDS = (0, 1, 0x7fffffff, 0x80000000, 0xffffffff)


def test_draw_and_index_of_are_bit_equal_to_the_restatement():
    g = np.random.default_rng(41)
    its = np.concatenate([np.array([0, 1, 1 << 20, (1 << 28) - 1], np.uint64), g.integers(0, 1 << 28, 100000).astype(np.uint64)])
    every = []
    for seed in SEEDS:
        for d in range(16):
            want = rr.draw(seed, its, d)
            got = h_draw(np.uint32(seed), its.astype(np.uint32), np.uint32(d))
            assert want.max() < 1 << 32 and np.array_equal(got.astype(np.uint64), want), (seed, d)
            every.append(got[:2000])
    assert int(h_draw(0, 0, 0)[0]) == 0xE220A8397B1DCDAF >> 32                                # splitmix64's first output for state 0
    r = np.concatenate(every + [np.array([0, 1, 0x7fffffff, 0x80000000, 0xffffffff], np.uint32)])
    for m in (1, 2, 3, 8, (1 << 27) - 1):
        out = np.zeros(r.shape[0], np.int32)
        hostlib().rs_index_of(int(r.shape[0]), _p(r), _p(np.full(r.shape[0], m, np.int32)), _p(out))
        assert np.array_equal(out.astype(np.int64), rr.index_of(r.astype(np.uint64), m)), m
        assert out.min() == 0 and out.max() == m - 1                                          # 0 .. m-1, both reached (r = 0 and r = 2^32 - 1)


@pytest.mark.parametrize("ns", (3, 4, 5, 6))
def test_select_samples_every_instantiation_down_to_n_equal_ns(ns):
    """n = NS leaves one possible set, n = NS + 1 makes every later draw collide with an earlier one most of the time; at n = 8000, the
    size the device tests use, two draws of an iteration collide about once in 1300 iterations."""
    its = np.arange(20000, dtype=np.uint64)
    its[-4:] = (1 << 20, (1 << 27) + 5, (1 << 28) - 2, (1 << 28) - 1)
    for n in (ns, ns + 1, 7, 50, 8000, (1 << 27) - 1):
        for seed in (7, 0xffffffff):
            got = h_select(seed, its, n, ns)
            assert np.array_equal(got.astype(np.int64), rr.select_samples(seed, its, n, ns)), (n, seed)
            assert (np.diff(got, axis=1) > 0).all() and got.min() >= 0 and got.max() < n      # ascending, hence distinct, inside the cloud
            if n <= 50:
                assert got.min() == 0 and got.max() == n - 1
            if n == ns:
                assert np.array_equal(got, np.broadcast_to(np.arange(ns, dtype=np.int32), got.shape))


def test_sqdist_and_edge_test_are_bit_equal_at_the_edges():
    g = np.random.default_rng(42)
    L = hostlib()
    m = 50000
    a, b = (g.random((m, 3)) * 3).astype(np.float32), (g.random((m, 3)) * 3).astype(np.float32)
    a2, b2 = (a + g.normal(scale=0.02, size=a.shape)).astype(np.float32), (b + g.normal(scale=0.02, size=a.shape)).astype(np.float32)
    d1, d2 = np.zeros(m, np.float32), np.zeros(m, np.float32)
    L.rs_sqdist(m, _p(a), _p(b), _p(d1))
    L.rs_sqdist(m, _p(a2), _p(b2), _p(d2))
    assert np.array_equal(d1.view(np.uint32), rr._sqdist32(a, b).view(np.uint32)) and np.array_equal(d2.view(np.uint32), rr._sqdist32(a2, b2).view(np.uint32))
    # through polygon_ok: one edge per row, source points a -> b, target points a2 -> b2 (about half pass at 0.98)
    s = np.stack([np.arange(m), np.arange(m) + m], axis=1)
    for sim in (0.0, 0.5, 0.9, 0.98):
        simsq = np.float32(sim) * np.float32(sim)
        ok = np.zeros(m, np.uint8)
        L.rs_edge_ok(m, _p(d1), _p(d2), C.c_float(simsq), _p(ok))
        want = rr.polygon_ok(np.concatenate([a, b]), np.concatenate([a2, b2]), s, s, sim)
        assert np.array_equal(ok.astype(bool), want), sim
        assert sim != 0.98 or 0.05 < want.mean() < 0.95
    # crafted lengths
    for sim in (0.0, 0.5, 0.9, 0.999):
        simsq = np.float32(sim) * np.float32(sim)
        up, dn = np.nextafter(simsq, np.float32(2)), np.nextafter(simsq, np.float32(-1))
        x = np.float32(2.5)
        ds = np.array([0, x, 0, x, simsq, 1, up, 1, dn, 1, simsq * x, np.nan, x], np.float32)
        dt = np.array([0, 0, x, x, 1, simsq, 1, up, 1, dn, x, x, np.nan], np.float32)
        want = np.array([0, sim == 0, sim == 0, 1, 1, 1, 1, 1, 0, 0, -1, 0, 0])
        ok = np.zeros(ds.shape[0], np.uint8)
        L.rs_edge_ok(int(ds.shape[0]), _p(ds), _p(dt), C.c_float(simsq), _p(ok))
        assert np.array_equal(ok.astype(bool), rr.edge_ok(ds, dt, simsq)), sim
        known = want >= 0
        assert np.array_equal(ok[known], want[known].astype(np.uint8)), (sim, ok, want)        # 0/0 fails, a ratio equal to simsq passes, one below fails


def _rotations(g, m):
    q = g.normal(size=(m, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], axis=1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], axis=1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def _judge(P, Q, what):
    """Every entry within one float32 spacing of the float64 Kabsch estimate rounded once; sets with sv[1] < 1e-6 sv[0] are left out."""
    M = h_estimate(P, Q)
    K, sv = rr.kabsch(P, Q)
    R = K.astype(np.float32)
    ok = sv[:, 1] >= 1e-6 * sv[:, 0]
    tol = np.spacing(np.maximum(np.abs(R), np.float32(1.0)).astype(np.float32))
    diff = np.abs(M.astype(np.float64) - R.astype(np.float64))
    print("rigid_estimate ns = %d, %s: %d sets, %d left out, worst |dM| / ulp = %.3f" % (P.shape[1], what, len(P), int((~ok).sum()), float((diff[ok] / tol[ok]).max())))
    assert (~ok).mean() <= 0.01 and ok.any(), what
    assert (diff[ok] <= tol[ok]).all(), what
    assert np.array_equal(M[:, 3], np.broadcast_to(np.array([0, 0, 0, 1], np.float32), (len(P), 4)))
    return M, ok


@pytest.mark.parametrize("ns", (3, 4, 5, 6))
def test_rigid_estimate_against_float64_kabsch(ns):
    """Horn's quaternion form by Jacobi sweeps against Kabsch's SVD.  Judged: random rigid motions of points in a 3 m cube with 0 - 2 cm
    noise, exactly planar sets, half turns about each axis, pure translations.  Not judged against Kabsch, observed instead:
      all points coincident (float32-valued coordinates, as the device feeds them: the centred points are exactly zero) -- the
        cross-covariance is zero, no sweep runs, the quaternion stays (1, 0, 0, 0): identity rotation, t = cq - cp, no NaN;
      collinear sets -- the largest eigenvalue is double, the sweeps converge on some vector of its plane: every entry finite, a proper
        rotation that carries the source line onto the target line (residual below 1e-6 m), the turn about the line arbitrary."""
    g = np.random.default_rng(100 + ns)
    m = 4000
    P = g.random((m, ns, 3)) * 3.0
    R = _rotations(g, m)
    t = g.normal(size=(m, 3))
    noise = g.random(m)[:, None, None] * 0.02 * g.normal(size=(m, ns, 3))
    _judge(P, np.einsum("mab,mib->mia", R, P) + t[:, None] + noise, "rigid motion + noise")
    _judge(P.astype(np.float32).astype(np.float64), (np.einsum("mab,mib->mia", R, P) + t[:, None] + noise).astype(np.float32).astype(np.float64), "the same from float32 points")
    flat = P.copy()
    flat[:, :, 2] = 1.25                                                                     # exactly planar in the source, planar to rounding in the target
    _judge(flat, np.einsum("mab,mib->mia", R, flat) + t[:, None], "planar")
    _judge(flat, flat + t[:, None], "planar, pure translation")
    for axis in range(3):
        D = -np.eye(3)
        D[axis, axis] = 1.0
        M, ok = _judge(P, P @ D.T + t[:, None], "half turn about axis %d" % axis)
        assert np.abs(M[ok][:, :3, :3] - D.astype(np.float32)).max() <= 1e-6
    M, ok = _judge(P, P + t[:, None], "pure translation")
    assert np.abs(M[ok][:, :3, :3] - np.eye(3, dtype=np.float32)).max() <= 1e-6
    # coincident points
    p1 = (g.random((m, 1, 3)) * 3.0).astype(np.float32).astype(np.float64)
    q1 = (g.random((m, 1, 3)) * 3.0).astype(np.float32).astype(np.float64)
    M = h_estimate(np.repeat(p1, ns, axis=1), np.repeat(q1, ns, axis=1))
    assert np.array_equal(M[:, :3, :3], np.broadcast_to(np.eye(3, dtype=np.float32), (m, 3, 3)))
    assert np.array_equal(M[:, :3, 3], (q1[:, 0] - p1[:, 0]).astype(np.float32)) and np.array_equal(M[:, 3], np.broadcast_to(np.array([0, 0, 0, 1], np.float32), (m, 4)))
    # collinear sets
    u, v = g.normal(size=(m, 1, 3)), g.normal(size=(m, 1, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    lam = g.random((m, ns, 1)) * 2.0 - 1.0
    Pc, Qc = p1 + lam * u, q1 + lam * v
    M = h_estimate(Pc, Qc).astype(np.float64)
    assert np.isfinite(M).all()
    Rm = M[:, :3, :3]
    assert np.abs(np.einsum("mab,mcb->mac", Rm, Rm) - np.eye(3)).max() < 1e-6 and np.abs(np.linalg.det(Rm) - 1.0).max() < 1e-6
    res = np.abs(np.einsum("mab,mib->mia", Rm, Pc) + M[:, None, :3, 3] - Qc).max()
    print("rigid_estimate ns = %d, collinear: worst residual %.3g" % (ns, res))
    assert res < 1e-6
    # the same line travelled backwards (a half turn about an axis the data does not name) and a zero-length line against a line
    Mb = h_estimate(Pc, q1 - lam * v)
    Mz = h_estimate(np.repeat(p1, ns, axis=1), Qc)
    assert np.isfinite(Mb).all() and np.isfinite(Mz).all()


def test_normal_dot_is_bit_equal_to_the_restatements_terms():
    g = np.random.default_rng(43)
    m, ns = 20000, 4
    M = np.zeros((m, 4, 4), np.float32)
    M[:, :3, :3] = _rotations(g, m)
    M[:, :3, 3] = g.normal(size=(m, 3))
    M[:, 3, 3] = 1
    sn, tn = g.normal(size=(m * ns, 3)).astype(np.float32), g.normal(size=(m * ns, 3)).astype(np.float32)
    sn /= np.linalg.norm(sn, axis=1, keepdims=True)
    tn /= np.linalg.norm(tn, axis=1, keepdims=True)
    sn[g.random(m * ns) < 0.05] = np.nan
    tn[g.random(m * ns) < 0.05] = np.nan
    idx = np.arange(m * ns).reshape(m, ns)
    want = rr.normal_dots(M, sn, tn, idx, idx)
    for i in range(ns):
        out = np.zeros(m, np.float32)
        hostlib().rs_normal_dot(m, _p(np.ascontiguousarray(M.reshape(m, 16))), _p(np.ascontiguousarray(sn[idx[:, i]])), _p(np.ascontiguousarray(tn[idx[:, i]])), _p(out))
        nan = np.isnan(want[:, i])
        assert 0.05 < nan.mean() < 0.15 and np.array_equal(np.isnan(out), nan)
        assert np.array_equal(out[~nan].view(np.uint32), want[~nan, i].view(np.uint32))
