"""Mesh smoothing without a GPU: the numpy restatement against a plain-Python loop and against known answers, what each
crafted mesh of tests/mesh_smooth_cases.py is meant to reach, what smoothing is for on a noisy sphere, csrc/er_mesh_smooth_math.h compiled
for the host against the restatement, the new symbols and defaults, the refusals that need no device and the programs' command lines."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_smooth_cases as cases
import mesh_smooth_restatement as rs
from elasticreconstruction_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NOT_A_HANDLE = C.create_string_buffer(4096)
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b, what=""):
    """two results of a smoothing, bit for bit; NaN normals by position"""
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in a:
        x, y = a[k], b[k]
        if k == "stats":
            assert tuple(x) == tuple(y), (what, k, x, y)
        elif k == "normals":
            assert x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y)), (what, k)
            assert np.array_equal(bits(x)[~np.isnan(x)], bits(y)[~np.isnan(y)]), (what, k, int((bits(x) != bits(y)).sum()))
        elif k == "verts":
            assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), (what, k, int((bits(x) != bits(y)).sum()))
        else:
            assert x.dtype == y.dtype and np.array_equal(x, y), (what, k)


def loop_smooth(verts, tris, iterations, lam, mu, fix_boundary):
    """The definitions once more, one vertex and one corner at a time, with Python sets and integers."""
    verts, tris = np.asarray(verts, np.float32), np.asarray(tris, np.int32).reshape(-1, 3)
    nv = len(verts)
    count = {}
    for t in tris:
        for c in range(3):
            u, w = int(t[c]), int(t[(c + 1) % 3])
            if u != w:
                count[(min(u, w), max(u, w))] = count.get((min(u, w), max(u, w)), 0) + 1
    N = [set() for _ in range(nv)]
    boundary = np.zeros(nv, np.uint8)
    for (u, w), m in count.items():
        N[u].add(w)
        N[w].add(u)
        if m == 1:
            boundary[u] = boundary[w] = 1
    p = verts[:, :3].copy()
    still = [len(N[v]) == 0 or bool(fix_boundary and boundary[v]) for v in range(nv)]
    for _ in range(iterations):
        for f in (np.float32(lam), np.float32(mu)):
            if f == 0:
                continue
            new = p.copy()
            for v in range(nv):
                if still[v]:
                    continue
                for a in range(3):
                    S = sum(int(np.rint(np.float64(p[w, a]) * 2.0 ** 20)) for w in N[v])
                    m = (np.float64(S) / np.float64(len(N[v]))) * np.float64(2.0 ** -20)
                    d = m - np.float64(p[v, a])
                    new[v, a] = np.float32(np.float64(p[v, a]) + np.float64(f) * d)
            p = new
    sums = [[0, 0, 0] for _ in range(nv)]
    for t in tris:
        a, b, c = (p[int(i)].astype(np.float64) for i in t)
        d1, d2 = b - a, c - a
        for q in range(3):
            r, s = (q + 1) % 3, (q + 2) % 3
            k = int(np.rint((d1[r] * d2[s] - d1[s] * d2[r]) * 2.0 ** 32))
            for i in t:
                sums[int(i)][q] += k
    normals = np.zeros((nv, 3), np.float32)
    for v in range(nv):
        g = [np.float64(((x + 2 ** 63) % 2 ** 64) - 2 ** 63) for x in sums[v]]           # (wrapped to int64)
        length = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
        normals[v] = [np.float32(x / length) for x in g] if length != 0 else np.nan
    out = np.zeros((nv, 4), np.float32)
    out[:, :3] = p
    return dict(verts=out, normals=normals, degree=np.array([len(n) for n in N], np.int32).reshape(nv), boundary=boundary,
                stats=(len(count), sum(m == 1 for m in count.values()), sum(m >= 3 for m in count.values()), int(sum(still))))


def crafted():
    if "crafted" not in _cache:
        _cache["crafted"] = cases.crafted()
    return _cache["crafted"]


SMALL = ["isolated vertex", "open fan", "open fan, boundary fixed", "closed fan", "closed fan, boundary fixed", "tetrahedron", "tetrahedron, lambda 1",
         "two on an edge, equal winding", "two on an edge, opposite winding", "three on an edge", "three on an edge, boundary fixed", "duplicated triangle",
         "a a b and a a a", "grid", "grid, boundary fixed", "grid in reverse order", "flat grid, boundary fixed", "negative zeros",
         "negative zeros, boundary fixed", "ties", "mu 0", "lambda 0", "lambda 0 and mu 0", "lambda 1, mu -1"]


@pytest.mark.parametrize("name", SMALL)
def test_restatement_equals_a_plain_loop(name):
    m = crafted()[name]
    same(rs.smooth(**m), loop_smooth(**m), name)


def test_restatement_equals_a_plain_loop_on_random_meshes():
    S = cases.sizes()
    for name in ("nv 2, nt 4, 2 iterations", "nv 3, nt 6, 10 iterations", "nv 65, nt 130, 2 iterations", "nv 257, nt 514, 1 iterations", "nv 63, nt 126, 0 iterations"):
        same(rs.smooth(**S[name]), loop_smooth(**S[name]), name)


def test_restatement_known_answers():
    # one pass with lambda = 1 on a tetrahedron with dyadic coordinates: every vertex lands on the mean of the other three
    r = rs.smooth(**cases.tetrahedron(iterations=1, lam=1.0, mu=0.0))
    for v in range(4):
        others = [w for w in range(4) if w != v]
        assert r["verts"][v, :3].tolist() == (cases.TETRA[others].sum(axis=0) / 3.0).tolist() and r["verts"][v, 3] == 0
    assert r["degree"].tolist() == [3] * 4 and not r["boundary"].any() and r["stats"] == (6, 0, 0, 0)
    r = rs.smooth(**cases.tetrahedron(iterations=0))          # (that pass turned the tetrahedron inside out: the normals of the one that went in)
    n = r["normals"].astype(np.float64)
    centre = r["verts"][:, :3].mean(axis=0)
    assert ((r["verts"][:, :3] - centre) * n).sum(axis=1).min() > 0, "the outward winding gives outward normals"
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6
    # a planar grid at multiples of 2^-10 with its boundary fixed: every bit stays, after any number of iterations
    for it in (1, 2, 7, 50):
        g = cases.grid(9, 7, iterations=it, fix_boundary=True)
        r = rs.smooth(**g)
        assert np.array_equal(bits(r["verts"][:, :3]), bits(g["verts"][:, :3])) and not r["verts"][:, 3].any(), it
        assert r["normals"].tolist() == [[0.0, 0.0, 1.0]] * 63
        assert r["stats"] == (9 * 6 + 8 * 7 + 8 * 6, 2 * 8 + 2 * 6, 0, 2 * 9 + 2 * 5), r["stats"]
    assert not np.array_equal(rs.smooth(**cases.grid(9, 7, iterations=1))["verts"][:, :3], g["verts"][:, :3]), "the boundary moves when it is not fixed"
    # nothing in, nothing out; no triangle: the positions pass through
    r = rs.smooth(np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    assert r["verts"].shape == (0, 4) and r["stats"] == (0, 0, 0, 0)
    v = np.arange(15, dtype=np.float32).reshape(5, 3)
    r = rs.smooth(v, np.zeros((0, 3), np.int32), 3)
    assert np.array_equal(r["verts"][:, :3], v) and np.isnan(r["normals"]).all() and not r["degree"].any() and r["stats"] == (0, 0, 0, 5)
    # iterations == 0: the input's bits, and the normals of the mesh as it is
    m = crafted()["grid"]
    r = rs.smooth(**dict(m, iterations=0))
    assert np.array_equal(bits(r["verts"][:, :3]), bits(m["verts"][:, :3])) and not r["verts"][:, 3].any() and not np.isnan(r["normals"]).any()
    # refusals
    for bad, words in (([[np.nan, 0, 0]], "vertex 1 has a coordinate"), ([[4096.0, 0, 0]], "vertex 1 has a coordinate"), ([[0, -np.inf, 0]], "vertex 1 has")):
        with pytest.raises(ValueError, match=words):
            rs.smooth(np.concatenate([[[0, 0, 0]], bad, [[np.inf, 0, 0]]]), [[0, 1, 2]])
    with pytest.raises(ValueError, match=r"triangle 1 names vertex 3, outside \[0, 3\)"):
        rs.smooth(np.zeros((3, 3)), [[0, 1, 2], [0, 3, -1], [9, 9, 9]])
    for kw in (dict(iterations=-1), dict(iterations=1025), dict(lam=1.5), dict(mu=-1.0000001), dict(lam=np.nan), dict(mu=np.inf)):
        with pytest.raises(ValueError, match="iterations|lambda|mu"):
            rs.smooth(np.zeros((3, 3)), [[0, 1, 2]], **kw)


def test_crafted_meshes_reach_what_they_are_meant_to_reach():
    C_ = crafted()
    r = {k: rs.smooth(**m) for k, m in C_.items() if k != "tetrahedron, 1024 iterations"}
    iso = r["isolated vertex"]
    assert iso["degree"].tolist() == [2, 3, 3, 2, 0, 0] and iso["stats"] == (5, 4, 0, 2)
    assert np.array_equal(bits(iso["verts"][4:, :3]), bits(C_["isolated vertex"]["verts"][4:, :3])) and np.isnan(iso["normals"][4:]).all()
    hub = r["hub of degree 65536"]
    assert hub["degree"][0] == 65536 and hub["degree"][1:].max() == 3 and hub["boundary"].all() and hub["stats"] == (2 * 65536 - 1, 65536 + 1, 0, 0)
    assert r["open fan"]["boundary"].all() and r["open fan, boundary fixed"]["stats"][3] == 10
    assert np.array_equal(r["open fan, boundary fixed"]["verts"][:, :3], C_["open fan"]["verts"][:, :3])
    closed = r["closed fan"]
    assert closed["boundary"].tolist() == [0] + [1] * 9 and closed["degree"].tolist() == [9] + [3] * 9
    fixed = r["closed fan, boundary fixed"]
    assert fixed["stats"][3] == 9 and not np.array_equal(fixed["verts"][0], C_["closed fan"]["verts"][0]) and np.array_equal(fixed["verts"][1:, :3], C_["closed fan"]["verts"][1:, :3])
    assert not r["tetrahedron"]["boundary"].any() and r["tetrahedron"]["stats"] == (6, 0, 0, 0)
    for k in ("two on an edge, equal winding", "two on an edge, opposite winding"):
        assert r[k]["degree"].tolist() == [3, 3, 2, 2] and r[k]["stats"] == (5, 4, 0, 0) and r[k]["boundary"].all(), k
    assert not np.array_equal(bits(r["two on an edge, equal winding"]["normals"]), bits(r["two on an edge, opposite winding"]["normals"]))
    three = r["three on an edge"]
    lo, hi, mult = rs.edges(C_["three on an edge"]["tris"])
    assert mult[(lo == 0) & (hi == 1)].tolist() == [3] and three["stats"] == (7, 6, 1, 0) and three["degree"].tolist() == [4, 4, 2, 2, 2] and three["boundary"].all()
    assert r["three on an edge, boundary fixed"]["stats"][3] == 5
    dup = r["duplicated triangle"]
    lo, hi, mult = rs.edges(C_["duplicated triangle"]["tris"])
    assert mult.tolist() == [2, 2, 3, 1, 1] and dup["degree"].tolist() == [2, 3, 3, 2] and dup["boundary"].tolist() == [0, 1, 1, 1] and dup["stats"] == (5, 2, 1, 0)
    aab = r["a a b and a a a"]
    lo, hi, mult = rs.edges(C_["a a b and a a a"]["tris"])
    assert list(zip(lo.tolist(), hi.tolist(), mult.tolist())) == [(0, 1, 2), (1, 2, 1), (1, 3, 1), (2, 3, 1), (3, 4, 2)]
    assert aab["degree"].tolist() == [1, 3, 2, 3, 1, 0] and aab["boundary"].tolist() == [0, 1, 1, 1, 0, 0]
    # the same surface in the reverse index order gives the same positions in the reverse order
    assert np.array_equal(bits(r["grid in reverse order"]["verts"][::-1]), bits(r["grid"]["verts"]))
    assert np.array_equal(bits(r["grid in reverse order"]["normals"][::-1]), bits(r["grid"]["normals"]))
    assert np.array_equal(r["grid, boundary fixed"]["verts"][r["grid"]["boundary"] != 0, :3], C_["grid"]["verts"][r["grid"]["boundary"] != 0, :3])
    for name, stride, m in (("progressions, stride 1", 1, 4096), ("progressions, stride 2^4", 16, 4096), ("progressions, stride 2^8", 256, 1024), ("progressions, stride 2^16", 65536, 16)):
        lo, hi, _ = rs.edges(C_[name]["tris"])
        key = (lo << 32) | hi
        fan_ = np.sort(key[(lo == 0) & (hi > 2)])
        steps = np.diff(fan_) if stride == 1 else np.diff(fan_[::2])
        assert len(fan_) >= m - 1 and (steps == stride).all(), name
        strip = np.sort(key[(hi == lo + 1) & (lo % stride == 0)]) if stride > 1 else np.sort(key[hi == lo + 1])
        assert len(strip) >= m and (np.diff(strip) == stride * (2 ** 32 + 1)).all(), name
    z = C_["negative zeros"]["verts"]
    assert np.signbit(z[0, :3]).all() and r["negative zeros"]["degree"][0] == 0 and np.signbit(r["negative zeros"]["verts"][0, :3]).all()
    assert not np.signbit(r["negative zeros"]["verts"][0, 3]) and np.signbit(r["negative zeros"]["verts"][1:, :3]).any()
    assert np.array_equal(bits(r["negative zeros, boundary fixed"]["verts"][:, :3]), bits(z[:, :3])), "every vertex of an open fan is a boundary vertex"
    t = C_["ties"]
    frac = t["verts"][:, 0].astype(np.float64) * 2.0 ** 20
    assert (frac - np.floor(frac) == 0.5).all() and (np.floor(frac) % 2 == 0).any() and (np.floor(frac) % 2 == 1).any()
    assert (rs.quantise(t["verts"][:, :3]) % 2 == 0).all(), "half to even"
    c = C_["cancellation"]
    assert r["cancellation"]["degree"][:300].tolist() == [3] * 300 and np.abs(r["cancellation"]["verts"][:300, :3]).max() < 1e-15
    assert (bits(r["cancellation"]["verts"][:300, :3]) != bits(fused_moves(c["verts"][:300, :3], 7 * rs.quantise(c["verts"][:300, :3]), 3, -0.75))).mean() > 0.3
    assert np.array_equal(bits(r["lambda 0 and mu 0"]["verts"][:, :3]), bits(C_["lambda 0 and mu 0"]["verts"][:, :3]))
    one = rs.smooth(**dict(C_["mu 0"], iterations=1))
    assert not np.array_equal(one["verts"], r["mu 0"]["verts"]) and not np.array_equal(r["lambda 0"]["verts"], r["mu 0"]["verts"])


def test_guard_cases_leave_the_range_where_they_are_meant_to():
    for name, (m, number, vertex) in cases.guards().items():
        with pytest.raises(ValueError, match=r"pass \d+ moves vertex \d+ ") as e:
            rs.smooth(**m)
        got = tuple(int(x) for x in re.search(r"pass (\d+) moves vertex (\d+) ", str(e.value)).groups())
        if name == "second iteration":
            assert got[0] >= 2, got
        elif name == "two blocks":
            assert got == (1, 2100) and rs.adjacency(m["tris"], 4097)["degree"][[2100, 3000]].min() > 0, got
        else:
            assert got == (number, vertex), (name, got)


def test_a_thousand_iterations_on_a_tetrahedron_stay_finite():
    m = crafted()["tetrahedron, 1024 iterations"]
    r = rs.smooth(**m)
    assert np.isfinite(r["verts"]).all() and np.ptp(r["verts"][:, :3], axis=0).max() < 1e-3, "lambda | mu contracts the complete graph"


def test_what_smoothing_is_for():
    """A 4-times subdivided icosphere of radius 0.5 m with 1 % radial noise: ten Taubin iterations more than halve the spread of the radii and
    move the mean radius less than a tenth as far as ten Laplacian iterations do.  Measured: input std 0.00501 mean 0.49997; Taubin std
    0.00188 mean 0.50038; Laplacian std 0.00093 mean 0.49290."""
    v, t = cases.icosphere()
    assert v.shape == (2562, 3) and t.shape == (5120, 3)
    radius = lambda r: np.linalg.norm(r["verts"][:, :3].astype(np.float64), axis=1)
    r0 = np.linalg.norm(v.astype(np.float32).astype(np.float64), axis=1)
    taubin = radius(rs.smooth(v, t, 10))
    laplace = radius(rs.smooth(v, t, 10, mu=0.0))
    print("radius std, mean: input %.5f %.5f, Taubin %.5f %.5f, Laplacian %.5f %.5f" % (r0.std(), r0.mean(), taubin.std(), taubin.mean(), laplace.std(), laplace.mean()))
    assert taubin.std() < 0.5 * r0.std()
    assert abs(taubin.mean() - r0.mean()) < 0.1 * abs(laplace.mean() - r0.mean())
    n = rs.smooth(v, t, 10)["normals"].astype(np.float64)
    p = rs.smooth(v, t, 10)["verts"][:, :3].astype(np.float64)
    assert ((p / np.linalg.norm(p, axis=1, keepdims=True)) * n).sum(axis=1).min() > 0.95, "the normals of a smoothed sphere point outwards"


def fused_moves(p, S, deg, f):
    """rs.move with the product and the sum of the last step rounded ONCE, as a fused multiply-add would: exact in rationals, then to float64"""
    from fractions import Fraction
    m = (S.astype(np.float64) / np.float64(deg)) * 2.0 ** -20
    d = m - p.astype(np.float64)
    out = [np.float32(float(Fraction(float(a)) + Fraction(float(np.float32(f))) * Fraction(float(b)))) for a, b in zip(p.reshape(-1), d.reshape(-1))]
    return np.array(out, np.float32).reshape(p.shape)


def hostlib():
    if "lib" not in _cache:
        src = os.path.join(ROOT, "tests", "hostcheck", "mesh_smooth_math_check.cpp")
        inc = os.path.join(ROOT, "elasticreconstruction_amd", "csrc")
        out = os.path.join(ROOT, "tests", "hostcheck", "_build", "libmesh_smooth_math_check.so")
        deps = [src, os.path.join(inc, "er_mesh_smooth_math.h"), os.path.join(inc, "er_mesh_simplify_math.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I" + inc, src, "-o", out], check=True)
        _cache["lib"] = C.CDLL(out)
    return _cache["lib"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_host_math_equals_the_restatement():
    """er_mesh_smooth_math.h on the host, bit for bit: 1.2 million (vertex, neighbour sum) cases per factor, cross products of random triangles
    and of triangles at the 4096 m edge, the finish of a normal, the predicates and the edge keys."""
    L = hostlib()
    rng = np.random.default_rng(23)
    n = 1200000
    big = np.nextafter(np.float32(4096.0), np.float32(0.0))
    edge = np.array([0.0, -0.0, big, -big, 2048.0, -2048.0, 1e-45, -1e-45, 1.1754944e-38, 0.5, -0.5, 4095.0], np.float32)
    p = np.concatenate([rng.uniform(-3, 3, (n, 3)), rng.uniform(-4096, 4096, (n // 8, 3)), rng.choice(edge, (20000, 3))]).astype(np.float32)
    m = len(p)
    deg = rng.integers(1, 2 ** rng.integers(1, 18, m), m).astype(np.int32)
    # sums near deg * p (a vertex among its neighbours), far from it, and beyond 2^53
    S = np.rint((p.astype(np.float64) + rng.normal(0, 0.01, (m, 3))) * deg[:, None] * 2.0 ** 20).astype(np.int64)
    S[::5] = (rng.uniform(-4096, 4096, (len(S[::5]), 3)) * deg[::5, None] * 2.0 ** 20).astype(np.int64)
    S[::11] = 0
    far = rng.integers(0, m, 50000)
    deg[far] = rng.integers(2 ** 22, 2 ** 31 - 1, len(far)).astype(np.int32)
    S[far] = (rng.uniform(-4095, 4095, (len(far), 3)) * deg[far, None].astype(np.float64) * 2.0 ** 20).astype(np.int64)
    assert (np.abs(S) > 2 ** 53).any()
    for f in (0.5, -0.53, 1.0, -1.0, 0.33, 1e-3):
        got = np.zeros((m, 3), np.float32)
        L.sm_moves(C.c_long(m), _p(p), _p(S), _p(deg), C.c_float(f), _p(got))
        want = rs.move(p, S, deg, f)
        assert np.array_equal(bits(got), bits(want)), f
    # the stars of cases.cancellation(): the rows on which a fused multiply-add in the update gives other bits
    c = cases.cancellation()
    pc = c["verts"][:300, :3].copy()
    Sc = 7 * rs.quantise(pc)
    got = np.zeros_like(pc)
    L.sm_moves(C.c_long(300), _p(pc), _p(Sc), _p(np.full(300, 3, np.int32)), C.c_float(-0.75), _p(got))
    assert np.array_equal(bits(got), bits(rs.smooth(**c)["verts"][:300, :3])) and np.array_equal(bits(got), bits(rs.move(pc, Sc, np.full(300, 3), -0.75)))
    assert (bits(got) != bits(fused_moves(pc, Sc, 3, -0.75))).mean() > 0.3
    # cross products: random triangles, and triangles whose corners lie at +-4096 m (|k| up to 2^59)
    tri = np.concatenate([rng.uniform(-1, 1, (n // 2, 3, 3)), rng.uniform(-4096, 4096, (n // 4, 3, 3)), rng.choice(np.array([big, -big, 0.0, 1.0], np.float32), (50000, 3, 3)),
                          (rng.uniform(-1, 1, (n // 4, 1, 3)) + rng.normal(0, 1e-3, (n // 4, 3, 3)))]).astype(np.float32)
    tri[0] = [[-big, -big, -big], [big, -big, -big], [-big, big, -big]]
    k = np.zeros((len(tri), 3), np.int64)
    L.sm_area_normals(C.c_long(len(tri)), _p(tri), _p(k))
    flat = tri.reshape(-1, 3)
    want = rs.area_normals(flat, np.arange(len(flat)).reshape(-1, 3))
    assert np.array_equal(k, want) and np.abs(k).max() > 2 ** 57 and np.abs(k).max() < 2 ** 59 and k[0].tolist() == [0, 0, int((2.0 * float(big)) ** 2 * 2.0 ** 32)]
    # the finish of a normal
    N = (rng.normal(size=(n, 3)) * 2.0 ** rng.integers(0, 62, (n, 1))).clip(-2.0 ** 62, 2.0 ** 62).astype(np.int64)
    N[:1000] = 0
    N[1000:2000, 1:] = 0
    got = np.zeros((n, 3), np.float32)
    L.sm_normals(C.c_long(n), _p(N), _p(got))
    want = rs.finish_normal(N)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want[:1000]).all() and np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)])
    # predicates and keys
    q = np.concatenate([rng.choice(np.concatenate([edge, np.array([np.nan, np.inf, -np.inf, 4096.0, -4096.0], np.float32)]), (20000, 3)), p[:1000]]).astype(np.float32)
    ok = np.zeros(len(q), np.int32)
    L.sm_positions_ok(C.c_long(len(q)), _p(q), _p(ok))
    assert np.array_equal(ok != 0, rs.position_ok(q)) and (ok == 0).any() and (ok != 0).any()
    f = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)), -1.5, np.nan, np.inf, -np.inf, 0.5, -0.53], np.float32)
    ok = np.zeros(len(f), np.int32)
    L.sm_factors_ok(C.c_long(len(f)), _p(f), _p(ok))
    assert ok.tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1]
    uw = rng.integers(0, 2 ** 31 - 1, (100000, 2)).astype(np.int32)
    key = np.zeros(len(uw), np.uint64)
    L.sm_edge_keys(C.c_long(len(uw)), _p(uw), _p(key))
    assert np.array_equal(key, (uw.min(axis=1).astype(np.uint64) << np.uint64(32)) | uw.max(axis=1).astype(np.uint64))


def test_new_symbols_are_in_the_header_the_binding_and_the_library():
    hdr = open(os.path.join(ROOT, "include", "er_hip.h")).read()
    L = _ffi.lib()
    for sym in ("er_mesh_smooth", "er_tsdf_extract_mesh_smoothed"):
        assert re.search(r"\bint %s\(" % sym, hdr) and sym in _ffi.SYMBOLS and hasattr(L, sym), sym
    from elasticreconstruction_amd import mesh
    from elasticreconstruction_amd.tsdf import TSDFVolume
    d = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d(mesh.smooth) == dict(iterations=10, lam=0.5, mu=-0.53, fix_boundary=False, device=0, probes=False)
    assert d(TSDFVolume.extract_smoothed_mesh) == dict(lam=0.5, mu=-0.53, fix_boundary=False, cell=0.0, min_triangles=0, largest_only=False, colors=False, stats=False)
    s = d(TSDFVolume.SaveMesh)
    assert (s["smooth"], s["smooth_lambda"], s["smooth_mu"], s["smooth_fix_boundary"]) == (0, 0.5, -0.53, False)
    assert d(rs.smooth) == dict(iterations=10, lam=0.5, mu=-0.53, fix_boundary=False)


def test_refusals_that_need_no_device():
    L = _ffi.lib()
    err = lambda: L.er_last_error().decode()
    v = np.zeros((3, 4), np.float32)
    tri = np.array([[0, 1, 2]], np.int32)
    out = np.full((3, 4), -7, np.float32)
    st = (C.c_long * 4)(-7, -7, -7, -7)
    p = lambda a: None if a is None else _ffi.ptr(a)

    def call(vv=v, n=3, tt=tri, m=1, it=1, lam=0.5, mu=-0.53):
        return L.er_mesh_smooth(p(vv), n, p(tt), m, it, C.c_float(lam), C.c_float(mu), 0, 0, p(out), None, None, None, st, None)

    assert call(vv=None) != 0 and err() == "er_mesh_smooth: NULL argument"
    assert call(tt=None) != 0 and err() == "er_mesh_smooth: NULL argument"
    assert call(n=-3) != 0 and "-3 vertices" in err()
    assert call(m=-1) != 0 and "-1 triangles" in err()
    assert call(n=2 ** 31) != 0 and "2^31 - 1" in err()
    assert call(m=(2 ** 31 - 1) // 3 + 1) != 0 and "2^31 - 1" in err()
    nv, nt = C.c_long(-7), C.c_long(-7)
    fake = C.cast(_NOT_A_HANDLE, C.c_void_p)                 # never dereferenced: every call with it is refused before the handle is looked at

    def ts(h, pv, pt, it=1, lam=0.5, mu=-0.53, cell=0.0, mt=0, colors=None, want=0):
        return L.er_tsdf_extract_mesh_smoothed(h, it, C.c_float(lam), C.c_float(mu), 0, C.c_float(cell), mt, 0, want, None, None, p(colors), 0, None, 0, pv, pt, None, None, None)

    assert ts(None, C.byref(nv), C.byref(nt)) != 0 and err() == "er_tsdf_extract_mesh_smoothed: NULL argument"
    assert ts(fake, None, C.byref(nt)) != 0 and err() == "er_tsdf_extract_mesh_smoothed: NULL argument"
    assert ts(fake, C.byref(nv), None) != 0 and err() == "er_tsdf_extract_mesh_smoothed: NULL argument"
    assert ts(fake, C.byref(nv), C.byref(nt), mt=-1) != 0 and err() == "er_tsdf_extract_mesh_smoothed: min_triangles = -1"
    assert ts(fake, C.byref(nv), C.byref(nt), colors=np.zeros((3, 4), np.uint8)) != 0 and "without want_colors" in err()
    if L.er_device_count() <= 0:
        assert call() != 0 and err() == "er_mesh_smooth: no HIP device available (liber_hip has no CPU fallback)"
        assert ts(fake, C.byref(nv), C.byref(nt)) != 0
        assert err() == "er_tsdf_extract_mesh_smoothed: no HIP device available (liber_hip has no CPU fallback)"
    else:
        for kw, words in ((dict(it=-1), "iterations = -1"), (dict(it=1025), "iterations = 1025"), (dict(lam=1.5), "lambda = 1.5"), (dict(mu=float("nan")), "mu = nan"),
                          (dict(mu=float("-inf")), "mu = -inf"), (dict(lam=-1.0000001), "lambda = -1")):
            assert call(**kw) != 0 and err().startswith("er_mesh_smooth: " + words), (kw, err())
            assert ts(fake, C.byref(nv), C.byref(nt), **kw) != 0 and err().startswith("er_tsdf_extract_mesh_smoothed: " + words), (kw, err())
        for cell in (-1.0, float("nan"), float("inf")):
            assert ts(fake, C.byref(nv), C.byref(nt), cell=cell) != 0 and "finite and not below 0" in err(), cell
    assert (nv.value, nt.value) == (-7, -7) and (out == -7).all() and tuple(st) == (-7,) * 4


def test_programs_name_the_new_flags_and_refuse_bad_values():
    bin_ = os.path.join(ROOT, "elasticreconstruction_amd", "bin")
    readme = os.path.join(ROOT, "README.md")
    r = subprocess.run([os.path.join(bin_, "MeshOutput"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(f in r.stdout for f in ("--smooth <n>", "--smooth_lambda", "--smooth_mu", "--smooth_fix_boundary")), r.stdout
    r = subprocess.run([os.path.join(bin_, "Integrate"), "--help"], capture_output=True, text=True, timeout=60)
    assert all(f in r.stdout + r.stderr for f in ("--mesh_smooth <n>", "--mesh_smooth_lambda", "--mesh_smooth_mu", "--mesh_smooth_fix_boundary"))
    for args, flag in ((["--smooth", "-1"], "--smooth"), (["--smooth", "1025"], "--smooth"), (["--smooth", "abc"], "--smooth"), (["--smooth", "2.5"], "--smooth"),
                       (["--smooth"], "--smooth"), (["--smooth", "3", "--smooth_lambda", "1.5"], "--smooth_lambda"), (["--smooth", "3", "--smooth_mu", "nan"], "--smooth_mu"),
                       (["--smooth", "3", "--smooth_mu", "x"], "--smooth_mu"), (["--smooth_mu", "-0.5"], "--smooth <iterations>"),
                       (["--smooth_fix_boundary"], "--smooth <iterations>")):
        r = subprocess.run([os.path.join(bin_, "MeshOutput"), readme] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and flag in r.stderr, (args, r.stderr)
    raw = ["--depth_raw", readme]                              # (a file that exists: the depth source is looked for before the switches)
    for args, words in ((["--mesh_smooth", "3"], "--mesh_smooth needs --save_mesh"), (["--save_mesh", "m.ply", "--mesh_smooth", "-2"], "--mesh_smooth needs a whole number"),
                        (["--save_mesh", "m.ply", "--mesh_smooth", "2", "--mesh_smooth_mu", "7"], "--mesh_smooth_mu needs a finite factor")):
        r = subprocess.run([os.path.join(bin_, "Integrate")] + raw + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and words in r.stderr, (args, r.stderr, r.stdout)
