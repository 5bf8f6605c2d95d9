"""Vertex clustering without a GPU: the numpy restatement against a plain-Python loop and against known answers, what each
crafted mesh of tests/mesh_simplify_cases.py is meant to reach, csrc/er_mesh_simplify_math.h compiled for the host against the restatement,
the new symbols, the refusals that need no device and the programs' command lines."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_simplify_cases as cases
import mesh_simplify_restatement as rs
from elasticreconstruction_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NOT_A_HANDLE = C.create_string_buffer(4096)
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b, what=""):
    """two results of a simplification, bit for bit; NaN normals by position"""
    assert set(a) == set(b)
    for k in a:
        x, y = a[k], b[k]
        if k == "stats":
            assert tuple(x) == tuple(y), (what, k, x, y)
        elif x is None or y is None:
            assert x is None and y is None, (what, k)
        elif k in ("verts", "normals"):
            assert x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y)), (what, k)
            assert np.array_equal(bits(x)[~np.isnan(x)], bits(y)[~np.isnan(y)]), (what, k, int((bits(x) != bits(y)).sum()))
        else:
            assert x.dtype == y.dtype and np.array_equal(x, y), (what, k)


def loop_simplify(verts, tris, cell, normals=None, colors=None):
    """The definitions once more, one vertex and one triangle at a time, with Python integers and floats."""
    verts, tris = np.asarray(verts, np.float32), np.asarray(tris, np.int32).reshape(-1, 3)
    nv, nt = len(verts), len(tris)
    cell = float(np.float32(cell))
    clusters, key_of = {}, []
    for v in range(nv):
        key = tuple(math.floor(float(verts[v, a]) / cell) for a in range(3))
        clusters.setdefault(key, []).append(v)
        key_of.append(key)
    lead = [clusters[k][0] for k in key_of]
    keep, seen, degenerate = [], set(), 0
    for t in range(nt):
        A, B, Cc = (lead[i] for i in tris[t])
        if A == B or B == Cc or A == Cc:
            degenerate += 1
            continue
        m = min(A, B, Cc)
        canon = (A, B, Cc) if m == A else (B, Cc, A) if m == B else (Cc, A, B)
        if canon not in seen:
            seen.add(canon)
            keep.append(t)
    named = sorted({lead[i] for t in keep for i in tris[t]})
    rank = {l: i for i, l in enumerate(named)}
    out_v, out_n, out_c, members = np.zeros((len(named), 4), np.float32), np.zeros((len(named), 3), np.float32), np.zeros((len(named), 4), np.uint8), []
    for i, l in enumerate(named):
        mem = clusters[key_of[l]]
        members.append(len(mem))
        for a in range(3):
            S = sum(int(np.rint(np.float64(verts[v, a]) * 2.0 ** 20)) for v in mem)
            out_v[i, a] = np.float32((np.float64(S) / np.float64(len(mem))) * 2.0 ** -20)
        if normals is not None:
            who = [v for v in mem if all(np.isfinite(normals[v, a]) and abs(normals[v, a]) < 4096 for a in range(3))]
            g = [np.float64(sum(int(np.rint(np.float64(normals[v, a]) * 2.0 ** 20)) for v in who)) for a in range(3)]
            length = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            out_n[i] = [np.float32(x / length) for x in g] if who and length != 0 else np.nan
        if colors is not None:
            who = [v for v in mem if colors[v, 3] != 0]
            if who:
                out_c[i] = [(2 * sum(int(colors[v, a]) for v in who) + len(who)) // (2 * len(who)) for a in range(3)] + [255]
    return dict(verts=out_v, normals=None if normals is None else out_n, colors=None if colors is None else out_c,
                tris=np.array([[rank[lead[i]] for i in tris[t]] for t in keep], np.int32).reshape(-1, 3),
                cluster=np.array([rank.get(l, -1) for l in lead], np.int32), members=np.array(members, np.int32), tri_index=np.array(keep, np.int32),
                stats=(len(clusters), degenerate, nt - degenerate - len(keep), len(clusters) - len(named)))


SMALL = {
    "triangle zoo": cases.triangle_zoo, "normals and colours": cases.normals_and_colours, "ties": cases.ties, "cell arithmetic": cases.cell_arithmetic,
    "low triangle, high vertices": cases.low_triangle_high_vertices, "reversed order": lambda: cases.reversed_order(40), "lattice ends": cases.lattice_ends,
    "below 4096": cases.below_4096, "random 257": lambda: cases.random_mesh(257, 500, 3), "random 65, few cells": lambda: cases.random_mesh(65, 300, 4, 16.0),
    "quotients 0.1": lambda: cases.quotients(np.float32(0.1)), "one cell of 300": lambda: cases.one_cell(300),
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_restatement_equals_a_plain_loop(name):
    m = SMALL[name]()
    same(rs.simplify(**m), loop_simplify(**m), name)


def test_restatement_known_answers():
    # the eight corners of a cube of vertices into one cluster, and three far vertices to hold a triangle
    corners = np.array([[x, y, z] for x in (0.25, 0.75) for y in (0.25, 0.75) for z in (0.25, 0.75)])
    v = np.concatenate([corners, [[5.5, 0.5, 0.5], [0.5, 5.5, 0.5]]])
    nrm = np.tile([[0.0, 0.0, 2.0]], (10, 1))
    col = np.tile(np.array([[10, 20, 31, 255]], np.uint8), (10, 1))
    col[0] = (11, 20, 30, 255)
    r = rs.simplify(v, [[7, 8, 9], [0, 9, 8], [1, 2, 9], [8, 9, 3]], 1.0, nrm, col)
    assert r["verts"].tolist() == [[0.5, 0.5, 0.5, 0.0], [5.5, 0.5, 0.5, 0.0], [0.5, 5.5, 0.5, 0.0]] and r["members"].tolist() == [8, 1, 1]
    assert r["tris"].tolist() == [[0, 1, 2], [0, 2, 1]] and r["tri_index"].tolist() == [0, 1] and r["cluster"].tolist() == [0] * 8 + [1, 2]
    assert r["normals"].tolist() == [[0.0, 0.0, 1.0]] * 3 and r["stats"] == (3, 1, 1, 0)
    assert r["colors"].tolist() == [[10, 20, 31, 255]] * 3                 # (2 * 81 + 8) // 16 = 10, (2 * 247 + 8) // 16 = 31
    # a strip whose cells alternate: vertices 0, 2, 4, .. in cell 0 and 1, 3, 5, .. in cell 1 of x, y = the pair's number
    n = 10
    i = np.arange(2 * n)
    v = np.stack([(i % 2) + 0.5, (i // 2) + 0.5, np.zeros(2 * n)], 1)
    t = np.arange(2 * n - 2)
    r = rs.simplify(v, np.stack([t, t + 1, t + 2], 1), 1.0)
    assert r["stats"] == (2 * n, 0, 0, 0) and np.array_equal(r["verts"][:, :3], v.astype(np.float32)) and (r["members"] == 1).all()
    r = rs.simplify(v, np.stack([t, t + 1, t + 2], 1), 2.0)                # two rows to a cell, both columns in one: every triangle collapses
    assert r["stats"] == (n // 2, 2 * n - 2, 0, n // 2) and len(r["verts"]) == 0 and (r["cluster"] == -1).all()
    # nothing in, nothing out
    r = rs.simplify(np.zeros((0, 3)), np.zeros((0, 3), np.int32), 1.0)
    assert r["stats"] == (0, 0, 0, 0) and r["verts"].shape == (0, 4)
    assert rs.simplify(np.zeros((5, 3)), np.zeros((0, 3), np.int32), 1.0)["cluster"].tolist() == [-1] * 5
    for bad, words in (([[np.nan, 0, 0]], "vertex 1 has a coordinate"), ([[4096.0, 0, 0]], "vertex 1 has a coordinate"), ([[0, 0, -4095.0]], "vertex 1 lies in cell")):
        with pytest.raises(ValueError, match=words):
            rs.simplify(np.concatenate([[[0, 0, 0]], bad, [[np.inf, 0, 0]]]), [[0, 1, 2]], 2.0 ** -9)
    with pytest.raises(ValueError, match=r"triangle 1 names vertex 3, outside \[0, 3\)"):
        rs.simplify(np.zeros((3, 3)), [[0, 1, 2], [0, 3, -1], [9, 9, 9]], 1.0)


def test_crafted_meshes_reach_what_they_are_meant_to_reach():
    C_ = cases.crafted()
    r = {k: rs.simplify(**m) for k, m in C_.items()}
    m = C_["every vertex alone"]
    assert r["every vertex alone"]["stats"][0] == len(m["verts"]) == 4097 and (r["every vertex alone"]["members"] == 1).all()
    one = r["65537 vertices in one cell"]
    assert one["stats"][0] == 3 and one["members"].tolist() == [65537, 1, 1] and one["stats"][1] == 64 and one["stats"][2] == 1 and len(one["tris"]) == 2
    assert one["colors"][0].tolist() == [255, 0, 0, 255]                  # 32768 ones among 65537, one short of a half: (65536 + 65537) // 131074 = 0
    assert rs.simplify(**cases.one_cell(300))["colors"][0].tolist() == [255, 0, 1, 255]          # 150 among 300, the tie: (300 + 300) // 600 = 1
    m = C_["cell arithmetic"]
    x = m["verts"][:, 0]
    assert (x == 0.25).any() and (x == -0.25).any() and np.signbit(x[x == 0]).any() and (x == np.nextafter(np.float32(0.5), np.float32(0))).any()
    c = rs.cells(m["verts"][:, :3], 0.25)[:, 0]
    assert c[x == np.float32(-0.25)].tolist() == [-1.0] and c[np.signbit(x) & (x == 0)].tolist() == [0.0] and c[x == np.nextafter(np.float32(-0.25), np.float32(-1))].tolist() == [-2.0]
    # Quotients next to integers.  With float32 operands the exact quotient p / cell is either an integer or at least 2^-43 of its size away
    # from one while |c| < 2^20 (cell * k - p is a multiple of ulp(cell) * 2^-24-ish steps), so the FLOAT64 division of the definition never rounds
    # across an integer: its floor is the floor of the exact quotient.  A float32 division does round across, and these cases tell the two apart.
    from fractions import Fraction
    for cell in (0.1, 0.3, 0.7):
        q = C_["quotients %g" % cell]
        k = np.arange(1, 2001)
        x = q["verts"][:, 0]
        c = rs.cells(q["verts"][:, :1], np.float32(cell))[:, 0]
        assert (c == k).any() and (c == k - 1).any(), cell
        assert c.tolist() == [math.floor(Fraction(float(p)) / Fraction(float(np.float32(cell)))) for p in x], cell
        assert (np.floor(x / np.float32(cell)) != c).any(), "a float32 division would pass"
    m = C_["lattice ends"]
    c = rs.cells(m["verts"][:, :3], m["cell"])
    assert c.min() == -2 ** 20 and c.max() == 2 ** 20 - 1
    k = rs.keys(m["verts"][:, :3], m["cell"])
    assert int(k[0]) >> 42 == 0 and int(k[1]) >> 42 == 2 ** 21 - 1 and int(k[4]) == ((2 ** 21 - 1) << 21)
    assert np.abs(C_["below 4096"]["verts"][:, :3]).max() == np.nextafter(np.float32(4096), np.float32(0)) and len(r["below 4096"]["verts"]) == 4
    m = C_["ties"]
    frac = m["verts"][:80, 0].astype(np.float64) * 2.0 ** 20
    assert (frac - np.floor(frac) == 0.5).all() and (np.floor(frac) % 2 == 0).any() and (np.floor(frac) % 2 == 1).any()
    assert sorted(r["ties"]["members"].tolist())[-2:] == [3, 7]
    big = r["ties"]["verts"][r["ties"]["members"] > 1][:, :3].astype(np.float64) * 2.0 ** 20
    assert (big != np.rint(big)).any(), "the means of the clusters of 3 and 7 are representable on the quantisation grid"
    h = C_["hash lines"]
    k = rs.keys(h["verts"][:, :3], h["cell"])
    assert r["hash lines"]["stats"][0] == len(k) == len(np.unique(k)) == 9 * 4096
    assert len(np.unique(k[:4096] & np.uint64((1 << 42) - 1))) == 1 and len(np.unique(k[2 * 4096:3 * 4096] >> np.uint64(42))) == 4096
    m = C_["reversed order"]
    k = rs.keys(m["verts"][:, :3], m["cell"])
    assert (np.diff(k[:300].astype(np.int64)) < 0).all() and r["reversed order"]["stats"][0] == 300 and (r["reversed order"]["members"] == 2).all()
    by_key = np.argsort(k[:300], kind="stable")
    assert not np.array_equal(r["reversed order"]["verts"], r["reversed order"]["verts"][by_key[: len(r["reversed order"]["verts"])]])
    low = r["low triangle, high vertices"]
    assert low["tris"].tolist() == [[6, 7, 8], [8, 7, 6], [0, 1, 2], [5, 3, 4]]
    nc = r["normals and colours"]
    assert nc["stats"] == (7, 0, 0, 0)
    n = nc["normals"]
    assert np.isnan(n[1]).all() and np.isnan(n[2]).all() and not np.isnan(n[[0, 3, 4, 5, 6]]).any()
    assert n[0].tolist() == [np.float32(np.sqrt(0.5)), 0.0, np.float32(np.sqrt(0.5))] and n[3].tolist() == [0.0, 1.0, 0.0]
    assert nc["colors"].tolist() == [[11, 21, 31, 255], [2, 3, 4, 255], [128, 128, 128, 255], [9, 9, 9, 255], [7, 8, 9, 255], [0, 0, 0, 0], [1, 2, 3, 255]]
    zoo = r["triangle zoo"]
    assert zoo["tri_index"].tolist() == [4, 7, 9] and zoo["tris"].tolist() == [[2, 3, 1], [1, 3, 2], [4, 5, 0]] and zoo["stats"] == (10, 5, 4, 4)
    assert zoo["cluster"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3] + [-1] * 8 + [4, 4, 5, 5, 0] and zoo["members"].tolist() == [3, 2, 2, 2, 2, 2]
    ends = r["duplicates at the ends"]
    assert ends["stats"][1:3] == (0, 1) and len(ends["tris"]) == 65536 and ends["tri_index"][0] == 0 and ends["tri_index"][-1] == 65535
    assert r["65536 copies"]["tris"].tolist() == [[2, 0, 1]] and r["65536 copies"]["stats"] == (4, 0, 65535, 1)


def hostlib():
    if "lib" not in _cache:
        src = os.path.join(ROOT, "tests", "hostcheck", "mesh_simplify_math_check.cpp")
        inc = os.path.join(ROOT, "elasticreconstruction_amd", "csrc")
        out = os.path.join(ROOT, "tests", "hostcheck", "_build", "libmesh_simplify_math_check.so")
        deps = [src, os.path.join(inc, "er_mesh_simplify_math.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I" + inc, src, "-o", out], check=True)
        _cache["lib"] = C.CDLL(out)
    return _cache["lib"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def edge_floats():
    big = np.float32(4096.0)
    k = np.arange(-64, 65)
    return np.concatenate([
        np.array([0.0, -0.0, np.nan, np.inf, -np.inf, big, -big, np.nextafter(big, np.float32(0)), -np.nextafter(big, np.float32(0)), 2048.0, -2048.0,
                  np.nextafter(np.float32(-2048), np.float32(-4096)), 2048.0 - 2.0 ** -9, 1e-45, -1e-45, 1.1754944e-38], np.float32),
        ((2 * k + 1) * 2.0 ** -21).astype(np.float32), (k * 0.25).astype(np.float32), np.nextafter((k * 0.25).astype(np.float32), np.float32(-np.inf)),
        (k.astype(np.float32) * np.float32(0.1)), (k.astype(np.float32) * np.float32(0.3))])


def test_host_math_equals_the_restatement():
    """er_mesh_simplify_math.h on the host, bit for bit: 1.2 million random vertices and triangles and the edge values, at five cells."""
    L = hostlib()
    rng = np.random.default_rng(21)
    e = edge_floats()
    n = 1200000
    for cell in (np.float32(0.25), np.float32(0.1), np.float32(2.0 ** -9), np.float32(3.0 * 7.5 / 512.0), np.float32(1e-4)):
        xyz = np.concatenate([rng.uniform(-3, 3, (n, 3)), rng.uniform(-4200, 4200, (n // 8, 3)), rng.choice(e, (20000, 3)),
                              np.stack([e, np.zeros_like(e), np.ones_like(e)], 1)]).astype(np.float32)
        m = len(xyz)
        off, key, q = np.zeros(m, np.int32), np.zeros(m, np.uint64), np.zeros((m, 3), np.int64)
        L.sc_vertices(C.c_long(m), _p(xyz), C.c_float(cell), _p(off), _p(key), _p(q))
        want = rs.offences(xyz, cell)
        assert np.array_equal(off, want) and (want == 1).any() and (want == 2).any() == (cell < 2.0 ** -8), cell
        ok = want == 0
        assert np.array_equal(key[ok], rs.keys(xyz[ok], cell)) and np.array_equal(q[ok], rs.quantise(xyz[ok])), cell
    # the finish of a position: sums and counts of every size, beyond 2^53 too
    m = 1000000
    members = rng.integers(1, 2 ** rng.integers(1, 31, m), m).astype(np.int64)
    S = (rng.uniform(-1, 1, (m, 3)) * members[:, None] * 2.0 ** 32).astype(np.int64)
    got = np.zeros((m, 3), np.float32)
    L.sc_positions(C.c_long(m), _p(S), _p(members), _p(got))
    want = ((S.astype(np.float64) / members.astype(np.float64)[:, None]) * 2.0 ** -20).astype(np.float32)
    assert np.array_equal(bits(got), bits(want)) and (np.abs(S) > 2 ** 53).any()
    # normals
    nr = np.concatenate([rng.normal(size=(m, 3)), rng.choice(e, (20000, 3))]).astype(np.float32)
    c = np.zeros(len(nr), np.int32)
    L.sc_contributes(C.c_long(len(nr)), _p(nr), _p(c))
    with np.errstate(all="ignore"):
        assert np.array_equal(c != 0, (np.abs(nr) < rs.LIMIT).all(axis=1))
    N = (rng.normal(size=(m, 3)) * 2.0 ** rng.integers(0, 62, (m, 1))).clip(-2.0 ** 62, 2.0 ** 62).astype(np.int64)
    N[:1000] = 0
    N[1000:2000, 1:] = 0
    count = rng.integers(0, 5, m).astype(np.int64)
    got = np.zeros((m, 3), np.float32)
    L.sc_normals(C.c_long(m), _p(N), _p(count), _p(got))
    want = rs.finish_normal(N, count)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want[:1000]).all() and np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)])
    # colours: every tie at one half among them
    mm = rng.integers(1, 70000, m).astype(np.int64)
    sums = np.minimum(rng.integers(0, 256, m) * mm + rng.integers(-3, 4, m), 255 * mm).clip(0)
    sums[::7] = (2 * rng.integers(0, 255, len(sums[::7])) + 1) * (mm[::7] // 2 * 2) // 2
    mm[::7] = mm[::7] // 2 * 2 + (mm[::7] < 2) * 2
    sums = np.minimum(sums, 255 * mm)
    got = np.zeros(m, np.uint32)
    L.sc_channels(C.c_long(m), _p(sums), _p(mm), _p(got))
    assert np.array_equal(got, (2 * sums + mm) // (2 * mm)) and got.max() <= 255 and ((2 * sums) % (2 * mm) == mm).any()
    # rotations
    T = np.stack([rng.permutation(5)[:3] for _ in range(1000)]).astype(np.int32) + rng.integers(0, 2 ** 31 - 6, (1000, 1)).astype(np.int32)
    T = np.concatenate([T, rng.integers(0, 2 ** 31 - 1, (m, 3)).astype(np.int32)])
    T = T[(T[:, 0] != T[:, 1]) & (T[:, 1] != T[:, 2]) & (T[:, 0] != T[:, 2])]
    got = np.zeros_like(T)
    L.sc_rotations(C.c_long(len(T)), _p(T), _p(got))
    assert np.array_equal(got, rs.canonical(T)) and (got[:, 0] == T.min(axis=1)).all()


def test_new_symbols_are_in_the_header_the_binding_and_the_library():
    hdr = open(os.path.join(ROOT, "include", "er_hip.h")).read()
    L = _ffi.lib()
    for sym in ("er_mesh_simplify", "er_tsdf_extract_mesh_simplified"):
        assert re.search(r"\bint %s\(" % sym, hdr) and sym in _ffi.SYMBOLS and hasattr(L, sym), sym
    from elasticreconstruction_amd import mesh
    from elasticreconstruction_amd.tsdf import TSDFVolume
    assert callable(mesh.simplify) and callable(TSDFVolume.extract_simplified_mesh)
    import inspect
    assert "cell" in inspect.signature(TSDFVolume.SaveMesh).parameters


def test_refusals_that_need_no_device():
    L = _ffi.lib()
    err = lambda: L.er_last_error().decode()
    v = np.zeros((3, 4), np.float32)
    tri = np.array([[0, 1, 2]], np.int32)
    out = np.full((3, 4), -7, np.float32)
    nv, nt = C.c_long(-7), C.c_long(-7)
    p = lambda a: None if a is None else _ffi.ptr(a)

    def call(vv=v, nn=None, cc=None, n=3, tt=tri, m=1, cell=1.0, no=None, co=None, pv=C.byref(nv), pt=C.byref(nt)):
        return L.er_mesh_simplify(p(vv), p(nn), p(cc), n, p(tt), m, C.c_float(cell), 0, p(out), p(no), p(co), None, 3, None, None, 0, None, pv, pt, None, None)

    assert call(pv=None) != 0 and err() == "er_mesh_simplify: NULL argument"
    assert call(pt=None) != 0 and err() == "er_mesh_simplify: NULL argument"
    assert call(vv=None) != 0 and err() == "er_mesh_simplify: NULL argument"
    assert call(tt=None) != 0 and err() == "er_mesh_simplify: NULL argument"
    assert call(no=out) != 0 and "without the input" in err()
    assert call(co=np.zeros((3, 4), np.uint8)) != 0 and "without the input" in err()
    assert call(n=-3) != 0 and "-3 vertices" in err()
    assert call(m=-1) != 0 and "-1 triangles" in err()
    assert call(n=2 ** 31) != 0 and "2^31 - 1" in err()
    assert call(m=2 ** 31) != 0 and "2^31 - 1" in err()
    fake = C.cast(_NOT_A_HANDLE, C.c_void_p)                 # never dereferenced: every call with it is refused before the handle is looked at
    ts = lambda h, cell, mt, pv, pt, colors=None, want=0: L.er_tsdf_extract_mesh_simplified(h, C.c_float(cell), mt, 0, want, None, None, p(colors), None, 0, None, 0,
                                                                                             pv, pt, None, None, None)
    assert ts(None, 0.01, 0, C.byref(nv), C.byref(nt)) != 0 and err() == "er_tsdf_extract_mesh_simplified: NULL argument"
    assert ts(fake, 0.01, 0, None, C.byref(nt)) != 0 and err() == "er_tsdf_extract_mesh_simplified: NULL argument"
    assert ts(fake, 0.01, 0, C.byref(nv), None) != 0 and err() == "er_tsdf_extract_mesh_simplified: NULL argument"
    assert ts(fake, 0.01, -1, C.byref(nv), C.byref(nt)) != 0 and err() == "er_tsdf_extract_mesh_simplified: min_triangles = -1"
    assert ts(fake, 0.01, 0, C.byref(nv), C.byref(nt), np.zeros((3, 4), np.uint8)) != 0 and "without want_colors" in err()
    if L.er_device_count() <= 0:
        assert call() != 0 and err() == "er_mesh_simplify: no HIP device available (liber_hip has no CPU fallback)"
        assert ts(fake, 0.01, 0, C.byref(nv), C.byref(nt)) != 0
        assert err() == "er_tsdf_extract_mesh_simplified: no HIP device available (liber_hip has no CPU fallback)"
    else:
        for cell in (0.0, -1.0, float("nan"), float("inf")):
            assert call(cell=cell) != 0 and "it has to be finite and above 0" in err(), cell
            assert ts(fake, cell, 0, C.byref(nv), C.byref(nt)) != 0 and "it has to be finite and above 0" in err(), cell
    assert (nv.value, nt.value) == (-7, -7) and (out == -7).all()


def test_programs_name_the_new_flags_on_their_command_lines():
    bin_ = os.path.join(ROOT, "elasticreconstruction_amd", "bin")
    r = subprocess.run([os.path.join(bin_, "MeshOutput"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--cell" in r.stdout and "--min_triangles" in r.stdout, r.stdout
    r = subprocess.run([os.path.join(bin_, "Integrate"), "--help"], capture_output=True, text=True, timeout=60)
    assert "--mesh_cell" in r.stdout + r.stderr and "--mesh_min_triangles" in r.stdout + r.stderr
    for bad in ("-1", "nan", "abc"):
        r = subprocess.run([os.path.join(bin_, "MeshOutput"), os.path.join(ROOT, "README.md"), "--cell", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--cell" in r.stderr, (bad, r.stderr)
