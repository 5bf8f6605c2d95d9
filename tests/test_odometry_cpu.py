"""Depth odometry without a GPU: the C ABI and its refusals, csrc/er_odom_math.h compiled for the host against the numpy
restatement (tests/odometry_restatement.py) bit for bit, the weight tables, and the restatement itself against known answers and against the
ground truth of rendered frames.  Nothing here is checked against PCL: the reference tree does not contain KinFu.

The restatement against ground truth, measured on the CPU (frames 0 .. 3 of synth.kinfu_camera_path(0, 4, 50), 1.83 .. 1.93 degrees and
3.07 mm of motion per pair; worst of the three pairs):
    160 x 120: rotation error 0.10074 deg, translation error 0.5246 mm   (17761 .. 17810 matches at level 0, 988 .. 1004 at level 2)
     72 x  52: rotation error 0.05349 deg, translation error 1.2371 mm   ( 3381 ..  3416 matches at level 0, 164 ..  177 at level 2)
The bars below are twice these values: a regression guard on the restatement, not a claim about the method.  (The bilateral filter and the
millimetre quantisation of the rendered depth cost accuracy: a float64 prototype without the filter stayed below 0.015 / 0.044 deg.)

The last section checks, on the restatement, that every fixture of tests/test_odometry_shapes_gpu.py sits on the edge it is meant for, and runs
the new images (and the two borders that the device's own maps can never reach: a valid model record in the last column, and the entry
after the end of the depth-weight table) through the host build of the header."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import odometry_restatement as orr
import odometry_cases as oc
from odometry_cases import same_bits, scaled_cam, scene, seeded_image
from elasticreconstruction_amd import _ffi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ODOM_SYMBOLS = ["er_odom_align_pairs", "er_odom_create", "er_odom_destroy", "er_odom_linearize", "er_odom_params_default", "er_odom_read_maps",
                "er_odom_tables", "er_odom_track"]
# measured (see the module docstring): (rotation error in degrees, translation error in metres), worst pair
MEASURED = {(160, 120): (0.10074, 0.5246e-3), (72, 52): (0.05349, 1.2371e-3)}
_cache = {}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def hostlib():
    if "lib" not in _cache:
        src = os.path.join(ROOT, "tests", "hostcheck", "odom_math_check.cpp")
        inc = os.path.join(ROOT, "elasticreconstruction_amd", "csrc")
        out = os.path.join(ROOT, "tests", "hostcheck", "_build", "libodom_math_check.so")
        deps = [src, os.path.join(inc, "er_odom_math.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I" + inc, src, "-o", out], check=True)
        _cache["lib"] = C.CDLL(out)
    return _cache["lib"]


def host_records(depth, K):
    rows, cols = depth.shape
    rec = np.zeros((rows * cols, 2, 4), F)
    cam = np.array(K, F)
    hostlib().od_maps(_p(np.ascontiguousarray(depth)), cols, rows, _p(cam), _p(rec))
    return rec


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_odometry_symbols():
    txt = open(os.path.join(ROOT, "include", "er_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    header = sorted(s for s in set(re.findall(r"\b(er_[a-z0-9_]+)\s*\(", txt)) if s.startswith("er_odom_"))
    assert header == ODOM_SYMBOLS
    assert sorted(s for s in _ffi.SYMBOLS if s.startswith("er_odom_")) == ODOM_SYMBOLS
    L = _ffi.lib()
    assert not [s for s in ODOM_SYMBOLS if not hasattr(L, s)]
    import elasticreconstruction_amd as pkg
    assert pkg.DepthOdometry is not None and pkg.accumulate is not None


def test_constructor_and_program_refuse_without_a_gpu_and_write_nothing(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from elasticreconstruction_amd import DepthOdometry
    with pytest.raises(_ffi.ErError, match="no HIP device"):
        DepthOdometry(160, 120, scaled_cam(160))
    d = str(tmp_path)
    np.zeros((3, 120 * 160), np.uint16).tofile(os.path.join(d, "frames.raw"))
    exe = os.path.join(ROOT, "elasticreconstruction_amd", "bin", "DepthOdometry")
    r = subprocess.run([exe, "--cols", "160", "--rows", "120", "--depth_raw", "frames.raw", "--traj_log", "traj.log"], cwd=d, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
    assert sorted(os.listdir(d)) == ["frames.raw"]


def test_default_parameters():
    from elasticreconstruction_amd import odometry
    p = odometry.default_params()
    assert p["levels"] == 3 and p["iterations"][:3] == (10, 5, 4) and p["bilateral"] == 1 and p["max_depth_mm"] == 0
    assert p["dist_thresh"] == F(0.10) and p["angle_thresh"] == F(math.sin(math.radians(20.0)))
    for k, v in orr.DEFAULTS.items():
        assert p[k] == v, k


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------
def test_tables_are_within_one_float32_ulp_of_float64_exp():
    from elasticreconstruction_amd import odometry
    space, dw = odometry.tables()
    assert space.shape == (73,) and 300 < len(dw) <= 512
    es = np.exp(-np.arange(73, dtype=np.float64) / (2.0 * 4.5 * 4.5))
    ed = np.exp(-np.arange(len(dw), dtype=np.float64) ** 2 / (2.0 * 30.0 * 30.0))
    for got, want in ((space, es), (dw, ed)):
        assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(want.astype(F)).astype(np.float64))
    # the end of the depth table: every product of two weights is a normal float32, and the next entry's would not be
    tiny = float(np.finfo(F).tiny)
    assert float(dw[-1]) * float(space[72]) >= tiny
    assert math.exp(-len(dw) ** 2 / 1800.0) * float(space[72]) < tiny
    hs, hd = np.zeros(73, F), np.zeros(512, F)
    n = hostlib().od_tables(_p(hs), _p(hd))
    assert n == len(dw) and np.array_equal(hs, space) and np.array_equal(hd[:n], dw) and not hd[n:].any()
    rs, rd = orr.tables()
    assert len(rd) == len(dw) and np.all(np.abs(rs.astype(np.float64) - es) <= np.spacing(es.astype(F)))


# ---- er_odom_math.h on the host against the restatement, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("cols,rows,seed", [(72, 52, 1), (40, 30, 2), (14, 6, 3)])
def test_host_bilateral_and_pyramid_equal_the_restatement(cols, rows, seed):
    img = seeded_image(cols, rows, seed)
    space, dw = orr.tables()
    out = np.zeros_like(img)
    hostlib().od_bilateral(_p(img), cols, rows, _p(space), _p(dw), len(dw), _p(out))
    want = orr.bilateral(img, space, dw)
    assert np.array_equal(out, want)
    assert np.array_equal(out == 0, img == 0) and (out != img).any()
    for src in (img, want):
        half = np.zeros((rows // 2, cols // 2), np.uint16)
        hostlib().od_pyr_down(_p(np.ascontiguousarray(src)), cols, rows, _p(half))
        assert np.array_equal(half, orr.pyr_down(src))


@pytest.mark.parametrize("cols,rows,seed", [(72, 52, 4), (18, 13, 5)])
def test_host_vertex_and_normal_maps_equal_the_restatement(cols, rows, seed):
    img = seeded_image(cols, rows, seed)
    for K in (scaled_cam(cols), (F(61.7), F(59.3), F(cols / 2 - 0.25), F(rows / 2 + 0.125))):
        rec = host_records(img, K)
        V, N = orr.vertex_map(img, K), orr.normal_map(img, K)
        assert same_bits(rec[:, 0, :3], V.reshape(-1, 3)) and same_bits(rec[:, 1, :3], N.reshape(-1, 3))
        assert np.isnan(N[-1]).all() and np.isnan(N[:, -1]).all() and np.isnan(V[img == 0]).all() and np.isfinite(N).any()


def _poses():
    P = synth.perturbation(3, 3.0, 0.03)
    far = np.eye(4)
    far[:3, :3] = orr.rotation(0.0, 0.9, 0.0)                  # most projections leave the image
    behind = np.eye(4)
    behind[2, 3] = -5.0                                        # vg.z <= 0
    huge = np.eye(4)
    huge[0, 3] = 1e30                                          # a projection far outside int range: must be refused in float
    nan = np.eye(4)
    nan[1, 3] = np.nan
    return [np.eye(4), P, far, behind, huge, nan]


@pytest.mark.parametrize("cols,rows", [(72, 52), (36, 26)])
def test_host_match_rows_and_products_equal_the_restatement(cols, rows):
    d, W, cam = scene(72, 52)
    level = 0 if cols == 72 else 1
    od = orr.Odometry(72, 52, cam)
    model, cur = od.maps(d[0]), od.maps(d[1])
    K = np.array(od.K(level), F)
    recm, recc = host_records(model[level][0], K), host_records(cur[level][0], K)
    npix = cols * rows
    seen = 0
    for T in _poses():
        R, t = np.ascontiguousarray(T[:3, :3], F), np.ascontiguousarray(T[:3, 3], F)
        ok, a, b, prod = np.zeros(npix, np.uint8), np.zeros((npix, 6), F), np.zeros(npix, F), np.zeros((npix, 27), np.float64)
        hostlib().od_rows.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float] + [C.c_void_p] * 4
        cnt = hostlib().od_rows(_p(R), _p(t), _p(recc), _p(recm), cols, rows, _p(K), od.p["dist_thresh"], od.p["angle_thresh"], _p(ok), _p(a), _p(b), _p(prod))
        ra, rb, rok = od.rows_of(model, cur, level, T, mask=True)
        assert np.array_equal(ok.astype(bool), rok) and cnt == rok.sum()
        assert np.array_equal(a[rok].view(np.uint32), ra.view(np.uint32)) and np.array_equal(b[rok].view(np.uint32), rb.view(np.uint32))
        a64, b64 = ra.astype(np.float64), rb.astype(np.float64)
        terms = np.stack([a64[:, i] * a64[:, j] for i, j in orr.PAIRS] + [a64[:, i] * b64 for i in range(6)], 1) if cnt else np.zeros((0, 27))
        assert np.array_equal(prod[rok], terms)
        seen += cnt
    assert seen > npix                                          # identity and the perturbation match most of the image; the last three nothing
    assert cnt == 0


# ---- the restatement against known answers ------------------------------------------------------------------------------------------------------
def test_constant_image_is_a_fixed_point_of_filter_and_pyramid():
    space, dw = orr.tables()
    for value in (1, 437, 1000, 65535):
        img = np.full((26, 36), value, np.uint16)
        assert np.array_equal(orr.bilateral(img, space, dw), img)
        assert np.array_equal(orr.pyr_down(img), img[::2, ::2])
    z = np.zeros((26, 36), np.uint16)
    assert not orr.bilateral(z, space, dw).any() and not orr.pyr_down(z).any()


def test_pyramid_mean_truncates_and_ignores_far_and_outside_taps():
    img = np.full((6, 6), 1000, np.uint16)
    img[0, 0:3] = 1001
    img[1, 0:2] = 1001                                        # window of (0, 0): the 9 taps inside the image, 5 x 1001 + 4 x 1000 = 9005
    assert orr.pyr_down(img)[0, 0] == 1000                    # 9005 / 9 = 1000.56: truncated, not rounded
    img2 = np.full((10, 10), 1000, np.uint16)
    img2[4, 5] = 1089                                         # |tap - centre| = 89 < 90 counts ...
    img2[5, 4] = 1090                                         # ... 90 does not
    assert orr.pyr_down(img2)[2, 2] == (23 * 1000 + 1089) // 24
    img2[4, 4] = 0
    assert orr.pyr_down(img2)[2, 2] == 0                      # a centre of 0 gives 0


def test_tilted_plane_gives_its_normal_to_float32_accuracy():
    cols, rows = 72, 52
    fx, fy, cx, cy = scaled_cam(cols)
    n = np.array([0.3, -0.2, -1.0])
    n /= np.linalg.norm(n)
    u, v = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    z = (n @ np.array([0.0, 0.0, 1.5])) / (ray @ n)            # the plane through (0, 0, 1.5)
    V = (ray * z[..., None]).astype(F)
    N = orr.normals_of(V)[:-1, :-1].astype(np.float64)
    # cross(a, b) of two steps along the surface: each float32 vertex is off by at most 2^-24 |v| per coordinate; the shortest step is `spacing`
    spacing = min(np.linalg.norm(V[:-1, 1:] - V[:-1, :-1], axis=-1).min(), np.linalg.norm(V[1:, :-1] - V[:-1, :-1], axis=-1).min())
    bound = 8.0 * 2.0 ** -24 * np.abs(V).max() / spacing
    sign = np.sign(N[0, 0] @ n)
    assert np.abs(N - sign * n).max() <= bound, (np.abs(N - sign * n).max(), bound)
    assert bound < 1e-4


def test_identical_frames_give_the_identity_at_the_first_iteration():
    d, W, cam = scene(72, 52)
    od = orr.Odometry(72, 52, cam)
    m = od.maps(d[0])
    T, lost, trace = od.align_maps(m, m)
    assert not lost and np.array_equal(trace[0][0], np.eye(4)) and np.array_equal(T, np.eye(4))
    assert trace[0][1] == int((np.isfinite(m[2][1]).all(-1) & np.isfinite(m[2][2]).all(-1)).sum())     # every valid pixel matches itself
    zero = od.maps(np.zeros_like(d[0]))
    T, lost, trace = od.align_maps(zero, m)
    assert lost and np.array_equal(T, np.eye(4)) and all(c == 0 for _, c in trace)


# ---- the restatement against ground truth -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,rows", [(160, 120), (72, 52)])
def test_restatement_recovers_every_relative_pose(cols, rows):
    d, W, cam = scene(cols, rows)
    od = orr.Odometry(cols, rows, cam)
    T_rel, lost = od.track(d)
    assert not lost.any()
    worst_r = worst_t = 0.0
    for i in range(3):
        G = np.linalg.inv(W[i]) @ W[i + 1]
        er, et = orr.pose_error(T_rel[i], G)
        motion = orr.pose_error(np.eye(4), G)
        print("%d x %d pair %d: rotation error %.5f deg, translation error %.4f mm (motion %.3f deg, %.3f mm)" % (cols, rows, i, er, et * 1e3, motion[0], motion[1] * 1e3))
        worst_r, worst_t = max(worst_r, er), max(worst_t, et)
    bar_r, bar_t = (2.0 * x for x in MEASURED[(cols, rows)])
    assert worst_r <= bar_r and worst_t <= bar_t, (worst_r, worst_t)


# ---- the fixtures of tests/test_odometry_shapes_gpu.py: each sits where it claims to -------------------------------------------------------------
def _library_tables():
    from elasticreconstruction_amd import odometry
    return odometry.tables()


def _edge_images(cols, rows):
    n = len(_library_tables()[1])
    return [("table end", oc.table_end_image(cols, rows, n)), ("extreme", oc.extreme_image(cols, rows, 11))]


@pytest.mark.parametrize("cols,rows", [(72, 52), (41, 25)])
def test_host_filter_pyramid_and_maps_equal_the_restatement_on_the_edge_images(cols, rows):
    space, dw = _library_tables()
    n = len(dw)
    for name, img in _edge_images(cols, rows):
        out = np.zeros_like(img)
        hostlib().od_bilateral(_p(img), cols, rows, _p(space), _p(dw), n, _p(out))
        want = orr.bilateral(img, space, dw)
        assert np.array_equal(out, want), name
        assert np.array_equal(out == 0, img == 0), name
        if cols % 2 == 0:
            half = np.zeros((rows // 2, cols // 2), np.uint16)
            hostlib().od_pyr_down(_p(np.ascontiguousarray(want)), cols, rows, _p(half))
            assert np.array_equal(half, orr.pyr_down(want)), name
        K = scaled_cam(cols)
        rec = host_records(want, K)
        assert same_bits(rec[:, 0, :3], orr.vertex_map(want, K).reshape(-1, 3)) and same_bits(rec[:, 1, :3], orr.normal_map(want, K).reshape(-1, 3)), name


def test_table_end_image_holds_the_last_entry_of_the_table_at_the_window_corner_and_on_every_border():
    space, dw = _library_tables()
    n, c = len(dw), 1000
    tiny = np.finfo(F).tiny
    assert float(dw[n - 1]) * float(space[72]) >= tiny > 0 and F(dw[n - 1] * space[72]) >= tiny             # the smallest weight is a normal float32
    for cols, rows in ((72, 52), (41, 25)):
        img = oc.table_end_image(cols, rows, n, c).astype(np.int64)
        assert sorted(set(np.unique(img - c))) == [-(n - 1), 0, n - 2, n - 1, n]
        ys, xs = np.nonzero(img != c)
        assert len(xs) == 12 and xs.min() == 0 and ys.min() == 0 and xs.max() == cols - 1 and ys.max() == rows - 1
        for px, py in oc.table_end_probes(cols, rows):
            assert img[py, px] == c
            got = {(dx, dy): img[py + dy, px + dx] - c for (dx, dy), _, _ in oc.TABLE_END_TAPS}
            assert got[(6, 6)] == n - 1 and got[(-6, 6)] == -(n - 1) and got[(-6, -6)] == n and got[(6, -5)] == n - 2
        # at 72 x 52 every tap is alone in its own window (at 41 x 25 the three groups' windows overlap)
        for x, y in zip(xs, ys):
            win = img[max(y - 6, 0):y + 7, max(x - 6, 0):x + 7]
            assert cols < 72 or (win != c).sum() == 1, (x, y)


def test_the_entry_after_the_end_of_the_table_is_never_read():
    """`delta >= n_depth_w` skips the tap.  The device's table is zero beyond its end, so reading entry n there would add a weight of +0 and
    change no bit: only a host run with a table that is NOT zero beyond its end can tell `>=` from `>`."""
    space, dw = _library_tables()
    n = len(dw)
    poisoned = np.concatenate([dw, np.ones(8, F)])
    for cols, rows in ((72, 52), (41, 25)):
        img = oc.table_end_image(cols, rows, n)
        out = np.zeros_like(img)
        hostlib().od_bilateral(_p(img), cols, rows, _p(space), _p(poisoned), n, _p(out))
        assert np.array_equal(out, orr.bilateral(img, space, dw))
        bad = orr.bilateral(img, space, poisoned[:n + 1])
        assert not np.array_equal(bad, out)                  # a filter that did read entry n would give another image


def test_extreme_image_holds_both_ends_of_uint16_and_the_int16_sign_bit():
    space, dw = _library_tables()
    for cols, rows in ((72, 52), (41, 25)):
        img = oc.extreme_image(cols, rows, 11)
        vals = set(np.unique(img).tolist())
        assert {0, 1, 2, 32767, 32768, 65535} <= vals
        smooth = img[:, cols // 2:]
        assert (smooth[smooth > 0] > 60000).all() and (smooth > 0).sum() > rows * cols // 3
        y, x = rows // 3 + 7, cols // 4
        patch = img[y:y + 3, x:x + 9]
        assert patch.max() <= 3 and (patch > 0).sum() >= 20 and not img[y - 1, x:x + 9].any()      # 1 .. 3 against the hole above
        out = orr.bilateral(img, space, dw)
        changed = (out != img) & (img > 60000)
        assert changed.sum() > 100 and out.max() <= 65535 and (out[img > 60000] > 60000).all()      # the filter does average large values
        assert (img.astype(np.int16) < 0).sum() > rows * cols // 3                                 # what a device int16 frame shows


@pytest.mark.parametrize("cols,rows,params", oc.ALIGNABLE, ids=lambda v: str(v))
def test_restatement_aligns_every_shape_of_the_table_and_the_system_is_well_conditioned(cols, rows, params):
    d, W, cam = scene(cols, rows)
    od = orr.Odometry(cols, rows, cam, **params)
    m0, m1 = od.maps(d[0]), od.maps(d[1])
    T, lost, trace = od.align_maps(m0, m1)
    assert not lost and min(c for _, c in trace) >= od.p["min_valid"]
    for level in range(od.levels):
        s, c = od.linearize(m0, m1, level, np.eye(4))
        A = np.zeros((6, 6))
        for k, (i, j) in enumerate(orr.PAIRS):
            A[i, j] = A[j, i] = s[k]
        cond = np.linalg.cond(A)
        print("%d x %d level %d: %d matches, condition number %.3g" % (cols, rows, level, c, cond))
        assert 6e1 <= cond <= 3e2, (level, cond)
    if (cols, rows) == (80, 56):
        assert min(c for _, c in trace) == 46 and trace[0][1] == 46                # below the default min_valid of 50: why this size sets 10


def test_shapes_have_the_pixel_counts_the_launch_geometry_needs():
    px = {(c, r): [(c >> l) * (r >> l) for l in range(p["levels"])] for c, r, p in oc.SHAPES}
    assert px[(32, 32)] == [1024] and px[(41, 25)] == [1025] and px[(128, 64)] == [8 * 1024] and px[(129, 64)] == [8 * 1024 + 64]
    assert px[(96, 64)] == [6144, 1536, 384, 96] and px[(80, 56)] == [4480, 1120, 280, 70] and px[(40, 26)] == [1040, 260] and px[(70, 50)] == [3500, 875]
    assert px[(16, 12)] == [192] and px[(5, 3)] == [15] and px[(1, 1)] == [1]
    # the restatement at the two sizes below one wave: no pixel of 1 x 1 has a normal; 5 x 3 has a few
    for cols, rows, want in ((1, 1, 0), (5, 3, 4)):
        d, W, cam = scene(cols, rows)
        od = orr.Odometry(cols, rows, cam, levels=1)
        s, c = od.linearize(od.maps(d[0]), od.maps(d[1]), 0, np.eye(4))
        assert c == want and (c > 0 or not s.any())


@pytest.mark.parametrize("cols,rows", [(72, 52), (160, 120)])
def test_a_comb_pair_is_lost_part_way_and_keeps_its_last_good_pose(cols, rows):
    d, W, cam = scene(cols, rows)
    od = orr.Odometry(cols, rows, cam)
    full, cb = od.maps(d[0]), od.maps(oc.comb(d[1]))
    assert not np.isfinite(cb[0][2]).any() and not np.isfinite(cb[1][2]).any() and np.isfinite(cb[2][2]).any()      # normals: level 2 only
    whole = od.maps(d[1])                                     # level 2 of the comb is as dense as level 2 of the frame it was cut from
    assert np.array_equal(cb[2][0] > 0, whole[2][0] > 0) and np.array_equal(np.isfinite(cb[2][2]), np.isfinite(whole[2][2]))
    first = [176] * 4 if (cols, rows) == (72, 52) else [934, 982, 982, 982]
    for model, cur in ((full, cb), (cb, full)):               # the comb in either role
        T, lost, trace = od.align_maps(model, cur)
        counts = [c for _, c in trace]
        k = counts.index(0)
        assert lost and len(trace) == 19 and 1 <= k < len(trace) - 1 and k == 4
        assert min(counts[:k]) >= 2 * od.p["min_valid"] and not any(counts[k:])
        assert all(np.array_equal(P, trace[k - 1][0]) for P, _ in trace[k:]) and np.array_equal(T, trace[k - 1][0])
        assert 0.02 <= np.abs(T - np.eye(4)).max() <= 0.035
        assert counts[:4] == first


@pytest.mark.parametrize("cols,rows,params", [(72, 52, {}), (129, 64, dict(levels=1))], ids=["72x52", "129x64"])
def test_border_poses_push_the_stated_fraction_of_pixels_through_the_stated_border(cols, rows, params):
    d, W, cam = scene(cols, rows)
    od = orr.Odometry(cols, rows, cam, **params)
    m0, m1 = od.maps(d[0]), od.maps(d[1])
    poses = oc.border_poses()
    neg_zero = on_last = 0
    for level in range(od.levels):
        c, r = cols >> level, rows >> level
        _, _, ok0 = od.rows_of(m0, m1, level, np.eye(4), mask=True)
        for name, (T, border) in poses.items():
            _, _, ok = od.rows_of(m0, m1, level, T, mask=True)
            valid, gz, pu, pv = oc.projection(m1[level][1], od.K(level), T)
            with np.errstate(all="ignore"):
                front = valid & (gz > 0)
                out = dict(left=front & (pu < -0.5), right=front & (pu > c - 0.5), top=front & (pv < -0.5), bottom=front & (pv > r - 0.5))
                frac = {k: v.sum() / valid.sum() for k, v in out.items()}
                behind = (valid & (gz <= 0)).sum() / valid.sum()
                if np.isfinite(T).all():
                    neg_zero += (front & (((pu > -0.45) & (pu < -0.05)) | ((pv > -0.45) & (pv < -0.05)))).sum()      # rounds to -0.0
                    on_last += (front & ((np.abs(pu - (c - 1)) < 0.45) & (pv > 0) & (pv < r - 1))).sum()             # rounds to cols - 1
            if border:
                assert 0.25 <= frac[border] <= 0.75, (level, name, frac)
                assert all(v < 0.01 for k, v in frac.items() if k != border) and behind == 0, (level, name, frac)
                assert 0 < ok.sum() < ok0.sum() and not (ok & out[border]).any(), (level, name)
            elif name == "-z":
                assert 0.05 <= behind < 1.0 and not (ok & valid & ~front).any(), (level, behind)
            elif name == "turn":
                # (scaled_cam puts the optical axis half a pixel to a pixel off the centre of 72 x 52 and 16 rows below that of 129 x 64, so here
                # and on the device the turn is about the principal point and some pixels leave; the device's count is held to the
                # restatement's all the same, and the turn about the exact image centre is the host test below)
                assert ok.sum() > 0, level
            else:
                assert ok.sum() == 0, (level, name)
    assert neg_zero >= 10 and on_last >= 100


def test_host_match_accepts_exactly_the_last_column_and_row_and_minus_zero():
    """The device's own model maps have no normal in the last column and the last row, so `pu <= cols - 1` and `pu < cols - 1` select the
    same pixels there.  The header's statement is the wider one; it is pinned here, on the host, with a model whose last column and row are valid
    records, under the 180 degree turn that sends pixel (u, v) to (cols - 1 - u, rows - 1 - v) and so column 0 onto column cols - 1."""
    cols, rows = 72, 52
    d, W, cam = scene(cols, rows)
    cam = (cam[0], cam[1], F((cols - 1) / 2.0), F((rows - 1) / 2.0))          # the optical axis through the image centre
    od = orr.Odometry(cols, rows, cam, dist_thresh=10.0, angle_thresh=2.0)
    model, cur = od.maps(d[0]), od.maps(d[0])
    dm, Vm, Nm = model[0]
    Nm = Nm.copy()
    Nm[:, -1], Nm[-1, :] = Nm[:, -2], Nm[-2, :]                               # what a ray-cast model map could hold
    Nm[-1, -1] = Nm[-2, -2]
    model = [(dm, Vm, Nm)] + model[1:]
    K = np.array(od.K(0), F)
    recm, recc = host_records(dm, K), host_records(cur[0][0], K)
    recm[:, 1, :3] = Nm.reshape(-1, 3)
    npix, neg_zero = cols * rows, 0
    hostlib().od_rows.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float] + [C.c_void_p] * 4
    for name in ("turn", "-x", "-y"):
        T = oc.border_poses()[name][0]
        R, t = np.ascontiguousarray(T[:3, :3], F), np.ascontiguousarray(T[:3, 3], F)
        ok, a, b, prod = np.zeros(npix, np.uint8), np.zeros((npix, 6), F), np.zeros(npix, F), np.zeros((npix, 27), np.float64)
        cnt = hostlib().od_rows(_p(R), _p(t), _p(recc), _p(recm), cols, rows, _p(K), od.p["dist_thresh"], od.p["angle_thresh"], _p(ok), _p(a), _p(b), _p(prod))
        ra, rb, rok = od.rows_of(model, cur, 0, T, mask=True)
        assert cnt == rok.sum() and np.array_equal(ok.astype(bool), rok), name
        assert np.array_equal(a[rok].view(np.uint32), ra.view(np.uint32)) and np.array_equal(b[rok].view(np.uint32), rb.view(np.uint32)), name
        grid = rok.reshape(rows, cols)
        if name == "turn":
            assert grid[1:-1, 0].sum() > rows // 2 and grid[0, 1:-1].sum() > cols // 2         # matched ON the last column and ON the last row
        else:
            valid, gz, pu, pv = oc.projection(cur[0][1], K, T)
            neg_zero += (rok & (((pu > -0.45) & (pu < -0.05)) | ((pv > -0.45) & (pv < -0.05)))).sum()
    assert neg_zero >= 3                                                                      # rint gives -0.0, and -0.0 >= 0 matches
