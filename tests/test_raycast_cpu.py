"""The ray caster without a GPU: csrc/er_raycast_math.h compiled for the host against the numpy restatement
(tests/raycast_restatement.py) bit for bit -- marched plainly and with the kernel's empty-space skip --, the restatement against analytic
surfaces and against the renderer on the integrated scene, and the refusals of the C ABI.  Nothing here is checked against PCL: the reference
tree has no ray caster.

The restatement on the integrated scene (4 frames of synth.render_depth at 160 x 120 into the CPU TSDF oracle, ray-cast from the pose of
frame 1 and compared with the rendered depth of frame 1, pixels at least 3 pixels from a depth step of 30 mm or a hole), measured on the CPU:
    median |1000 vertex.z - rendered| = 0.3542 mm, 99th percentile = 2.873 mm   (13416 pixels compared; one voxel is 5.86 mm)
The bars are twice these values: the margin covers voxelisation by a moving camera.  The same figures are in profiles/raycast.txt.
(99.9 % of the view is hit.  The scene is moved off the unit lattice and integrated up to 4 m: tests/raycast_cases.py says why.)

On the analytic surfaces (rays at less than 60 degrees from the normal, two pixels from a silhouette), measured: plane, 12967 rays, hit distance
off by at most 0.00022 mm and the normal by 3.7e-7; sphere (step of one voxel, tests/raycast_cases.py says why), 7320 rays, 0.041 mm and 4.8e-5.
The bars: 0.05 mm and 1e-3."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import raycast_cases as rcc
import raycast_restatement as rcr
from odometry_cases import same_bits
from elasticreconstruction_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MEASURED_SCENE_MM = (0.3542, 2.873)                # median, 99th percentile (module docstring)
_cache = {}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def hostlib():
    if "lib" not in _cache:
        src = os.path.join(ROOT, "tests", "hostcheck", "raycast_math_check.cpp")
        inc = os.path.join(ROOT, "elasticreconstruction_amd", "csrc")
        out = os.path.join(ROOT, "tests", "hostcheck", "_build", "libraycast_math_check.so")
        deps = [src, os.path.join(inc, "er_raycast_math.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I" + inc, src, "-o", out], check=True)
        L = C.CDLL(out)
        L.rc_raycast.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                 C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        L.rc_count_steps.argtypes = [C.c_float, C.c_float, C.c_float, C.POINTER(C.c_int)]
        L.rc_skip_steps.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_float]
        _cache["lib"] = L
    return _cache["lib"]


def host_raycast(units, cols, rows, cam4, T, params=None, skip=False):
    """The host build of the header over a {key: (sdf, weight)} volume -> (depth, vmap, nmap) like raycast_restatement.raycast."""
    keys = np.array(sorted(units), np.int32)
    n = len(keys)
    sdf = np.ascontiguousarray(np.stack([units[int(k)][0] for k in keys]) if n else np.zeros((1, 64 ** 3)), F)
    w = np.ascontiguousarray(np.stack([units[int(k)][1] for k in keys]) if n else np.zeros((1, 64 ** 3)), F)
    t_min, t_max, step = rcr.DEFAULT_PARAMS if params is None else params
    rec = np.zeros((rows * cols, 2, 4), F)
    depth = np.zeros(rows * cols, np.uint16)
    cam = np.array(cam4, F)
    T = np.ascontiguousarray(T, np.float64).reshape(16)
    rc = hostlib().rc_raycast(_p(keys), n, _p(sdf), _p(w), cols, rows, _p(cam), _p(T), F(t_min), F(t_max), F(step), int(skip), _p(rec), _p(depth))
    if rc:
        raise rcr.Refused("count_steps: %d" % rc)
    assert not rec[:, :, 3].any()
    return depth.reshape(rows, cols), rec[:, 0, :3].reshape(rows, cols, 3).copy(), rec[:, 1, :3].reshape(rows, cols, 3).copy()


def same_maps(a, b):
    return np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2])


def restated(name, case):
    """The restatement of a case, computed once."""
    if ("r", name) not in _cache:
        _cache["r", name] = rcr.raycast(case["units"], case["cols"], case["rows"], case["cam"], case["T"], case["params"])
    return _cache["r", name]


def oracle_scene():
    """{key: (sdf, weight)} of the 4-frame scene from the CPU TSDF oracle, and its inputs."""
    if "scene" not in _cache:
        from oracle.pyoracle import OracleVolume
        d, W, cam, cam6 = rcc.scene_inputs()
        ora = OracleVolume(cols=rcc.SCENE_COLS, rows=rcc.SCENE_ROWS, camera=cam6)
        for i in range(len(d)):
            ora.Integrate(d[i].reshape(-1), W[i])
        units = {int(k): ora.read_unit(int(k)) for k in ora.unit_keys()}
        ora.close()
        _cache["scene"] = (units, d, W, cam)
    return _cache["scene"]


ALL_CASES = dict(rcc.crafted(), plane=rcc.plane(), sphere=rcc.sphere(), sphere_default_step=rcc.sphere_default_step())


# ---- header == restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_header_equals_restatement_bit_for_bit_with_and_without_the_skip(name):
    c = ALL_CASES[name]
    want = restated(name, c)
    for skip in (False, True):
        got = host_raycast(c["units"], c["cols"], c["rows"], c["cam"], c["T"], c["params"], skip=skip)
        assert same_maps(got, want), (name, skip)


@pytest.mark.parametrize("view", ["frame1", "novel"])
def test_header_equals_restatement_on_the_integrated_scene(view):
    units, d, W, cam = oracle_scene()
    T = W[1] if view == "frame1" else rcc.novel_pose()
    want = restated(("scene", view), dict(units=units, cols=rcc.SCENE_COLS, rows=rcc.SCENE_ROWS, cam=cam, T=T, params=None))
    assert (want[0] > 0).mean() > 0.9, "the scene fills the view"
    for skip in (False, True):
        assert same_maps(host_raycast(units, rcc.SCENE_COLS, rcc.SCENE_ROWS, cam, T, skip=skip), want), skip


def test_levels_use_the_odometry_intrinsics():
    import odometry_restatement as orr
    units, d, W, cam = oracle_scene()
    od = orr.Odometry(rcc.SCENE_COLS, rcc.SCENE_ROWS, cam)
    lv = rcr.raycast_levels(units, rcc.SCENE_COLS, rcc.SCENE_ROWS, cam, W[1], 3)
    for l, (dep, V, N) in enumerate(lv):
        assert dep.shape == (rcc.SCENE_ROWS >> l, rcc.SCENE_COLS >> l)
        got = host_raycast(units, rcc.SCENE_COLS >> l, rcc.SCENE_ROWS >> l, od.K(l), W[1], skip=True)
        assert same_maps(got, (dep, V, N)), l


# ---- the crafted cases sit where they claim to ----------------------------------------------------------------------------------------------------
def centre(case, m):
    return m[case["rows"] // 2, case["cols"] // 2]


def test_crafted_cases_are_on_their_edges():
    for a in "xyz":
        c = ALL_CASES["border_%s" % a]
        dep, V, N = restated("border_%s" % a, c)
        assert np.isfinite(V).all() and np.isfinite(N).all(), "the cell and the gradient straddle two units that both exist"
        hit = c["T"][:3, 3] + c["T"][:3, :3] @ centre(c, V).astype(np.float64)
        assert abs(hit["xyz".index(a)] - (-0.4 * rcc.UL)) < 1e-4, "the surface lies between voxel 63 and voxel 0 of the next unit"
        assert np.allclose(centre(c, N), [0, 0, 1], atol=1e-5), "away from the camera"
        c = ALL_CASES["border_%s_neighbour_absent" % a]
        dep, V, N = restated("border_%s_neighbour_absent" % a, c)
        assert np.isfinite(V).all() and np.isnan(N).all() and (dep > 0).all(), "nearest-pair fallback: the vertex stays, no normal"
    c = ALL_CASES["corner_unseen"]
    dep, V, N = restated("corner_unseen", c)
    assert np.isfinite(centre(c, V)).all() and np.isnan(centre(c, N)).all() and np.isfinite(N).all(-1).any(), "the vertex stays, the normal goes"
    c = ALL_CASES["exact_zero"]
    dep, V, N = restated("exact_zero", c)
    hit = c["T"][2, 3] + float(centre(c, V)[2])
    assert abs(hit - (rcc.MID + 8 * rcc.UL)) < 1e-5 and np.isfinite(N).all()
    dep, V, N = restated("back_face_first", ALL_CASES["back_face_first"])
    assert not dep.any() and np.isnan(V).all() and np.isnan(N).all(), "a back face met first ends the ray"
    c = ALL_CASES["starts_negative"]
    dep, V, N = restated("starts_negative", c)
    assert np.isfinite(V).all() and abs(c["T"][2, 3] + float(centre(c, V)[2]) - (rcc.MID + 8.4 * rcc.UL)) < 1e-4
    c = ALL_CASES["identity"]
    dep, V, N = restated("identity", c)
    assert np.isfinite(V).all() and np.isfinite(N).all()
    assert centre(c, V)[0] == 0 and centre(c, V)[1] == 0 and (V[:, 8, 0] == 0).all() and (V[6, :, 1] == 0).all()


# ---- truth ------------------------------------------------------------------------------------------------------------------------------------
def away_from_silhouette(hit, px):
    """Pixels whose (2 px + 1)^2 neighbourhood (clipped by the image) holds hits only, and that are px pixels from the image's border."""
    ok = hit.copy()
    rows, cols = hit.shape
    for dy in range(-px, px + 1):
        for dx in range(-px, px + 1):
            s = np.zeros_like(hit)
            s[max(0, -dy):rows - max(0, dy), max(0, -dx):cols - max(0, dx)] = hit[max(0, dy):rows - max(0, -dy), max(0, dx):cols - max(0, -dx)]
            ok &= s
    return ok


@pytest.mark.parametrize("name", ["plane", "sphere"])
def test_restatement_meets_the_analytic_surface(name):
    """Rays that meet the surface at less than 60 degrees from its normal and at least two pixels from a silhouette: the hit distance within
    0.05 mm, the normal within 1e-3 of the analytic one."""
    c = ALL_CASES[name]
    dep, V, N = restated(name, c)
    t, n, cosi = (rcc.plane_truth if name == "plane" else rcc.sphere_truth)(c)
    hit = np.isfinite(V).all(-1)
    sel = away_from_silhouette(hit, 2) & (cosi > 0.5) & np.isfinite(t)
    assert sel.sum() > 5000, sel.sum()
    dist = np.linalg.norm(V.astype(np.float64), axis=-1)
    e_t = np.abs(dist - t)[sel]
    e_n = np.abs(N.astype(np.float64) - n)[sel]
    print("%s: %d rays, hit distance error max %.3g mm, normal error max %.3g" % (name, sel.sum(), 1e3 * e_t.max(), e_n.max()))
    assert np.isfinite(N[sel]).all()
    assert e_t.max() < 0.05e-3
    assert e_n.max() < 1e-3


def scene_depth_errors():
    units, d, W, cam = oracle_scene()
    dep, V, N = restated(("scene", "frame1"), dict(units=units, cols=rcc.SCENE_COLS, rows=rcc.SCENE_ROWS, cam=cam, T=W[1], params=None))
    ref = d[1].astype(np.int64)
    # away from silhouettes: no depth step of 30 mm or more and no hole, in either image, within 3 pixels
    smooth = (ref > 0) & (dep > 0)
    for dy, dx in ((0, 1), (1, 0)):
        a, b = ref[dy:, dx:], ref[:ref.shape[0] - dy, :ref.shape[1] - dx]
        step = np.abs(a - b) >= 30
        smooth[dy:, dx:] &= ~step
        smooth[:ref.shape[0] - dy, :ref.shape[1] - dx] &= ~step
    sel = away_from_silhouette(smooth, 3)
    return np.abs(1000.0 * V[..., 2].astype(np.float64) - ref)[sel]             # (the vertex's z, not its rounding to whole millimetres)


def test_restatement_meets_the_renderer_on_the_integrated_scene():
    e = scene_depth_errors()
    med, p99 = float(np.median(e)), float(np.percentile(e, 99))
    print("scene: %d pixels, median %.4g mm, 99th percentile %.4g mm" % (e.size, med, p99))
    assert e.size > 10000
    assert 2 * MEASURED_SCENE_MM[0] <= 1e3 * rcc.UL, "the bar on the median may not exceed a voxel"
    assert med <= 2 * MEASURED_SCENE_MM[0] and p99 <= 2 * MEASURED_SCENE_MM[1]


# ---- steps, skip bound --------------------------------------------------------------------------------------------------------------------------
def test_count_steps_and_its_refusals():
    L = hostlib()
    n = C.c_int(-1)
    for args, want in (((0.0, 4.0, 0.8 * 0.03), None), ((0.0, 1.0, 1.0), 1), ((0.0, 1.0, 1.0 / 65536), 65536), ((1.0, 1.0, 0.1), 0), ((2.0, 1.0, 0.1), 0)):
        assert L.rc_count_steps(F(args[0]), F(args[1]), F(args[2]), C.byref(n)) == 0
        assert n.value == rcr.count_steps(*args) and (want is None or n.value == want), args
    assert L.rc_count_steps(F(0), F(1), F(1.0 / 65537), C.byref(n)) == 2
    with pytest.raises(rcr.Refused):
        rcr.count_steps(0, 1, 1.0 / 65537)
    for bad in ((np.nan, 1, 0.1), (0, np.inf, 0.1), (0, 1, 0.0), (0, 1, -0.1), (0, 1, np.nan)):
        assert L.rc_count_steps(F(bad[0]), F(bad[1]), F(bad[2]), C.byref(n)) == 1, bad
        with pytest.raises(rcr.Refused):
            rcr.count_steps(*bad)


def test_skip_bound_never_leaves_the_unit():
    """Random points in a unit's box and unit-length directions: every sample the bound skips rounds into that same unit; the count is an
    integer >= 1 whatever the step (1e-30 and 1e30 included: tested as a float before it becomes an int)."""
    L = hostlib()
    g = np.random.default_rng(5)
    u = (255, 257, 250)
    lo = np.array([(64 * a - rcc.HALF - 0.5) * rcc.UL for a in u])
    worst = 0
    for _ in range(4000):
        p = (lo + g.random(3) * 64 * rcc.UL).astype(F)
        d = g.normal(size=3)
        d = (d / np.linalg.norm(d)).astype(F)
        step = F(10.0 ** g.uniform(-4, -1))
        n = L.rc_skip_steps(p[0], p[1], p[2], u[0], u[1], u[2], step)
        assert n >= 1
        worst = max(worst, n)
        for j in (n - 1, max(n - 2, 0)):
            q = d * (F(j) * step) + p
            ok, idx = zip(*[rcr.nearest_index(np.array([x], F)) for x in q])
            assert all(o[0] for o in ok) and tuple(int(i[0]) >> 6 for i in idx) == u, (p, d, step, n)
    assert worst > 100
    for step in (1e-30, 1e30, 1e-45):
        assert 1 <= L.rc_skip_steps(F(lo[0] + 0.18), F(lo[1] + 0.18), F(lo[2] + 0.18), u[0], u[1], u[2], F(step)) <= 65536


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------------
def test_abi_refusals_without_a_device():
    """Every refusal of er_tsdf_raycast that does not need a volume: the message names the reason, nothing is computed."""
    L = _ffi.lib()
    hdr = open(os.path.join(ROOT, "include", "er_hip.h")).read()
    for name in ("er_raycast_params_default", "er_tsdf_raycast", "er_frame_to_model_align"):
        assert name + "(" in hdr and name in _ffi.SYMBOLS and hasattr(L, name), name
    P = _ffi.ErRaycastParams()
    assert L.er_raycast_params_default(C.byref(P)) == 0
    assert (F(P.t_min), F(P.t_max), F(P.step)) == rcr.DEFAULT_PARAMS
    assert L.er_raycast_params_default(None) != 0
    cam, T = np.array([100, 100, 10, 10], F), np.eye(4).reshape(16)
    rec, dep = np.zeros((4, 2, 4), F), np.zeros(4, np.uint16)

    def call(h=None, cols=2, rows=2, cam=cam, T=T, params=None, rec=rec, dep=dep):
        rc = L.er_tsdf_raycast(h, cols, rows, None if cam is None else _p(cam), None if T is None else _p(T), params,
                               None if rec is None else _p(rec), None if dep is None else _p(dep), 0)
        return rc, L.er_last_error().decode()

    def params(t_min, t_max, step):
        return C.byref(_ffi.ErRaycastParams(t_min, t_max, step))

    for kw, word in ((dict(cam=None), "NULL"), (dict(T=None), "NULL"), (dict(cols=0), "image"), (dict(rows=-1), "image"),
                     (dict(params=params(0, 1, 0)), "step"), (dict(params=params(0, 1, -1)), "step"), (dict(params=params(np.nan, 1, 0.1)), "finite"),
                     (dict(params=params(0, np.inf, 0.1)), "finite"), (dict(params=params(0, 1, 1.0 / 65537)), "65536"),
                     (dict(rec=None, dep=None), "outputs"), (dict(), "NULL handle")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, msg)
    assert not rec.any() and not dep.any()
    rc = L.er_frame_to_model_align(None, None, 0, None, 0, None, None, None, None, None, 0)
    assert rc != 0
