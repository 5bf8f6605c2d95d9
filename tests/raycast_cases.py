"""Volumes and views that tests/test_raycast_cpu.py and tests/test_raycast_gpu.py share: analytic TSDFs sampled into whole
units with every voxel observed, crafted units that put a surface on the edges of the ray caster's rule, and the integrated 160 x 120 scene.
A case is a dict: units {key: (sdf, weight)}, cols, rows, cam, T (world_T_camera), params (t_min, t_max, step).  Everything is built once
per process and never written again.

Voxel g (0-based, per axis) sits at (g - 16384) * 3/512 metres; unit u holds voxels 64 u .. 64 u + 63; key = x << 18 | y << 9 | z.
"""
import numpy as np

F = np.float32
UL = 3.0 / 512.0
HALF = 256 * 64
_cache = {}

# the cyclic rotations that turn the camera's z axis to the world's x, y and z axis
LOOK = {0: np.array([[0., 0., 1.], [1., 0., 0.], [0., 1., 0.]]), 1: np.array([[0., 1., 0.], [0., 0., 1.], [1., 0., 0.]]), 2: np.eye(3)}


def key_of(ux, uy, uz):
    return int(ux) << 18 | int(uy) << 9 | int(uz)


def unit_positions(key):
    """float64 [64, 64, 64, 3]: the voxel centres of a unit, in the pool's order (x slowest)."""
    u = np.array([key >> 18, (key >> 9) & 511, key & 511])
    ax = [((64 * u[a] + np.arange(64)) - HALF) * UL for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1)


def sample_units(sdist, keys, trunc):
    """{key: (clip(sdist(x) / trunc, -1, 1) as float32, weight 1)}: every voxel observed."""
    out = {}
    for k in keys:
        f = np.clip(sdist(unit_positions(k)) / trunc, -1.0, 1.0).astype(F).reshape(-1)
        out[k] = (f, np.ones(64 ** 3, F))
    return out


def pose(R, o):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, o
    return T


def cached(name, make):
    if name not in _cache:
        c = make()
        for s, w in c["units"].values():
            s.setflags(write=False)
            w.setflags(write=False)
        _cache[name] = c
    return _cache[name]


EIGHT = [key_of(x, y, z) for x in (255, 256) for y in (255, 256) for z in (255, 256)]      # the units around the lattice's centre: +-0.375 m
# Truncation of the analytic cases: the normalised tsdf is linear (plane) only while a sample's whole trilinear cell lies inside the band, so
# the band must hold a step (0.024 m) plus a cell's diagonal (0.0102 m) on either side of the surface: 0.06 m.
TRUNC_ANALYTIC = 0.06
PLANE_N = np.array([0.3, -0.2, -1.0]) / np.linalg.norm([0.3, -0.2, -1.0])                  # faces the camera; the plane passes through the origin
SPHERE_C, SPHERE_R = np.array([0.0, 0.0, 0.5]), 0.5
ANALYTIC_VIEW = dict(cols=160, rows=120, cam=(160.0, 160.0, 79.5, 59.5), T=pose(np.eye(3), [0.0, 0.0, -1.0]), params=(0.0, 4.0, 0.8 * 0.03))


def plane():
    """Case 1: an oblique plane through the corner that eight units share; the camera sits one metre in front of it in a unit that does not
    exist, and the image is wider than the units, so their border is a silhouette."""
    return cached("plane", lambda: dict(units=sample_units(lambda x: x @ PLANE_N, EIGHT, TRUNC_ANALYTIC), **ANALYTIC_VIEW))


def sphere():
    """Case 2: a sphere of radius 0.5 m whose nearest point is the same corner.  step: along a ray that meets the sphere at the angle a from its
    normal the distance function has the second derivative sin^2 a / R, so the straight line between two samples a step s apart misses the
    crossing by up to s^2 sin^2 a / (8 R cos a) -- 0.22 mm at 60 degrees for the default step of 24 mm, the method's error (KinFu's too), not
    the implementation's.  With a step of one voxel it is 0.013 mm, beside the trilinear cell's own h^2 / (8 R cos a) = 0.017 mm: the bound
    of 0.05 mm is then a statement about the code.  (sphere_default_step: the same units at the default step, for the bit comparisons.)"""
    view = dict(ANALYTIC_VIEW, params=(0.0, 4.0, UL))
    return cached("sphere", lambda: dict(units=sample_units(lambda x: np.linalg.norm(x - SPHERE_C, axis=-1) - SPHERE_R, EIGHT, TRUNC_ANALYTIC), **view))


def sphere_default_step():
    return cached("sphere_default_step", lambda: dict(sphere(), params=ANALYTIC_VIEW["params"]))


def plane_truth(case):
    """(hit distance along the normalised ray, normal in the camera frame, cosine of the incidence) per pixel, float64."""
    dc, o = rays(case)
    t = -(o @ PLANE_N) / (dc @ PLANE_N)
    n = np.broadcast_to(-PLANE_N, dc.shape)            # er_od::normal's sense: away from the camera
    return t, n, np.abs(dc @ PLANE_N)


def sphere_truth(case):
    dc, o = rays(case)
    oc = o - SPHERE_C
    b = dc @ oc
    disc = b * b - (oc @ oc - SPHERE_R ** 2)
    with np.errstate(invalid="ignore"):
        t = -b - np.sqrt(disc)
    x = o + t[..., None] * dc
    n = -(x - SPHERE_C) / SPHERE_R
    return t, n, np.abs(np.sum(dc * n, -1))


def rays(case):
    """float64 unit rays [rows, cols, 3] of an identity-rotation view, and the camera's position."""
    fx, fy, cx, cy = case["cam"]
    u, v = np.meshgrid(np.arange(case["cols"], dtype=np.float64), np.arange(case["rows"], dtype=np.float64))
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    assert np.array_equal(case["T"][:3, :3], np.eye(3))
    return d / np.linalg.norm(d, axis=-1, keepdims=True), case["T"][:3, 3]


# ---- crafted units ------------------------------------------------------------------------------------------------------------------------------
FINE = (0.0, 0.5, 0.9 * UL)                            # a step below a voxel: no voxel along the ray is stepped over
MID = (64 * 256 + 32 - HALF) * UL                      # coordinate of voxel 32 of unit 256


def slab_units(axis, plane_at, keys, trunc=0.03, edit=None):
    """sdf = (plane_at - x[axis]) / trunc: positive in front of the plane for a camera that looks up the axis."""
    units = sample_units(lambda x: plane_at - x[..., axis], keys, trunc)
    if edit:
        units = {k: (s.copy(), w.copy()) for k, (s, w) in units.items()}
        edit(units)
    return units


def along(axis, at, lateral=MID):
    o = np.full(3, lateral)
    o[axis] = at
    return pose(LOOK[axis], o)


def border(axis, neighbour=True):
    """The surface between voxel 63 of unit 255 and voxel 0 of unit 256 along `axis` (neighbour = True: the trilinear cell and the gradient
    straddle the two units), or between voxels 62 and 63 of unit 255 with unit 256 ABSENT: the crossing is found on the nearest voxels, the cell
    of the later sample and the gradient reach into the missing unit -- the nearest-pair fallback, a vertex and no normal."""
    def make():
        u = [256, 256, 256]
        u[axis] = 255
        keys = [key_of(*u)] + ([key_of(256, 256, 256)] if neighbour else [])
        at = -0.4 * UL if neighbour else -1.4 * UL
        return dict(units=slab_units(axis, at, keys), cols=7, rows=5, cam=(30.0, 30.0, 3.0, 2.0), T=along(axis, -0.2), params=FINE)
    return cached(("border", axis, neighbour), make)


K0 = key_of(256, 256, 256)
VOX = lambda i, j, k: i * 4096 + j * 64 + k            # noqa: E731  (index of a voxel in its unit)


def inside_view(z_cam=5):
    return dict(cols=7, rows=5, cam=(30.0, 30.0, 3.0, 2.0), T=along(2, (64 * 256 + z_cam - HALF) * UL), params=FINE)


def corner_unseen():
    """A surface inside one unit, and one corner of the centre ray's hit cell with weight 0: not the voxel nearest to the ray (an unobserved
    SAMPLE would make the march forget the free space in front of it), the one diagonally across the cell."""
    def edit(units):
        units[K0][1][VOX(33, 33, 41)] = 0.0
    return cached("corner_unseen", lambda: dict(units=slab_units(2, MID + 8.4 * UL, [K0], edit=edit), **inside_view()))


def exact_zero():
    """The plane lies exactly on a layer of voxel centres: that layer's sdf is 0.0f, the sample before the crossing."""
    def make():
        c = dict(units=slab_units(2, MID + 8 * UL, [K0]), **inside_view())
        assert np.count_nonzero(c["units"][K0][0] == 0) == 64 * 64
        return c
    return cached("exact_zero", make)


def two_faces(gap):
    """Seen from a camera inside the unit: negative space up to voxel 20 (a back face), free space, and a front face at voxel 40.  gap = False:
    the ray meets the back face first and ends.  gap = True: the layers around the back face are unobserved, the ray forgets that it started
    in negative space and finds the front face."""
    def make():
        z1, z2 = MID - 12.4 * UL, MID + 8.4 * UL
        sd = lambda x: np.minimum(x[..., 2] - z1, z2 - x[..., 2])              # noqa: E731
        units = {k: (s.copy(), w.copy()) for k, (s, w) in sample_units(sd, [K0], 0.03).items()}
        if gap:
            units[K0][1].reshape(64, 64, 64)[:, :, 16:24] = 0.0
        return dict(units=units, **inside_view())
    return cached(("two_faces", gap), make)


def identity_view():
    """The identity pose with integer cx, cy: the camera at the lattice's centre, the centre ray exactly (0, 0, 1), a column and a row of rays
    with a zero component, and an oblique plane 0.2 m ahead across four units."""
    def make():
        n = np.array([0.2, 0.1, -1.0]) / np.linalg.norm([0.2, 0.1, -1.0])
        keys = [key_of(x, y, 256) for x in (255, 256) for y in (255, 256)]
        return dict(units=sample_units(lambda x: (x - np.array([0.0, 0.0, 0.2])) @ n, keys, 0.03), cols=17, rows=13, cam=(60.0, 60.0, 8.0, 6.0),
                    T=np.eye(4), params=(0.0, 4.0, 0.8 * 0.03))
    return cached("identity", make)


def crafted():
    """name -> case, for the bit-for-bit comparisons."""
    out = {"identity": identity_view(), "corner_unseen": corner_unseen(), "exact_zero": exact_zero(), "back_face_first": two_faces(False),
           "starts_negative": two_faces(True)}
    for a in range(3):
        out["border_%s" % "xyz"[a]] = border(a, True)
        out["border_%s_neighbour_absent" % "xyz"[a]] = border(a, False)
    return out


# ---- the integrated scene ----------------------------------------------------------------------------------------------------------------------
SCENE_COLS, SCENE_ROWS, SCENE_FRAMES = 160, 120, 4
SCENE_SHIFT = np.array([0.19, 0.17, 0.2])


def scene_inputs(n=SCENE_FRAMES):
    """(depth uint16 [n, rows, cols], poses [n, 4, 4], cam4, cam6 for TSDFVolume): synth.render_depth at 160 x 120 with cam / 4."""
    import odometry_cases as oc
    d, W, cam = oc.scene(SCENE_COLS, SCENE_ROWS, n)
    # integration_trunc 4 m, the ray caster's default t_max: at the default 2.5 m the volume holds the sphere and one wall only, and a
    # sphere in front of a plane leaves a point-to-plane alignment free to turn about the axis through the sphere's centre
    cam6 = np.array([cam[0], cam[1], cam[2], cam[3], 2.5, 4.0], F)
    # The room's walls lie at 0 and 3 m: on borders of the 0.375 m units.  A unit exists only where a depth pixel's surface point falls
    # (TSDFVolume.cpp:47-52), so the half of a wall's band that lies across such a border is in no unit, the sdf never changes sign there and
    # the ray caster cannot see the wall.  The world is moved off the lattice: walls in the middle of units.
    W = np.asarray(W, np.float64).copy()
    W[:, :3, 3] += SCENE_SHIFT
    return d, W, cam, cam6


def novel_pose():
    """A pose none of the frames was integrated from: between frames 1 and 2, moved 3 cm sideways."""
    _, W, _, _ = scene_inputs()
    T = W[1].copy()
    T[:3, 3] = 0.5 * (W[1][:3, 3] + W[2][:3, 3]) + W[1][:3, :3] @ np.array([0.03, -0.01, 0.0])
    return T
