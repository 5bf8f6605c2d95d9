"""Inputs that tests/test_odometry_cpu.py, tests/test_odometry_gpu.py and tests/test_odometry_shapes_gpu.py share: the rendered sweep at the
test sizes (rendered once per process), a seeded image with holes, a depth step and occupied borders, the images and poses that sit on the
edges of the kernels (SHAPES, comb, table_end_image, extreme_image, border_poses), the bit comparison of float32 maps and a pose step in
extended precision.  tests/test_odometry_cpu.py checks on the restatement that every fixture is where it claims to be."""
import math

import numpy as np

from elasticreconstruction_amd import synth

F = np.float32
_cache = {}


def scaled_cam(cols):
    fx, fy, cx, cy = synth.CAM
    return (fx * cols / 640, fy * cols / 640, (cx + 0.5) * cols / 640 - 0.5, (cy + 0.5) * cols / 640 - 0.5)


def scene(cols, rows, n=4):
    """Frames 0 .. n-1 of the hand-held sweep (sphere and five walls in view), their poses and the intrinsics; rendered once."""
    key = ("scene", cols, rows, n)
    if key not in _cache:
        W = synth.kinfu_camera_path(0, 4, 50)[:n]
        cam = scaled_cam(cols)
        d = synth.to_numpy_u16(synth.render_depth(W, cols=cols, rows=rows, cam=cam)).reshape(n, rows, cols)
        d.setflags(write=False)
        _cache[key] = (d, W, cam)
    return _cache[key]


def seeded_image(cols, rows, seed):
    """A slanted surface with noise, a depth step down the middle, two holes (one at a corner), single dropped pixels, and values at
    the borders of the image."""
    g = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(cols), np.arange(rows))
    d = 900 + 3 * u + 2 * v + g.integers(-12, 13, (rows, cols))
    d[:, cols // 2:] += 400                                   # a step far beyond the filter's depth support
    d[:, cols // 3] += 60                                     # and a ridge inside it
    d[rows // 3:rows // 3 + 7, cols // 4:cols // 4 + 9] = 0
    d[:5, :6] = 0
    d[g.random((rows, cols)) < 0.02] = 0
    return d.astype(np.uint16)


def same_bits(a, b):
    """float32 arrays: NaN in the same places, the same bits everywhere else."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


# ---- the edges of the launch geometry, the levels and the data (tests/test_odometry_shapes_gpu.py) ------------------------------------------
# k_odom_iter gives a workgroup 1024 consecutive pixels of a level; k_odom_final adds the workgroups' partial vectors in 8 strided slices.
# (cols, rows, parameters): whole renders, never crops (a top-left crop shows one wall, and J^T J is rank-deficient).
SHAPES = [
    (32, 32, dict(levels=1)),                  # 1024 pixels: one full workgroup
    (41, 25, dict(levels=1)),                  # 1025: a second workgroup that holds one pixel
    (40, 26, dict(levels=2)),                  # 1040, 260
    (128, 64, dict(levels=1)),                 # 8192: 8 workgroups, one per slice
    (129, 64, dict(levels=1)),                 # 8256: 9 workgroups, the first slice takes two
    (70, 50, dict(levels=2)),                  # 3500, 875
    (96, 64, dict(levels=4)),                  # 6144, 1536, 384, 96: level 3
    (80, 56, dict(levels=4, min_valid=10)),    # 4480, 1120, 280, 70 (46 matches at level 3, below the default min_valid)
    (16, 12, dict(levels=1)),                  # 192: less than one workgroup
    (5, 3, dict(levels=1)),                    # 15: less than one wave, narrower than the filter's window; maps and linearisation only
    (1, 1, dict(levels=1)),                    # 1: maps and linearisation only
]
ALIGNABLE = [s for s in SHAPES if s[0] >= 16]


def comb(frame):
    """The frame with every pixel zeroed except those at [::4, ::4].  The pyramid keeps a pixel whenever its centre is valid, so level 2 is
    dense while levels 0 and 1 have no valid normal: a pair with a comb in it is lost at the first iteration of level 1."""
    out = np.zeros_like(np.asarray(frame))
    out[::4, ::4] = np.asarray(frame)[::4, ::4]
    return out


TABLE_END_TAPS = [((6, 6), +1, -1), ((-6, 6), -1, -1), ((6, -5), +1, -2), ((-6, -6), +1, 0)]     # (offset (dx, dy), sign, n_depth_w + this)


def table_end_probes(cols, rows):
    """The (x, y) around which table_end_image puts its taps: the interior, and one 6 pixels from the left and top borders and one 6 pixels
    from the right and bottom borders (their taps sit ON the borders)."""
    return [(cols // 2, rows // 2), (6, 6), (cols - 7, rows - 7)]


def table_end_image(cols, rows, n_depth_w, c=1000):
    """A constant background c with isolated taps c + (n - 1) and c - (n - 1) (the last entry of the depth-weight table, n = n_depth_w),
    c + (n - 2) and c + n (the first difference the table does not hold), at the offsets TABLE_END_TAPS from every probe pixel: two corners
    of the probe's 13 x 13 window (dx^2 + dy^2 = 72, the smallest space weight), the third corner, and the pixel beside the fourth."""
    assert cols >= 39 and rows >= 25 and c > n_depth_w
    d = np.full((rows, cols), c, np.int64)
    for px, py in table_end_probes(cols, rows):
        for (dx, dy), sign, k in TABLE_END_TAPS:
            assert d[py + dy, px + dx] == c
            d[py + dy, px + dx] = c + sign * (n_depth_w + k)
    return d.astype(np.uint16)


def extreme_image(cols, rows, seed):
    """seeded_image moved to the ends of uint16: the half right of the step becomes a smooth (noisy, slanted) surface that ends at 65535 and
    stays above 60000, the half left of it straddles 32767 | 32768 (the sign bit of an int16 frame), and a patch of 1 .. 3 lies against
    the hole in the interior.  Holes and dropped pixels stay where they are."""
    s = seeded_image(cols, rows, seed).astype(np.int64)
    hole = s == 0
    out = np.zeros_like(s)
    left, right = s[:, :cols // 2], s[:, cols // 2:]
    out[:, cols // 2:] = 65535 - (right.max() - right)
    out[:, :cols // 2] = 32767 + (left - int(np.median(left[left > 0])))
    y, x = rows // 3 + 7, cols // 4                          # the rows below the interior hole
    u, v = np.meshgrid(np.arange(9), np.arange(3))
    out[y:y + 3, x:x + 9] = 1 + (u + v) % 3
    out[hole] = 0
    out[rows // 2 + 3, 2:4] = (32767, 32768)
    out[y, x:x + 2] = (1, 2)
    assert out.min() == 0 and out.max() == 65535
    return out.astype(np.uint16)


def pose(R=None, t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = t
    return T


# Poses m_T_c that push pixels through the borders of the projective match, for scene(72, 52) and scene(129, 64), frame 0 against frame 1
# (tests/test_odometry_cpu.py asserts the fractions on the restatement).  name -> (pose, border the pixels leave through or None).
def border_poses():
    nan, inf = pose(), pose()
    nan[1, 2] = np.nan
    inf[0, 3] = np.inf
    return {
        "+x": (pose(t=(0.9, 0.0, 0.0)), "right"),
        "-x": (pose(t=(-0.9, 0.0, 0.0)), "left"),
        "+y": (pose(t=(0.0, 0.5, 0.0)), "bottom"),
        "-y": (pose(t=(0.0, -0.5, 0.0)), "top"),
        "-z": (pose(t=(0.0, 0.0, -2.0)), None),                       # gz <= 0 for the near part of the scene
        "turn": (pose(R=np.diag([-1.0, -1.0, 1.0])), None),         # 180 degrees about the optical axis: pixel (u, v) -> (cols-1-u, rows-1-v)
        "nan": (nan, None),
        "inf": (inf, None),
    }


def projection(V, K, T):
    """float64 statement of where the valid vertices of a float32 vertex map land under T: (valid, gz, pu, pv) with pu, pv not rounded.
    For stating fixture conditions only; the pin of the match itself is Odometry.rows_of."""
    fx, fy, cx, cy = (float(k) for k in K)
    v = V.reshape(-1, 3).astype(np.float64)
    valid = np.isfinite(v).all(1)
    with np.errstate(all="ignore"):
        g = v @ T[:3, :3].T + T[:3, 3]
        return valid, g[:, 2], g[:, 0] * fx / g[:, 2] + cx, g[:, 1] * fy / g[:, 2] + cy


# ---- one pose step in extended precision (the solve test of tests/test_odometry_shapes_gpu.py) -------------------------------------------
def step_longdouble(sums, T):
    """Odometry.step in numpy.longdouble with a hand-written 6 x 6 Cholesky: A = L L^T, L y = b, L^T x = y, then
    T <- [Rz Ry Rx | x[3:6]] T.  Returns the new pose as longdouble [4, 4]."""
    LD = np.longdouble
    s = np.asarray(sums, np.float64).astype(LD)
    T = np.asarray(T, np.float64).reshape(4, 4).astype(LD)
    A = np.zeros((6, 6), LD)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = s[k]
            k += 1
    b = s[21:27]
    L = np.zeros((6, 6), LD)
    for j in range(6):
        d = A[j, j] - sum((L[j, q] * L[j, q] for q in range(j)), LD(0))
        assert d > 0
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - sum((L[i, q] * L[j, q] for q in range(j)), LD(0))) / L[j, j]
    y = np.zeros(6, LD)
    for i in range(6):
        y[i] = (b[i] - sum((L[i, q] * y[q] for q in range(i)), LD(0))) / L[i, i]
    x = np.zeros(6, LD)
    for i in range(5, -1, -1):
        x[i] = (y[i] - sum((L[q, i] * x[q] for q in range(i + 1, 6)), LD(0))) / L[i, i]
    sa, ca, sb, cb, sg, cg = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    M = np.array([[cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca],
                  [sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca],
                  [-sb, cb * sa, cb * ca]], LD)
    out = np.zeros((4, 4), LD)
    out[3, 3] = 1
    for r in range(3):
        for c in range(3):
            out[r, c] = sum((M[r, q] * T[q, c] for q in range(3)), LD(0))
        out[r, 3] = sum((M[r, q] * T[q, 3] for q in range(3)), LD(0)) + x[3 + r]
    return out
