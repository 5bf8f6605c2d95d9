"""Inputs that tests/test_odometry_cpu.py and tests/test_odometry_gpu.py share: the rendered sweep at the two test sizes (rendered once per
process), a seeded image with holes, a depth step and occupied borders, and the bit comparison of float32 maps."""
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
