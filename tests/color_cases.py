"""Fixtures of the colour tests (tests/test_color_cpu.py, tests/test_color_gpu.py): small RGB-D scenes rendered by synth.render_rgbd with a camera
scaled to the image, and the conditions each one is there for.  A scene is a dict(cols, rows, cam = fx fy cx cy icp_trunc integration_trunc,
poses float64[n, 4, 4], depth uint16[n, rows * cols], rgb uint8[n, rows * cols, 3], lo, hi)."""
import math

import numpy as np

from elasticreconstruction_amd import synth

KEY0 = 256 << 18 | 256 << 9 | 256                     # the unit whose voxel (0, 0, 0) sits at the origin


def small_cam(cols, rows, trunc=2.5):
    """The reference camera (TSDFVolumeUnit.h:69) scaled to a cols x rows image; integration_trunc = trunc metres."""
    s = cols / 640.0
    return np.array([525.0 * s, 525.0 * s, (cols - 1) / 2.0, (rows - 1) / 2.0, 2.5, trunc], np.float32)


def scene(poses, cols, rows, trunc=2.5, lo=synth.ROOM_LO, hi=synth.ROOM_HI, sphere=True):
    cam = small_cam(cols, rows, trunc)
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    d, c = synth.render_rgbd(poses, cols, rows, tuple(float(x) for x in cam[:4]), lo, hi, sphere)
    return dict(cols=cols, rows=rows, cam=cam, poses=poses, depth=synth.to_numpy_u16(d), rgb=c.numpy(), lo=lo, hi=hi, sphere=sphere)


def orbit(n, radius, arc, height=0.15, start=0.0):
    """n cameras on an arc of `arc` radians around the room's centre at `radius`, looking at the sphere, bobbing `height` metres."""
    out = []
    for i in range(n):
        th = start + arc * i / max(n - 1, 1)
        eye = np.array([1.5 + radius * math.cos(th), 1.5 + height * math.sin(3.0 * th), 1.5 + radius * math.sin(th)])
        out.append(synth.look_at(eye, np.array(synth.SPHERE_C) - eye))
    return np.array(out)


def room_with_sphere(cols, rows):
    """The GPU scene: two views of the sphere from 0.75 m (the walls behind it lie beyond integration_trunc = 1.2 m: pixels step 2 rejects) and
    two of a wall from the circle trajectory, 0.9 m in front of it.  55 units."""
    poses = np.concatenate([orbit(2, 0.75, 0.2), synth.circle_trajectory(40, radius=0.6)[3:5]])
    return scene(poses, cols, rows, trunc=1.2)


def negative_corner(cols, rows):
    """A room around the origin seen from near it, looking into the corner (-1.49, -1.49, -1.49): every coordinate of the surface is negative,
    and the three walls cross unit borders (a unit is 0.375 m wide)."""
    poses = [synth.look_at((-0.6, -0.7, -0.5), (-1.0, -0.9, -0.8)), synth.look_at((-0.55, -0.7, -0.55), (-1.0, -0.8, -0.9))]
    return scene(poses, cols, rows, lo=-1.49, hi=1.51, sphere=False)


def ground_truth_scene():
    """The CPU scene: 20 rigid frames at 160 x 120 on a 108 degree arc at 1.05 m around the sphere, which they all see in front of the walls
    (up to 2.5 m away).  152 units."""
    return scene(orbit(20, 1.05, 0.6 * math.pi), 160, 120)


def contention_frame(cols, rows):
    """Every pixel of a frame in ONE voxel: a camera whose focal length is so long that the whole image spans a fraction of a millimetre at
    1 m, looking along +z from a point chosen so that the surface point is the centre of voxel (10, 20, 30 + 171) of unit KEY0; colour
    255 255 255.  -> (cam, T, depth, rgb, voxel index inside the unit)."""
    cam = np.array([1.0e6, 1.0e6, (cols - 1) / 2.0, (rows - 1) / 2.0, 2.5, 2.5], np.float32)
    ul = 3.0 / 512.0
    T = np.eye(4)
    T[:3, 3] = [10 * ul, 20 * ul, 30 * ul + 0.002]                    # + z = 1.000 m: 30 ul + 0.002 + 1.0 = 201.0 ul + 0.0003: inside voxel 201
    depth = np.full(rows * cols, 1000, np.uint16)
    rgb = np.full((rows * cols, 3), 255, np.uint8)
    g = (10, 20, 201)
    key = KEY0 + (g[2] >> 6)
    return cam, T, depth, rgb, key, (g[0] * 64 + g[1]) * 64 + (g[2] & 63)


def warp_case(cols, rows, interval=2, amplitude=0.04, resolution=8, length=3.0):
    """Four frames under a control-grid warp (synth's fragment bookkeeping at a small image): the scene dict plus traj and warp =
    IntegrateFrames' warp dict; two fragments of two frames, lattices deformed by 4 cm.  Two views of the sphere in front of the far wall:
    source pixels are occluded after the warp.  Two frontal views of a wall from 0.9 m: every source depth is 900 mm, and where the lattice
    compresses the image two source pixels of equal warped depth land in one cell."""
    from elasticreconstruction_amd.tsdf import mat4_mul
    world = np.concatenate([orbit(2, 0.75, 0.2), [synth.look_at((1.5, 1.5, 2.09), (0, 0, 1)), synth.look_at((1.56, 1.47, 2.09), (0, 0, 1))]])
    sc = scene(world, cols, rows, trunc=1.2)
    n = len(world)
    pose, seg = synth.split_trajectory(world, interval, length)
    traj = np.empty_like(world)
    for i in range(n // interval):
        for j in range(interval):
            traj[i * interval + j] = mat4_mul(pose[i], seg[i * interval + j])
    full = dict(traj=traj, pose=pose, seg=seg, grids=synth.control_grids(pose, resolution, length, amplitude), interval=interval,
                resolution=resolution, length=length, n=n)
    sc.update(traj=traj, warp=synth.warp_arrays(full))
    return sc
