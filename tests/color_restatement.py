"""numpy restatement of the colour entries (include/er_hip.h): the splat of registered RGB frames into per-voxel integer
accumulators (er_tsdf_color_frames) and the colour of a point (er_tsdf_sample_colors).

The accumulators are {unit key: uint32[64^3, 4] = r_sum, g_sum, b_sum, n}; a key of the dict is a unit that exists.  Every float operation is
an elementwise numpy operation of the precision and in the order the header gives, so the device's sums are these bit for bit; the sums
themselves are integers (np.add.at), which no order changes."""
import numpy as np

UL = 3.0 / 512.0
UNIT_VOX = 64 ** 3
HALF = 256 * 64                                       # lattice offset: voxel g in [-16384, 16384) is index g + 16384 of the 0-based lattice


def empty_units(keys):
    return {int(k): np.zeros((UNIT_VOX, 4), np.uint32) for k in keys}


def usable(depth, cam, cols, rows):
    """The pixels TSDFVolume::IntegrateVolumeUnit uses: d != 0 and ScaleDepth(d) > 0.001f (float32; beyond integration_trunc ScaleDepth is 0).
    depth: uint16[rows * cols]; cam: fx fy cx cy icp_trunc integration_trunc."""
    c = np.asarray(cam, np.float32)
    p = np.arange(rows * cols)
    u, v = (p % cols).astype(np.float32), (p // cols).astype(np.float32)
    xl = (u - c[2]) / c[0]
    yl = (v - c[3]) / c[1]
    lam = np.sqrt((xl * xl + yl * yl) + np.float32(1.0))
    with np.errstate(over="ignore", invalid="ignore"):
        res = (depth.astype(np.float32) * lam) / np.float32(1000.0)
    res = np.where(res > c[5], np.float32(0.0), res)
    return (depth != 0) & (res > np.float32(0.001))


def world_voxels(depth, T, cam, cols, rows):
    """g = floor(p / UL + 0.5) per axis, float64[rows * cols, 3], of every pixel's world point: UVD2XYZ (TSDFVolume.h:40-49), then
    ((T0 x + T1 y) + T2 z) + T3."""
    c = np.asarray(cam, np.float32)
    T = np.asarray(T, np.float64).reshape(4, 4)
    p = np.arange(rows * cols)
    u, v = (p % cols).astype(np.float32), (p // cols).astype(np.float32)
    z = depth.astype(np.float64) / 1000.0
    x = (u - c[2]).astype(np.float64) * z / np.float64(c[0])
    y = (v - c[3]).astype(np.float64) * z / np.float64(c[1])
    g = np.empty((rows * cols, 3), np.float64)
    for a in range(3):
        pa = ((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3]
        g[:, a] = np.floor(pa / UL + 0.5)
    return g


def splat(units, depth, rgb, T, cam, cols, rows):
    """One frame into `units` in place.  depth uint16[rows * cols], rgb uint8[rows * cols, 3].  Returns (added, no_unit, out_of_range)."""
    depth = np.asarray(depth, np.uint16).reshape(-1)
    rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
    ok = usable(depth, cam, cols, rows)
    with np.errstate(over="ignore", invalid="ignore"):
        g = world_voxels(depth, T, cam, cols, rows)
        inside = ((g >= -HALF) & (g < HALF)).all(axis=1)              # (NaN fails)
    out_of_range = int((ok & ~inside).sum())
    sel = np.nonzero(ok & inside)[0]
    a = g[sel].astype(np.int64) + HALF
    key = (a[:, 0] >> 6) << 18 | (a[:, 1] >> 6) << 9 | (a[:, 2] >> 6)
    local = ((a[:, 0] & 63) * 64 + (a[:, 1] & 63)) * 64 + (a[:, 2] & 63)
    added = 0
    for k in np.unique(key):
        if int(k) not in units:
            continue
        m = key == k
        val = np.concatenate([rgb[sel[m]].astype(np.uint32), np.ones((int(m.sum()), 1), np.uint32)], axis=1)
        np.add.at(units[int(k)], local[m], val)
        added += int(m.sum())
    return added, len(sel) - added, out_of_range


def splat_frames(units, depth, rgb, Ts, cam, cols, rows):
    st = np.zeros(3, np.int64)
    for f in range(len(Ts)):
        st += splat(units, depth[f], rgb[f], Ts[f], cam, cols, rows)
    return tuple(int(x) for x in st)


def nearest_voxel(points):
    """rint((double)p / UL) per component, half to even: float64[n, 3] on the signed lattice (er_tsdf_extract_oriented's nearest voxel)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.rint(np.asarray(points, np.float32)[:, :3].astype(np.float64) / UL)


def _gather(units, a):
    """Accumulators uint64[n, 4] of the 0-based lattice voxels a int64[n, 3]; 0 off the lattice and in units that do not exist."""
    out = np.zeros((a.shape[0], 4), np.uint64)
    on = ((a >= 0) & (a < 512 * 64)).all(axis=1)
    key = (a[:, 0] >> 6) << 18 | (a[:, 1] >> 6) << 9 | (a[:, 2] >> 6)
    local = ((a[:, 0] & 63) * 64 + (a[:, 1] & 63)) * 64 + (a[:, 2] & 63)
    for k in np.unique(key[on]):
        if int(k) in units:
            m = on & (key == k)
            out[m] = units[int(k)][local[m]]
    return out


def sample(units, points):
    """-> (rgba uint8[n, 4], level int[n]: 0, 1, or -1 = no colour)."""
    v = nearest_voxel(points)
    n = v.shape[0]
    with np.errstate(invalid="ignore"):
        on = ((v >= -HALF) & (v < HALF)).all(axis=1)                  # (NaN and infinities fail)
    a = np.where(on[:, None], v, 0.0).astype(np.int64) + HALF
    s = _gather(units, a)
    s[~on] = 0
    level = np.where(s[:, 3] > 0, 0, -1)
    rest = np.nonzero(on & (level < 0))[0]
    if rest.size:
        t = np.zeros((rest.size, 4), np.uint64)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    t += _gather(units, a[rest] + np.array([dx, dy, dz], np.int64))
        s[rest] = t
        level[rest] = np.where(t[:, 3] > 0, 1, -1)
    rgba = np.zeros((n, 4), np.uint8)
    c = level >= 0
    cnt = s[c, 3].astype(np.int64)
    for ch in range(3):
        rgba[c, ch] = ((2 * s[c, ch].astype(np.int64) + cnt) // (2 * cnt)).astype(np.uint8)
    rgba[c, 3] = 255
    return rgba, level


# ---- the warped colour image -------------------------------------------------------------------------------------------------------------

def build_color_check(root):
    """tests/hostcheck/color_check.cpp compiled for the host (er::reproject_px, erfmt::load_png_rgb8, the coloured erfmt::save_ply)."""
    import os
    import subprocess
    src = os.path.join(root, "tests", "hostcheck", "color_check.cpp")
    out = os.path.join(root, "tests", "hostcheck", "_build", "color_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    deps = [src, os.path.join(root, "elasticreconstruction_amd", "csrc", "host", "er_formats.h"),
            os.path.join(root, "elasticreconstruction_amd", "csrc", "er_tsdf_math.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", src, "-o", out, "-lz"], check=True)
    return out


def reproject_cells(color_check, tmp, depth, cam, cols, rows, ctr, resolution, length, seg, madj):
    """(cell int32[rows * cols], dd int32[rows * cols]) of every source pixel through er::reproject_px on the host; cell -1 = depth 0 or no cell."""
    import os
    import subprocess
    a, b = os.path.join(str(tmp), "cells_in.bin"), os.path.join(str(tmp), "cells_out.bin")
    with open(a, "wb") as f:
        f.write(np.array([cols, rows, resolution], np.int32).tobytes())
        f.write(np.asarray(cam, np.float32).tobytes())
        f.write(np.float32(length).tobytes())
        f.write(np.asarray(seg, np.float64).reshape(16).tobytes())
        f.write(np.asarray(madj, np.float64).reshape(16).tobytes())
        f.write(np.ascontiguousarray(ctr, np.float32).tobytes())
        f.write(np.ascontiguousarray(depth, np.uint16).tobytes())
    subprocess.run([color_check, "cells", a, b], check=True, timeout=60)
    out = np.fromfile(b, np.int32)
    return out[:rows * cols].copy(), out[rows * cols:].copy()


def warp_images(cell, dd, rgb):
    """(Z uint16[px], C' uint8[px, 3], winner int64[px] (-1: none)) from the per-pixel (cell, dd).  Z is the reference's sequential replay,
    "write if empty or closer" in source order (IntegrateApp.cpp:260-263; a write of 0 empties the cell).  winner(c) = the lowest source pixel
    with cell c and dd == Z[c] != 0."""
    px = cell.shape[0]
    Z = np.zeros(px, np.uint16)
    for p in np.nonzero(cell >= 0)[0]:
        c = cell[p]
        if Z[c] == 0 or Z[c] > dd[p]:
            Z[c] = dd[p]
    win = np.full(px, -1, np.int64)
    for p in np.nonzero(cell >= 0)[0][::-1]:
        c = cell[p]
        if Z[c] != 0 and dd[p] == Z[c]:
            win[c] = p
    C = np.zeros((px, 3), np.uint8)
    C[win >= 0] = np.asarray(rgb, np.uint8).reshape(-1, 3)[win[win >= 0]]
    return Z, C, win
