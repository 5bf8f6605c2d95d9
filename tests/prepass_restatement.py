"""numpy restatement of path A's pre-pass (k_prepare): what one batch of depth frames hands to the voxel pass.

  scaled        ScaleDepth (TSDFVolume.cpp:19-36), float32, each frame followed by PAD zeros;
  tile_max      per 32 x 32 pixel tile and frame: the maximum of the scaled depth (0 for a tile without depth);
  tile_lo       per 32 x 32 tile and frame: the minimum over EVERY pixel of the tile that lies in the image of (scaled > 0.001f ? scaled : 0);
  tile_lo_fine  the same minimum per 16 x 16 tile;
  keys, masks   the units the batch touches (TSDFVolume.cpp:45-58; the reference's float64 expression, division for division) in ascending
                key order, and per unit the frames that touch it (bit f);
  out_of_range  pixels with depth whose unit index leaves [0, 512) on some axis: skipped and counted.

Every float operation is an elementwise numpy operation of the precision and in the order the reference gives; minima and maxima are over sets,
which no order changes.  The device's products are these bit for bit."""
import numpy as np

UL = 3.0 / 512.0
HALF = 256 * 64                                       # voxel g in [-16384, 16384) is index g + 16384 of the 0-based lattice
PAD = 64                                              # kScaledPad
TILE, FINE = 32, 16
BATCH = 64
BIG = np.float32(3.0e38)                              # "no pixel yet" of the minima
DEFAULT_CAM = (525.0, 525.0, 319.5, 239.5, 2.5, 2.5)


def _uv(cols, rows):
    p = np.arange(rows * cols)
    return (p % cols).astype(np.float32), (p // cols).astype(np.float32)


def scale_lambda(cam, cols, rows):
    c = np.asarray(cam, np.float32)
    u, v = _uv(cols, rows)
    xl = (u - c[2]) / c[0]
    yl = (v - c[3]) / c[1]
    return np.sqrt((xl * xl + yl * yl) + np.float32(1.0))


def scale_depth(depth, cam, cols, rows):
    """depth uint16[..., rows * cols] -> float32 of the same shape."""
    c = np.asarray(cam, np.float32)
    res = (np.asarray(depth).astype(np.float32) * scale_lambda(cam, cols, rows)) / np.float32(1000.0)
    return np.where(res > c[5], np.float32(0.0), res).astype(np.float32)


def unit_keys(depth, T, cam, cols, rows):
    """int64[rows * cols]: the hash key of the unit each pixel touches; -1 without depth, -2 out of range."""
    c = np.asarray(cam, np.float32)
    T = np.asarray(T, np.float64).reshape(4, 4)
    d = np.asarray(depth, np.uint16).reshape(-1)
    u, v = _uv(cols, rows)
    z = d.astype(np.float64) / 1000.0
    x = (u - c[2]).astype(np.float64) * z / np.float64(c[0])
    y = (v - c[3]).astype(np.float64) * z / np.float64(c[1])
    key = np.zeros(d.size, np.int64)
    ok = np.ones(d.size, bool)
    for a in range(3):
        pa = ((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3]
        g = np.floor(pa / UL + 0.5)
        ok &= (g >= -HALF) & (g < HALF)
        key = key * 512 + (np.where(ok, g, 0).astype(np.int64) + HALF) // 64
    return np.where(d == 0, -1, np.where(ok, key, -2))


def _tiles(a, cols, rows, size, fill, reduce):
    """a float32[n, rows * cols] -> [ceil(rows / size), ceil(cols / size), n]: `reduce` over the pixels of each tile that lie in the image."""
    n = a.shape[0]
    ty, tx = (rows + size - 1) // size, (cols + size - 1) // size
    full = np.full((n, ty * size, tx * size), fill, np.float32)
    full[:, :rows, :cols] = a.reshape(n, rows, cols)
    return np.ascontiguousarray(reduce(full.reshape(n, ty, size, tx, size), axis=(2, 4)).transpose(1, 2, 0))


def products(depth, Ts, cam, cols, rows):
    """depth uint16[n, rows * cols] as k_prepare reads it (re-projected already on the warped path), Ts float64[n, 4, 4]."""
    depth = np.asarray(depth, np.uint16).reshape(-1, rows * cols)
    n = depth.shape[0]
    assert 1 <= n <= BATCH
    Ts = np.asarray(Ts, np.float64).reshape(n, 4, 4)
    sc = scale_depth(depth, cam, cols, rows)
    scaled = np.zeros((n, rows * cols + PAD), np.float32)
    scaled[:, :rows * cols] = sc
    usable = np.where(sc > np.float32(0.001), sc, np.float32(0.0)).astype(np.float32)
    masks, out_of_range = {}, 0
    for f in range(n):
        k = unit_keys(depth[f], Ts[f], cam, cols, rows)
        out_of_range += int((k == -2).sum())
        for key in np.unique(k[k >= 0]):
            masks[int(key)] = masks.get(int(key), 0) | (1 << f)
    keys = np.array(sorted(masks), np.int32)
    return dict(scaled=scaled, tile_max=_tiles(sc, cols, rows, TILE, np.float32(0.0), np.max),
                tile_lo=_tiles(usable, cols, rows, TILE, BIG, np.min), tile_lo_fine=_tiles(usable, cols, rows, FINE, BIG, np.min),
                keys=keys, masks=np.array([masks[int(k)] for k in keys], np.uint64), out_of_range=out_of_range)
