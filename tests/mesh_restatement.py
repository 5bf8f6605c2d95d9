"""numpy restatement of er_tsdf_extract_mesh_indexed (include/er_hip.h) over {key: (sdf[262144], weight[262144])}.

The cells are enumerated as test_tsdf_gpu._mesh_oracle enumerates them (units by ascending key, cells in i, j, k order, triangles in table
order; a cell is valid iff its eight voxels are observed, a corner is inside iff sdf < 0), but every triangle corner carries the lattice
EDGE it sits on -- the edge's lower voxel on the whole 512 x 64 lattice and its axis -- next to its position.  The vertices are the unique
edges sorted by (unit key of the lower voxel, i, j, k, axis); a triangle is three positions in that list.  A vertex is never keyed by its
coordinates."""
import ctypes as C

import numpy as np

UL = 3.0 / 512.0


def _table():
    from elasticreconstruction_amd import _ffi
    tab = np.zeros(256 * 16, np.uint8)
    assert _ffi.lib().er_mc_table(tab.ctypes.data_as(C.c_void_p)) == 0
    return tab.reshape(256, 16)


def _padded(units, key):
    """The unit's 64^3 voxels with the first layer of its +x / +y / +z neighbours (and their combinations): sdf and weight [65, 65, 65];
    a voxel of a unit that does not exist or lies outside the 512-unit lattice is (0, 0) = unobserved."""
    xi, yi, zi = key >> 18, (key >> 9) & 511, key & 511
    S = np.zeros((65, 65, 65), np.float32)
    W = np.zeros((65, 65, 65), np.float32)
    for dx in range(2):
        for dy in range(2):
            for dz in range(2):
                k2 = key + dx * 512 * 512 + dy * 512 + dz
                if k2 not in units or xi + dx > 511 or yi + dy > 511 or zi + dz > 511:
                    continue
                s, w = (a.reshape(64, 64, 64) for a in units[k2])
                to = tuple(slice(64, 65) if d else slice(0, 64) for d in (dx, dy, dz))
                src = tuple(slice(0, 1) if d else slice(0, 64) for d in (dx, dy, dz))
                S[to], W[to] = s[src], w[src]
    return S, W


def edge_code(g, axis):
    """Sort key of the edge with lower voxel g = [n, 3] (0-based index on the whole lattice) and axis [n]: unit key of the voxel, then its
    i, j, k inside the unit, then the axis."""
    g = np.asarray(g, np.int64)
    key = (g[:, 0] >> 6) << 18 | (g[:, 1] >> 6) << 9 | (g[:, 2] >> 6)
    return (((key * 64 + (g[:, 0] & 63)) * 64 + (g[:, 1] & 63)) * 64 + (g[:, 2] & 63)) * 3 + np.asarray(axis, np.int64)


def indexed_mesh(units):
    """-> (verts float32[n, 4] = x y z axis, tris int32[m, 3], codes int64[n] = edge_code of every vertex)."""
    tab = _table()
    ulf = np.float32(UL)
    codes, pos, axes = [], [], []
    for key in sorted(units):
        xi, yi, zi = key >> 18, (key >> 9) & 511, key & 511
        S, W = _padded(units, key)
        corner = lambda A, c: A[(c & 1):(c & 1) + 64, ((c >> 1) & 1):((c >> 1) & 1) + 64, (c >> 2):(c >> 2) + 64]
        valid = np.ones((64, 64, 64), bool)
        case = np.zeros((64, 64, 64), np.int32)
        for c in range(8):
            valid &= corner(W, c) != 0
            case |= (corner(S, c) < 0).astype(np.int32) << c
        ntri = (tab[case][..., 0::3][..., :5] != 255).sum(-1) * valid
        cells = np.argwhere(ntri > 0)                                        # C order = i, j, k order
        if not len(cells):
            continue
        ci, cj, ck = cells.T
        cs, nt = case[ci, cj, ck], ntri[ci, cj, ck]
        G = [((np.arange(66) + (q - 256) * 64).astype(np.float64) * UL).astype(np.float32) for q in (xi, yi, zi)]
        P = np.zeros((len(cells), 15, 3), np.float32)
        E = np.zeros((len(cells), 15), np.int64)
        A = np.zeros((len(cells), 15), np.int64)
        for t in range(15):
            live = 3 * nt > t
            e = np.where(live, tab[cs, t].astype(np.int32), 0)
            axis, u, v = e >> 2, e & 1, (e >> 1) & 1
            a0 = np.where(axis == 0, 0, u)
            b0 = np.where(axis == 1, 0, np.where(axis == 0, u, v))
            c0 = np.where(axis == 2, 0, v)
            li, lj, lk = ci + a0, cj + b0, ck + c0
            fl, fh = S[li, lj, lk], S[li + (axis == 0), lj + (axis == 1), lk + (axis == 2)]
            with np.errstate(divide="ignore", invalid="ignore"):
                add = ((fl / (fl - fh)).astype(np.float32) * ulf).astype(np.float32)
            p = np.stack([G[0][li], G[1][lj], G[2][lk]], 1)
            for q in range(3):
                p[:, q] = np.where(axis == q, (p[:, q] + add).astype(np.float32), p[:, q])
            P[:, t] = p
            E[:, t] = edge_code(np.stack([li + xi * 64, lj + yi * 64, lk + zi * 64], 1), axis)
            A[:, t] = axis
        keep = np.arange(15)[None, :] < (3 * nt)[:, None]
        codes.append(E[keep])
        pos.append(P[keep])
        axes.append(A[keep])
    if not codes:
        return np.zeros((0, 4), np.float32), np.zeros((0, 3), np.int32), np.zeros(0, np.int64)
    codes, pos, axes = np.concatenate(codes), np.concatenate(pos), np.concatenate(axes)
    uniq, first, inv = np.unique(codes, return_index=True, return_inverse=True)
    verts = np.concatenate([pos[first], axes[first][:, None].astype(np.float32)], 1).astype(np.float32)
    # whichever cell asks, an edge gives the same bits (the position is taken from the edge's lower end)
    assert np.array_equal(verts[inv.reshape(-1), :3].view(np.uint32), pos.view(np.uint32))
    assert len(uniq) < 2 ** 31
    return verts, inv.reshape(-1, 3).astype(np.int32), uniq


def crossed_observed_edges(units):
    """edge_code of every lattice edge whose two voxels are observed and (F_L < 0) != (F_H < 0): the superset the mesh vertices are drawn
    from (a vertex also needs one complete cell around its edge)."""
    out = []
    for key in sorted(units):
        xi, yi, zi = key >> 18, (key >> 9) & 511, key & 511
        S, W = _padded(units, key)
        for axis in range(3):
            hi = tuple(slice(1, 65) if q == axis else slice(0, 64) for q in range(3))
            lo = (slice(0, 64),) * 3
            cross = (W[lo] != 0) & (W[hi] != 0) & ((S[lo] < 0) != (S[hi] < 0))
            g = np.argwhere(cross) + np.array([xi * 64, yi * 64, zi * 64])
            out.append(edge_code(g, np.full(len(g), axis)))
    return np.sort(np.concatenate(out)) if out else np.zeros(0, np.int64)
