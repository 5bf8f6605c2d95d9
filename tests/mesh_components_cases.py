"""The index lists and crafted volumes that tests/test_mesh_components_cpu.py and tests/test_mesh_components_gpu.py share: the smallest shapes
at which a kernel of csrc/er_mesh_cc.hip can still go wrong (wave and workgroup edges of 64 and 256; one block and several; one word taking
every atomic), and voxels planted in observed free space, each of which marching cubes turns into a small closed shell."""
import numpy as np

KEY = 256 << 18 | 256 << 9 | 256
DX, DY, DZ = 512 * 512, 512, 1
N_STRIP = 65537


def strip(p):
    """Triangles (p[t], p[t + 1], p[t + 2]): one component whatever the permutation p."""
    p = np.asarray(p, np.int32)
    return np.stack([p[:-2], p[1:-1], p[2:]], 1)


def bit_reversed(n):
    """The permutation of 0 .. n - 1 that sorts the indices by their bit-reversed value."""
    bits = max(1, int(n - 1).bit_length())
    i = np.arange(n, dtype=np.int64)
    rev = np.zeros(n, np.int64)
    for b in range(bits):
        rev |= ((i >> b) & 1) << (bits - 1 - b)
    return np.argsort(rev, kind="stable").astype(np.int32)


def zig_zag(n):
    p = np.empty(n, np.int32)
    p[0::2] = np.arange((n + 1) // 2)
    p[1::2] = n - 1 - np.arange(n // 2)
    return p


def strips():
    """name -> (tris, nv): 65 537 triangles each, every label 0."""
    nv = N_STRIP + 2
    ident = np.arange(nv, dtype=np.int32)
    perms = {"identity": ident, "reversed": ident[::-1].copy(), "bit-reversed": bit_reversed(nv),
             "seeded permutation": np.random.default_rng(20240607).permutation(nv).astype(np.int32), "zig-zag": zig_zag(nv)}
    return {name: (strip(p), nv) for name, p in perms.items()}


def disjoint(n, seed=None):
    """n triangles without a common vertex; with a seed the vertices are shuffled."""
    v = np.arange(3 * n, dtype=np.int32)
    if seed is not None:
        v = np.random.default_rng(seed).permutation(3 * n).astype(np.int32)
    return v.reshape(n, 3), 3 * n


def fan(n=65536):
    """n triangles (hub, 2 i, 2 i + 1) around a hub whose index is nv - 1: they meet only in the hub, so every hook of the first round goes to
    the hub's word."""
    i = np.arange(n, dtype=np.int32)
    nv = 2 * n + 1
    return np.stack([np.full(n, nv - 1, np.int32), 2 * i, 2 * i + 1], 1), nv


def interleaved(n=3000):
    """Two strips, one over the even and one over the odd vertices, their triangles alternating in the list: labels 0 and 1."""
    a, b = strip(2 * np.arange(n + 2)), strip(2 * np.arange(n + 2) + 1)
    out = np.empty((2 * n, 3), np.int32)
    out[0::2], out[1::2] = a, b
    return out, 2 * (n + 2)


def odd_triangles():
    """Triangles that repeat a vertex, duplicates, and a component that only a degenerate triangle holds together."""
    t = np.array([[5, 5, 7], [7, 9, 9], [2, 2, 2], [1, 3, 4], [1, 3, 4], [4, 3, 1], [9, 11, 11], [0, 6, 6], [6, 6, 8], [8, 10, 12], [8, 10, 12]], np.int32)
    return t, 14                                             # 13 is named by nobody


def unused_vertices():
    """Vertices that no triangle names at index 0, in the middle and at nv - 1."""
    t = np.array([[1, 2, 3], [3, 4, 5], [300, 301, 302], [302, 5, 301], [598, 597, 596]], np.int32)
    return t, 600


def index_lists():
    """name -> (tris int32[nt, 3], nv) of every list case."""
    cases = {"no triangle": (np.zeros((0, 3), np.int32), 5), "one triangle": (np.array([[2, 0, 1]], np.int32), 3),
             "two triangles": (np.array([[0, 1, 2], [3, 2, 4]], np.int32), 6)}
    for n in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        cases["%d disjoint triangles" % n] = disjoint(n, seed=n if n % 2 else None)
    for name, c in strips().items():
        cases["strip, " + name] = c
    cases["fan around the last vertex"] = fan()
    cases["two interleaved strips"] = interleaved()
    cases["duplicate and degenerate triangles"] = odd_triangles()
    cases["unused vertices"] = unused_vertices()
    return cases


# ---- crafted volumes --------------------------------------------------------------------------------------------------------------------

def free_unit():
    """Observed free space: sdf +1, weight 1."""
    return np.ones(64 ** 3, np.float32), np.ones(64 ** 3, np.float32)


def plant(units, key, voxels, value=-0.5):
    """Sets the sdf of the listed voxels (i, j, k) of an existing unit."""
    s = units[key][0].reshape(64, 64, 64)
    for i, j, k in voxels:
        s[i, j, k] = np.float32(value)


def planted(voxels, with_x_neighbour=False, neighbour_voxels=()):
    units = {KEY: free_unit()}
    plant(units, KEY, voxels)
    if with_x_neighbour:
        units[KEY + DX] = free_unit()
        plant(units, KEY + DX, neighbour_voxels)
    return units
