"""Oriented surface extraction (er_tsdf_extract_oriented / er_cloud_create_from_tsdf), the part that needs no GPU: the numpy restatement of
the normal rule -- the statement the kernel is compared with bit for bit in tests/test_oriented_gpu.py -- checked against the independent
statement the tree already has (synth.kinfu_fragment's dense-grid gradient), and the two entry points at the C ABI."""
import ctypes as C
import os

import numpy as np

from elasticreconstruction_amd import _ffi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UL = 3.0 / 512.0                          # the library's kUnitLength (double)
LATTICE = 512 * 64                        # voxels per axis of the whole unit lattice


def nearest_voxel(pts):
    """v = rint((double)p / ul) per component (round half to even), in the fragment's voxel coordinates (voxel 0 = unit index 256)."""
    return np.rint(np.asarray(pts, np.float32)[:, :3].astype(np.float64) / UL).astype(np.int64)


def oriented_oracle(units, pts):
    """numpy restatement of the normal er_tsdf_extract_oriented gives each point of er_tsdf_extract_surface's list.
    units: {key: (sdf[262144], weight[262144])}, pts: float32 [n, >= 3].  The nearest voxel v and its six neighbours must all be observed
    (weight != 0; a voxel of a unit that is not in `units` or outside the 512-unit lattice is not); g_a = S[v + e_a] - S[v - e_a],
    n2 = (gx gx + gy gy) + gz gz, n = g / sqrt(n2), every float32 operation rounded on its own; NaN in all three components otherwise.
    Returns float32 [n, 3]."""
    keys = np.array(sorted(units), np.int64)
    S = np.stack([np.asarray(units[int(k)][0], np.float32).reshape(-1) for k in keys]) if len(keys) else np.zeros((0, 64 ** 3), np.float32)
    W = np.stack([np.asarray(units[int(k)][1], np.float32).reshape(-1) != 0 for k in keys]) if len(keys) else np.zeros((0, 64 ** 3), bool)
    v = nearest_voxel(pts) + 256 * 64                                           # on the 0-based lattice
    n = v.shape[0]

    def fetch(g):
        inside = ((g >= 0) & (g < LATTICE)).all(axis=1)
        gc = np.where(inside[:, None], g, 0)
        key = (gc[:, 0] >> 6) << 18 | (gc[:, 1] >> 6) << 9 | (gc[:, 2] >> 6)
        loc = (gc[:, 0] & 63) * 4096 + (gc[:, 1] & 63) * 64 + (gc[:, 2] & 63)
        slot = np.searchsorted(keys, key)
        slot_c = np.minimum(slot, max(len(keys) - 1, 0))
        have = inside & (slot < len(keys)) & (keys[slot_c] == key if len(keys) else np.zeros(n, bool))
        s, w = np.zeros(n, np.float32), np.zeros(n, bool)
        s[have], w[have] = S[slot_c[have], loc[have]], W[slot_c[have], loc[have]]
        return s, w

    _, seen = fetch(v)
    g = np.zeros((n, 3), np.float32)
    for a in range(3):
        e = np.zeros(3, np.int64)
        e[a] = 1
        (sh, wh), (sl, wl) = fetch(v + e), fetch(v - e)
        seen = seen & wh & wl
        g[:, a] = sh - sl                                                        # float32 - float32 -> float32
    n2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
    nrm = np.sqrt(n2)
    assert n2.dtype == np.float32 and nrm.dtype == np.float32
    ok = seen & (nrm > 0)
    out = np.full((n, 3), np.nan, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = g / nrm[:, None]
    out[ok] = q[ok]
    return out


def compare_with_synth(pts, nrm, x_synth, n_synth, length=3.0):
    """The comparison of a restatement / the kernel (pts [n, 4], nrm [n, 3] over the WHOLE volume) with synth.kinfu_fragment(..., target_points =
    10**9, density = "tsdf") of the same volume (x_synth, n_synth: the rows inside the cube, in order).  Returns the figures it asserts on."""
    P = pts[:, :3]
    inside = ((P >= np.float32(0.0)) & (P < np.float32(length))).all(axis=1)
    x, n = P[inside], nrm[inside]
    assert x.shape == x_synth.shape, (x.shape, x_synth.shape)
    assert np.array_equal(x.view(np.uint32), x_synth.view(np.uint32)), "the points differ"
    v = nearest_voxel(x)
    sub = ((v >= 1) & (v <= 510)).all(axis=1)                                   # synth's dense grid ends at the cube, the lattice does not
    nan_a, nan_s = np.isnan(n), np.isnan(n_synth)
    assert np.array_equal(nan_a.any(axis=1), nan_a.all(axis=1)), "a NaN normal must be NaN in all three components"
    assert np.array_equal(nan_a[sub], nan_s[sub]), "NaN patterns differ on %d rows whose nearest voxel is in [1, 510]^3" % int((nan_a[sub] != nan_s[sub]).any(axis=1).sum())
    fin_a, fin_s = ~nan_a.any(axis=1), ~nan_s.any(axis=1)
    both = fin_a & fin_s
    worst = float(np.abs(n[both].astype(np.float64) - n_synth[both].astype(np.float64)).max()) if both.any() else 0.0
    only_a = fin_a & ~fin_s
    figures = dict(crossings=int(pts.shape[0]), inside=int(inside.sum()), outside_sub=int((~sub).sum()), finite_only_here=int(only_a.sum()),
                   finite_both=float(both.mean()), max_abs_diff=worst, bit_equal=float((n[both].view(np.uint32) == n_synth[both].view(np.uint32)).all(axis=1).mean()))
    print("oriented vs synth.kinfu_fragment:", figures)
    assert not (only_a & sub).any(), "finite here, NaN in synth, although the nearest voxel is inside synth's grid"
    assert not (fin_s & ~fin_a).any(), "finite in synth, NaN here"
    # components are <= 1 and the two statements differ by a handful of float32 roundings of 2^-24 each (torch's norm): 1e-6 is about 8 of them
    assert worst <= 1e-6, worst
    assert both.mean() >= 0.90, "only %.1f %% of the rows inside the cube have a finite normal in both statements" % (100 * both.mean())
    return figures


def _capturing_volume():
    """test_round5_helpers' oracle-backed stand-in for TSDFVolume that remembers its units and its point list past close()."""
    from test_round5_helpers import _OracleBackedVolume

    class Capturing(_OracleBackedVolume):
        last = None

        def extract_surface(self):
            self.units = {int(k): self.o.read_unit(k) for k in self.o.unit_keys()}
            self.points = super().extract_surface()
            Capturing.last = self
            return self.points
    return Capturing


def test_normal_rule_restatement_agrees_with_the_dense_grid_statement(monkeypatch):
    """oriented_oracle against synth.kinfu_fragment on the same CPU-backed volume (3 noisy frames of sweep 3 of 50) and the same points."""
    from elasticreconstruction_amd import tsdf
    cls = _capturing_volume()
    monkeypatch.setattr(tsdf, "TSDFVolume", cls)
    x, n, F, st = synth.kinfu_fragment(3, 50, target_points=10 ** 9, frames=3, noise_mm=2.0, density="tsdf", device="cpu")
    vol = cls.last
    assert vol is not None and vol.points.shape[0] == st["zero_crossings"] > 100000
    got = oriented_oracle(vol.units, vol.points)
    fig = compare_with_synth(vol.points, got, x, n)
    assert fig["inside"] == st["inside_cube"] == x.shape[0]
    # the lattice goes on where synth's grid ends: some of the rows at the cube's faces do get a normal here
    assert fig["outside_sub"] > 0 and fig["finite_only_here"] > 0


def test_restatement_on_a_hand_made_unit():
    """A plane at x = 10.25 voxels through one unit (sdf linear in x): +x normals exactly; NaN where the nearest voxel lies on the unit's border
    (a neighbour is in a unit that does not exist) and where one of the seven voxels is unobserved."""
    from test_tsdf_gpu import _surface_oracle
    i = np.arange(64, dtype=np.float32)
    sdf = np.broadcast_to(((i - np.float32(10.25)) * np.float32(0.125))[:, None, None], (64, 64, 64)).astype(np.float32).copy()
    w = np.ones((64, 64, 64), np.float32)
    w[9, 30, 30] = 0                       # the -x neighbour of nearest voxel (10, 30, 30); the crossing between voxels 10 and 11 stays
    w[10, 20, 20] = 0                      # removes the crossing of row (20, 20) and is a y / z neighbour of four other nearest voxels
    key = 256 << 18 | 256 << 9 | 256
    units = {key: (sdf.reshape(-1), w.reshape(-1))}
    pts = _surface_oracle(units)
    assert pts.shape[0] == 64 * 64 - 1 and (pts[:, 3] == 0).all()
    v = nearest_voxel(pts)
    assert (v[:, 0] == 10).all()                                               # 10.25 rounds to the edge's lower voxel
    n = oriented_oracle(units, pts)
    y, z = v[:, 1], v[:, 2]
    want_nan = (y == 0) | (y == 63) | (z == 0) | (z == 63) | ((y == 30) & (z == 30)) | ((np.abs(y - 20) + np.abs(z - 20)) == 1)
    nan = np.isnan(n).all(axis=1)
    assert np.array_equal(np.isnan(n).any(axis=1), nan) and np.array_equal(nan, want_nan)
    assert np.array_equal(n[~nan], np.tile(np.array([1, 0, 0], np.float32), (int((~nan).sum()), 1)))
    # the point above the mid-point of its edge takes the UPPER voxel: plane at 10.75
    sdf2 = np.broadcast_to(((i - np.float32(10.75)) * np.float32(0.125))[:, None, None], (64, 64, 64)).astype(np.float32).copy()
    pts2 = _surface_oracle({key: (sdf2.reshape(-1), np.ones(64 ** 3, np.float32))})
    assert (nearest_voxel(pts2)[:, 0] == 11).all()


def test_new_entry_points_are_declared_bound_and_refuse_to_run_without_a_device():
    hdr = open(os.path.join(ROOT, "include", "er_hip.h")).read()
    L = _ffi.lib()
    for name in ("er_tsdf_extract_oriented", "er_cloud_create_from_tsdf"):
        assert name + "(" in hdr and name in _ffi.SYMBOLS and hasattr(L, name)
    import torch
    n, h, m = C.c_long(-1), C.c_void_p(), C.c_int(-1)
    rc = L.er_tsdf_extract_oriented(None, None, None, 0, C.byref(n))
    msg = L.er_last_error().decode()
    assert rc != 0 and "er_tsdf_extract_oriented" in msg
    if not torch.cuda.is_available():
        assert "no HIP device" in msg, msg
    rc = L.er_cloud_create_from_tsdf(None, C.c_float(3.0), C.c_float(0.03), C.byref(h), C.byref(m))
    msg = L.er_last_error().decode()
    assert rc != 0 and "er_cloud_create_from_tsdf" in msg and not h.value
    if not torch.cuda.is_available():
        assert "no HIP device" in msg, msg
