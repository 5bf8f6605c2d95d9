"""The voxel-grid, normal and FPFH kernels of csrc/er_fpfh.hip (k_vox_keys / heads / starts / mean, k_fp_normals, k_fp_spfh, k_fp_fpfh) and the
temporary radius grid they build, at the shape edges of tests/fpfh_cases.py, against tests/fpfh_restatement.py.  Every stage gets the
restatement's float32 output of the stage before it, so one wrong stage cannot hide another.  The bars are those of tests/test_fpfh_gpu.py:
voxel rows within 2^-23 max(1, max|input|), counts and the NaN mask exact, normals within 1e-6 rad, the 33 integer counts exact (no fixture
has a pair near a bin edge or a normal to leave out: tests/test_fpfh_cases_cpu.py), descriptors within one float32 step.

Observed on one MI355X (printed by the tests; nothing is asserted against these figures):
  voxel grid   every output row of every fixture bit-identical to the restatement, points and normals (sizes 4800 of 4800 rows, clumps 17 of
               17, star 168 of 168, exact 7 of 7, coarse 17 of 17, voxels 22 + 1 + 257 + 201 + 257 + 40 + 22 of as many)
  normals      worst angle to the restatement 1.11e-16 rad (star); 0 rad in sizes, clumps, exact and coarse: the float32 normals are the same bits
  descriptors  worst descriptor step 0: all 457677 + 33957 + 5544 + 495 + 4950 values bit-identical to the restatement, and the permuted runs
               bit-identical to the unpermuted ones
  wall time    this file 3.65 s for its 29 tests (5.4 s with the interpreter's start); tests/test_fpfh_gpu.py, unchanged since the parent
               commit, 8.61 s for its 12 tests (10.7 s) on the same machine
"""
import numpy as np
import pytest

import fpfh_cases as fc
import fpfh_restatement as fr
from elasticreconstruction_amd.icp import Cloud, fpfh

pytestmark = pytest.mark.gpu
CELL = fc.CELL


def angle(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(axis=1))


def steps(a, b):
    """The distance of two float32 arrays of non-negative values in float32 steps."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def device_normals(x, nrm, r):
    """(normals, counts, the cloud read back) of er_cloud_estimate_normals."""
    c = Cloud(x, nrm, CELL)
    e, cnt = c.estimate_normals(r, want_counts=True)
    gx, gn = e.read()
    back = c.read()
    c.close()
    e.close()
    return gx, gn, cnt, back


def device_fpfh(x, nrm, r):
    """(descriptors, the 33 integer counts, nn) of er_fpfh_estimate."""
    c = Cloud(x, nrm, CELL)
    f, counts, nn = fpfh(c, r, want_counts=True)
    feat = f.read()
    assert (f.n, f.dim) == (len(x), 33) and feat.shape == (len(x), 33)
    c.close()
    f.close()
    return feat, counts, nn


# ---- voxel grid ------------------------------------------------------------------------------------------------------------------
VOXEL_CASES = ("voxels-a-faces", "voxels-b-one-cell", "voxels-c-own-cells", "voxels-d-segment-200", "voxels-d-segment-256", "voxels-e-column",
               "voxels-f-negative")


@pytest.mark.parametrize("family", fc.FEATURE_FAMILIES + VOXEL_CASES)          # the clouds of a feature family together, every voxel fixture alone
def test_shapes_voxel_grid(gpu, family):
    same = rows = 0
    if family == VOXEL_CASES[0]:
        assert [c.name for c in fc.cases("voxels")] == list(VOXEL_CASES)
    for c in (fc.cases(family) if family in fc.FAMILIES else [fc.case(family)]):
        if not c.voxel:
            continue
        rx, rn, key = fc.restated(c)["vox"]
        src = Cloud(c.xyz, c.nrm, CELL)
        d = src.voxel_grid(fc.LEAF, CELL)
        gx, gn = d.read()
        src.close()
        d.close()
        assert d.n == len(rx) == len(gx), (c.name, d.n, len(rx))
        tol_x = 2.0 ** -23 * max(1.0, float(np.abs(c.xyz).max()))
        tol_n = 2.0 ** -23 * max(1.0, float(np.abs(c.nrm).max()))
        ex = np.abs(gx.astype(np.float64) - rx).max()
        en = np.abs(gn.astype(np.float64) - rn).max()
        ident = int(((gx.view(np.uint32) == rx.view(np.uint32)).all(axis=1) & (gn.view(np.uint32) == rn.view(np.uint32)).all(axis=1)).sum())
        same, rows = same + ident, rows + len(rx)
        print("voxel grid %s: %d -> %d points, worst |dx| %.3g (bound %.3g), worst |dn| %.3g (bound %.3g), %d bit-identical rows"
              % (c.name, len(c.xyz), d.n, ex, tol_x, en, tol_n, ident))
        assert ex <= tol_x and en <= tol_n, c.name
        # ascending key order: output k lies in cell k of the sorted key list (wherever the restatement's own rounded mean does)
        own = fc.voxel_key_of(rx, c.xyz) == key
        assert np.array_equal(fc.voxel_key_of(gx, c.xyz)[own], key[own]), c.name
        if "m" in c.facts:
            assert d.n == c.facts["m"]
    print("voxel grid %s: %d of %d rows bit-identical" % (family, same, rows))


def test_shapes_voxel_counts_stated_literally(gpu):
    for name, m in (("voxels-b-one-cell", 1), ("voxels-c-own-cells", 257), ("voxels-d-segment-200", 201), ("voxels-d-segment-256", 257)):
        c = fc.case(name)
        src = Cloud(c.xyz, c.nrm, CELL)
        d = src.voxel_grid(fc.LEAF, CELL)
        assert d.n == m, (name, d.n)
        if m == 257 and name.startswith("voxels-c"):
            gx, gn = d.read()                                        # a single member comes back as it is, in key order
            o = np.argsort(fr.voxel_cells(c.xyz, fc.LEAF)[0], kind="stable")
            assert np.array_equal(gx.view(np.uint32), c.xyz[o].view(np.uint32)) and np.array_equal(gn.view(np.uint32), c.nrm[o].view(np.uint32))
        src.close()
        d.close()


# ---- normals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", fc.FEATURE_FAMILIES)
def test_shapes_normals(gpu, family):
    worst = 0.0
    for c in fc.cases(family):
        p = fc.restated(c)
        gx, gn, cnt, (bx, bn) = device_normals(c.xyz, c.nrm, c.r_normal)
        assert np.array_equal(cnt, p["n_counts"]), (c.name, np.nonzero(cnt != p["n_counts"])[0][:8])
        few = p["n_counts"] < 3
        assert np.array_equal(np.isnan(gn).any(axis=1), few) and np.array_equal(np.isnan(gn).all(axis=1), few), c.name
        assert np.array_equal(gx.view(np.uint32), c.xyz.view(np.uint32))                      # the same points
        assert np.array_equal(bx.view(np.uint32), c.xyz.view(np.uint32)) and np.array_equal(bn.view(np.uint32), c.nrm.view(np.uint32))
        if (~few).any():
            a = angle(gn[~few], p["normals"][~few])
            worst = max(worst, float(a.max()))
            assert a.max() <= 1e-6, (c.name, a.max())                                         # (an opposite sign would be an angle of pi)
            assert (np.abs(np.linalg.norm(gn[~few].astype(np.float64), axis=1) - 1.0) < 1e-6).all(), c.name
    print("normals %s: worst angle to the restatement %.3g rad" % (family, worst))


# ---- SPFH and FPFH ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", fc.FEATURE_FAMILIES)
def test_shapes_spfh_counts_and_descriptors(gpu, family):
    worst = apart = values = 0
    for c in fc.cases(family):
        p = fc.restated(c)
        feat, counts, nn = device_fpfh(c.xyz, p["feat_nrm"], c.r_feature)
        assert np.array_equal(nn, p["nn"]), (c.name, np.nonzero(nn != p["nn"])[0][:8])
        assert np.array_equal(counts, p["counts"]), (c.name, np.nonzero((counts != p["counts"]).any(axis=1))[0][:8])
        assert np.isfinite(feat).all() and (feat >= 0).all(), c.name
        d = steps(feat, p["feat"])
        worst, apart, values = max(worst, int(d.max())), apart + int((d > 0).sum()), values + d.size
        assert d.max() <= 1, (c.name, int(d.max()))
        assert not feat[~np.isfinite(p["feat_nrm"]).all(axis=1)].any(), c.name               # a NaN normal: a zero row
    print("FPFH %s: descriptors at most %d float32 steps from the restatement, %d of %d values not bit-identical" % (family, worst, apart, values))


# ---- what each fixture was built for, stated literally --------------------------------------------------------------------------
def test_shapes_clumps_every_point_counts_all_k(gpu):
    for c in fc.cases("clumps"):
        k, p = c.facts["k"], fc.restated(c)
        _, _, cnt, _ = device_normals(c.xyz, c.nrm, c.r_normal)
        _, _, nn = device_fpfh(c.xyz, p["feat_nrm"], c.r_feature)
        assert (cnt == k).all() and (nn == k).all(), (k, cnt.min(), cnt.max(), nn.min(), nn.max())


def test_shapes_star_centre_counts_its_26_cells(gpu):
    for c in fc.cases("star"):
        want = 27 if c.name.endswith("inner") else 1
        _, counts, nn = device_fpfh(c.xyz, c.nrm, c.r_feature)
        assert nn[0] == want == c.facts["centre_nn"], (c.name, nn[0])
        # the normals kernel at r itself: the count only (the centre's scatter matrix is a multiple of the identity there)
        _, _, cnt, _ = device_normals(c.xyz, c.nrm, c.facts["r"])
        assert cnt[0] == want and np.array_equal(cnt, fc.restated(c)["nn"]), (c.name, cnt[0])
        if want == 27:
            assert counts[0, :11].sum() == 26                                                 # every one of the 26 pairs made it into the histogram


def test_shapes_exact_radius_is_excluded(gpu):
    c = fc.case("exact")
    p = fc.restated(c)
    _, _, cnt, _ = device_normals(c.xyz, c.nrm, c.r_normal)
    _, _, nn = device_fpfh(c.xyz, p["feat_nrm"], c.r_feature)
    assert list(nn[:3]) == [14, 1, 2] == list(cnt[:3]) and list(nn) == c.facts["nn"] == list(cnt)


def test_shapes_coarse_doubled_cell(gpu):
    c = fc.case("coarse")
    p = fc.restated(c)
    _, _, cnt, _ = device_normals(c.xyz, c.nrm, c.r_normal)
    _, _, nn = device_fpfh(c.xyz, p["feat_nrm"], c.r_feature)
    assert list(nn[148:]) == [1, 1] == list(cnt[148:])                                        # one doubled cell, 0.015 apart: no neighbours
    assert list(nn) == c.facts["nn"] == list(cnt)


# ---- order independence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sizes-n257-t0", "clumps-k129"])
def test_shapes_results_do_not_depend_on_the_input_order(gpu, name):
    c = fc.case(name)
    p = fc.restated(c)
    perm = np.random.default_rng(17).permutation(len(c.xyz))
    _, gn, cnt, _ = device_normals(c.xyz, c.nrm, c.r_normal)
    _, gn2, cnt2, _ = device_normals(c.xyz[perm], c.nrm[perm], c.r_normal)
    assert np.array_equal(cnt2, cnt[perm]) and np.array_equal(np.isnan(gn2), np.isnan(gn)[perm])
    ok = ~np.isnan(gn2).any(axis=1)
    assert angle(gn2[ok], gn[perm][ok]).max() <= 2e-6 if ok.any() else True
    fn = np.ascontiguousarray(p["feat_nrm"])
    feat, counts, nn = device_fpfh(c.xyz, fn, c.r_feature)
    feat2, counts2, nn2 = device_fpfh(c.xyz[perm], fn[perm], c.r_feature)
    assert np.array_equal(nn2, nn[perm]) and np.array_equal(counts2, counts[perm])
    d = steps(feat2, feat[perm])
    print("%s permuted: descriptors at most %d float32 steps apart" % (name, int(d.max())))
    assert d.max() <= 2
