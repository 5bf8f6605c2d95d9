"""The fixtures of tests/fpfh_cases.py, without a GPU: their own assertions hold, the restatement's neighbour search agrees with the quadratic
float32 loop on every one of them, and the conditions tests/test_fpfh_shapes_gpu.py relies on are met -- no SPFH pair within DELTA of a bin
edge and no normal with three or more neighbours that would have to be left out of the angle comparison.  These are conditions on the
fixtures, not measurements: a seed that breaks one is changed, the cap is not."""
import numpy as np
import pytest

import fpfh_cases as fc
import fpfh_restatement as fr


@pytest.mark.parametrize("family", sorted(fc.FAMILIES))
def test_fixture_builds_and_its_own_assertions_hold(family):
    cs = fc.cases(family)                                             # the assertions inside the builders
    assert len({c.name for c in cs}) == len(cs)
    for c in cs:
        assert c.xyz.dtype == np.float32 and c.nrm.dtype == np.float32 and np.isfinite(c.xyz).all() and np.isfinite(c.nrm).all()
        assert 1 <= len(c.xyz) <= 1100
    expect = {"sizes": 2 * len(fc.SIZES_N) * len(fc.SIZES_T), "clumps": len(fc.CLUMPS_K), "star": 2 * len(fc.STAR_R), "exact": 1, "coarse": 1,
              "voxels": 7}
    assert len(cs) == expect[family]


def test_sizes_are_the_named_counts_and_small_ones_have_lone_points():
    raw = [c for c in fc.cases("sizes") if c.voxel]
    assert sorted({len(c.xyz) for c in raw}) == sorted(fc.SIZES_N) and {c.facts["t"] for c in raw} == set(fc.SIZES_T)
    for c in raw:
        assert len(c.xyz) == c.facts["n"]
        if c.facts["n"] <= 65:
            few = fc.restated(c)["n_counts"] < 3                     # a large share alone (the NaN mask, the zero rows) ...
            assert few.mean() >= 0.25 and (c.facts["n"] < 63 or not few.all()), c.name      # ... and, from 63 on, both sides of the mask
        if c.facts["n"] >= 1023:
            assert (fc.restated(c)["n_counts"] >= 3).all(), c.name
    # the same patch at the three translations keeps its voxel count only by accident; what is pinned is that a large offset is present
    assert max(float(np.abs(c.xyz).max()) for c in raw) > 40.0


@pytest.mark.parametrize("family", fc.FEATURE_FAMILIES)
def test_neighbour_search_of_the_restatement_equals_the_quadratic_loop(family):
    for c in fc.cases(family):
        for r in sorted({c.r_normal, c.r_feature}):
            a, b = fr.neighbour_pairs(c.xyz, r), fr.neighbours_brute(c.xyz, r)
            assert all(np.array_equal(p, q) for p, q in zip(a, b)), (c.name, r)


@pytest.mark.parametrize("family", fc.FEATURE_FAMILIES)
def test_exclusion_caps_are_zero(family):
    worst_gap, worst_dot, pairs = np.inf, np.inf, 0
    for c in fc.cases(family):
        p = fc.restated(c)
        assert p["edge"].sum() == 0, "%s: %d pairs near a bin edge" % (c.name, int(p["edge"].sum()))
        has = p["n_counts"] >= 3
        assert np.array_equal(np.isnan(p["normals"]).any(axis=1), ~has)
        if has.any():
            worst_gap, worst_dot = min(worst_gap, p["gap"][has].min()), min(worst_dot, p["absdot"][has].min())
            assert (p["gap"][has] >= 1e-6).all() and (p["absdot"][has] > 1e-6).all(), (c.name, p["gap"][has].min(), p["absdot"][has].min())
        pairs += int((p["nn"] - 1).sum())
        assert np.isfinite(p["feat"]).all() and (p["feat"] >= 0).all()
        assert not p["feat"][~np.isfinite(p["feat_nrm"]).all(axis=1)].any()
    print("%s: %d cases, %d pairs, none near an edge; smallest gap %.3g, smallest |n . n_in| %.3g" % (family, len(fc.cases(family)), pairs, worst_gap, worst_dot))


def test_clumps_are_mutual_neighbours_at_both_radii():
    for c in fc.cases("clumps"):
        k, p = c.facts["k"], fc.restated(c)
        assert len(c.xyz) == k and (p["n_counts"] == k).all() and (p["nn"] == k).all()
        # one cell of each radius grid would do, but what the walk needs is one ROW RANGE with all k candidates: the clump is 0.05 wide
        for r in (c.r_normal, c.r_feature):
            org, cell, dim, doublings = fc.grid_of(c.xyz, r)
            assert doublings == 0 and list(dim) == [1, 1, 1]


def test_star_exact_and_coarse_counts_are_as_constructed():
    for c in fc.cases("star"):
        p = fc.restated(c)
        assert p["nn"][0] == c.facts["centre_nn"] == (27 if c.name.endswith("inner") else 1)
        assert p["n_counts"][0] == 1 and (p["n_counts"][1:27] >= 3).sum() == 20         # at 0.75 r: 12 edge points and 8 corners have a normal
    c = fc.case("exact")
    p = fc.restated(c)
    assert list(p["nn"]) == c.facts["nn"] == list(p["n_counts"]) and list(p["nn"][:3]) == [14, 1, 2]
    c = fc.case("coarse")
    p = fc.restated(c)
    assert list(p["nn"]) == c.facts["nn"] == list(p["n_counts"]) and list(p["nn"][148:]) == [1, 1]


def test_voxel_fixtures_meet_the_conditions_of_the_order_check():
    """Output k is the mean of cell k of the ascending key list; the GPU test checks the cell of every output row where the restatement's own
    rounded mean lies in its cell (a mean can round onto a face).  That must be nearly every row, or the check would be empty."""
    for family in sorted(fc.FAMILIES):
        for c in fc.cases(family):
            if not c.voxel:
                continue
            ox, on, key = fc.restated(c)["vox"]
            assert (np.diff(key) > 0).all() and len(ox) == len(key) == len(np.unique(fr.voxel_cells(c.xyz, fc.LEAF)[0]))
            own = fc.voxel_key_of(ox, c.xyz) == key
            assert own.mean() >= 0.9, (c.name, own.mean())
    a, f = fc.case("voxels-a-faces"), fc.case("voxels-f-negative")
    for c in (a, f):
        _, ijk, _, _ = fr.voxel_cells(c.xyz, fc.LEAF)
        trunc = (c.xyz * (np.float32(1.0) / np.float32(fc.LEAF))).astype(np.int64)      # truncation instead of floorf: other cells
        assert (trunc != ijk).any(), c.name
