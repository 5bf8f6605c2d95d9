"""k_fopt_gram (er_fopt.hip: the FP64 matrix-core Gram kernel of the rigid, SLAC and non-rigid normal equations), the point-state
kernels and the on-device Cholesky solve at their edges, entry by entry.

Every assembled value is compared with the np.longdouble sums of tests/fopt_sums.py (bucket arithmetic from oracle/fopt_oracle.cpp,
placement restated there; the reference is itself checked against the sequential oracle in tests/test_fopt_sums_cpu.py):

    |device - S| <= 2 n u A      n addends, A = sum of their absolute values, u = 2^-53: any summation order, the MFMA's unrounded
                                 products, the atomics of several chunks;
    n = 0  ->  exactly 0.0;      n = 1  ->  the float64 product bit for bit (the kernel's bucket arithmetic IS the oracle's).

The cases are crafted (tests/fopt_cases.py): groups of chosen sizes around the 4 rows of one MFMA and the 512 rows of a chunk, every
relation of the two lattice cells in both index orders, trilinear weights that are exactly 0 or 1, lattices of resolution 1, 2, 3 and 8,
odd list structures, the device-sorted route.  The solve is checked against its own matrix by the scaled residual.

Measured on one MI355X, worst error / bound over all cases and both routes, entries with n >= 2 (every test prints its own per case):
    rigid JJ 0.31  Jb 0.20  score 0.23     SLAC JJ 0.47  Jb 0.34  score 0.23     non-rigid 0.46
Every single-addend entry was bit-equal and every entry without an addend 0.0, on the host route and on the device-sorted one."""
import ctypes as C
import types

import numpy as np
import pytest

import fopt_cases as cases
import fopt_sums as fs
from elasticreconstruction_amd import _ffi
from elasticreconstruction_amd.fopt import FragmentOptimizer
from fopt_helpers import lattice_ctr
from oracle.pyoracle import FoptOracle

pytestmark = pytest.mark.gpu

WEIGHT = 1.7                       # the non-rigid data weight: a general number


def _both(case, posed=True):
    g, o = FragmentOptimizer(case.num, case.res, case.length), FoptOracle(case.num, case.res, case.length)
    for f, (x, n) in enumerate(case.frags):
        assert g.SetCloud(f, x, n) == -1 and o.set_cloud(f, x, n) == -1
        if posed:
            g.UpdatePose(f, case.poses[f])
            o.update_pose(f, case.poses[f])
    return g, o


def _group_table(g):
    ng = g._lib.er_fopt_group_count(g._h)
    info = np.zeros((max(ng, 1), 4), np.int32)
    _ffi.check(g._lib.er_fopt_group_info(g._h, _ffi.ptr(info)), "er_fopt_group_info")
    return info[:ng]


def _set_dev(g, pairs):
    """The lists uploaded into one device block and handed to er_fopt_set_correspondences_dev; returns the group count."""
    from elasticreconstruction_amd.icp import DeviceLists
    dl = DeviceLists([types.SimpleNamespace(n=len(p[2])) for p in pairs])
    for k, (_, _, pr) in enumerate(pairs):
        rows = np.ascontiguousarray(pr, np.int32)
        if rows.size:
            _ffi.check(g._lib.er_host_copy_h2d(C.c_void_p(dl.base + 4 * int(dl.offs[k])), _ffi.ptr(rows), rows.nbytes), "er_host_copy_h2d")
        dl.counts[k] = rows.shape[0]
    try:
        return g.SetCorrespondencesDev([(i, j) for i, j, _ in pairs], dl)
    finally:
        dl.close()


def _nonrigid_entries(num, res, diag, off, info):
    """The 24 x 24 blocks of AssembleNonrigid as (flat index, value) of the (num nper)^2 matrix: local entry c * 8 + t of a block sits at
    lattice index idx_[0] + offset of cell corner t (t = 4 dx + 2 dy + dz) + c.  Blocks of vertices that are no cell's corner stay zero."""
    n1 = res + 1
    nv, nper = n1 ** 3, 3 * n1 ** 3
    M = num * nper
    e = np.arange(24)
    t, c = e % 8, e // 8
    loc = (((t >> 2) & 1) + ((t >> 1) & 1) * n1 + (t & 1) * n1 * n1) * 3 + c
    v = np.arange(nv)
    corner = (v % n1 < res) & ((v // n1) % n1 < res) & (v // (n1 * n1) < res)
    assert diag.shape == (num, nv, 24, 24) and not diag[:, ~corner].any()
    f, cv = np.nonzero(np.broadcast_to(corner, (num, nv)))
    r = (f * nper + cv * 3)[:, None] + loc[None, :]
    keys, vals = [(r[:, :, None] * M + r[:, None, :]).reshape(-1)], [diag[f, cv].reshape(-1)]
    if len(info):
        a = (info[:, 0].astype(np.int64) * nper + info[:, 2])[:, None] + loc[None, :]
        b = (info[:, 1].astype(np.int64) * nper + info[:, 3])[:, None] + loc[None, :]
        keys.append((a[:, :, None] * M + b[:, None, :]).reshape(-1))
        vals.append(off.reshape(-1))
    return np.concatenate(keys), np.concatenate(vals)


def _assembled(g, case):
    """Everything the three assembly calls return, as {name: (flat indices, values)} of the non-zero candidates."""
    out = {}
    for mode, (JJ, Jb, s) in (("rigid", g.AssembleRigid()), ("slac", g.AssembleSLAC(case.Rt))):
        for name, arr in (("JJ", JJ), ("Jb", Jb), ("score", np.array([s]))):
            flat = arr.reshape(-1)
            k = np.flatnonzero(flat)
            out[mode, name] = (k, flat[k])
    diag, off, info = g.AssembleNonrigid(WEIGHT)
    assert np.array_equal(info, _group_table(g)) and off.shape == (len(info), 24, 24)
    out["nonrigid", "AA"] = _nonrigid_entries(case.num, case.res, diag, off, info)
    return out


def _compare(case, got, ref, route="host", patterns=True):
    worst = {}
    for (mode, name), (k, v) in got.items():
        what = "%s [%s route]: %s %s" % (case.name, route, mode, name)
        worst[mode, name] = fs.compare(ref[mode][name], k, v, what)
        if patterns:                                             # the G == 0.0 skip hides nothing: non-zero exactly where some addend is
            assert fs.zero_pattern_matches(ref[mode][name], k, v), what + ": zero pattern differs from the reference's A == 0"
    print("%-44s %-6s %5d rows  worst error / bound: %s" % (case.name, route, case.rows(), "  ".join("%s %s %.3f" % (m, n, w) for (m, n), w in worst.items())))
    return max(worst.values())


def _check(case, dev_route=False):
    """Host route (and the device-sorted one) of one case against the reference sums.  Returns (worst ratio, group table)."""
    fs.require_longdouble()
    g, o = _both(case)
    ref = fs.reference_sums(o, case.pairs, case.Rt, WEIGHT)
    ng = g.SetCorrespondences(case.pairs)
    table = _group_table(g)
    assert ng == len(table)
    worst = _compare(case, _assembled(g, case), ref)
    if dev_route:
        assert _set_dev(g, case.pairs) == ng
        assert np.array_equal(_group_table(g), table), case.name + ": the device-sorted route builds another group table"
        worst = max(worst, _compare(case, _assembled(g, case), ref, "device"))
    g.close()
    o.close()
    return worst, table


# ---- group sizes ---------------------------------------------------------------------------------------------------------------
def test_group_sizes_each_in_its_own_handle_and_all_in_one(gpu):
    """Lists of 1 .. 1025 rows that form one group each (1 - 5: partial quads of one MFMA; 63 - 65: a wave's width; 511 - 513, 1024, 1025:
    one, two and three chunks of kChunkMax = 512 rows whose atomics meet in the same entries -- in mode 2 in the same 24 x 24 block).
    Once every size alone, once all as the 13 lists of one handle, on the host route and the device-sorted one: the same group table
    (one group per list, in list order, with the cells the points were drawn in) and every entry inside the bound."""
    whole, expected = cases.group_size_case()
    worst, table = _check(whole, dev_route=True)
    assert np.array_equal(table, expected)
    alone = []
    for k, m in enumerate(cases.GROUP_SIZES):
        w, t = _check(whole.with_pairs([whole.pairs[k]], "group of %d rows" % m), dev_route=True)
        assert len(whole.pairs[k][2]) == m and t.shape == (1, 4)
        alone.append(t[0])
        worst = max(worst, w)
    assert np.array_equal(np.array(alone), table), "the groups of the single lists are not the groups of the 13 lists together"
    print("group sizes: worst error / bound %.3f" % worst)


# ---- cell relations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,relation", [(r, rel) for r in (2, 8) for rel in sorted(cases.RELATIONS) if not (r == 2 and rel == "disjoint")])
def test_cell_relations(gpu, res, relation):
    """The cells of p_i and p_j coincide (all 24 lattice indices fold: ia == ic -> 2 G on the diagonal), share a face (12), an edge (6), a
    vertex (3) or nothing, with idx_[0] of c_i below and above that of c_j (the ia < ic and ia > ic branches), as a one-row list -- every
    entry is one product or a fold of few -- and as a 37-row list (nine full quads and one lane of the tenth)."""
    folded = {"same": 24, "face": 12, "edge": 6, "vertex": 3, "disjoint": 0}[relation]
    for case in cases.relation_cases(res, relation):
        _, table = _check(case, dev_route=True)
        assert len(table) == 1
        o = FoptOracle(case.num, case.res, case.length)
        for f, (x, n) in enumerate(case.frags):
            assert o.set_cloud(f, x, n) == -1
        idx = o.slac_bucket(0, 0, 1, 0, case.Rt)[0]
        assert len(set(idx[12:36]) & set(idx[36:])) == folded and (idx[12:] >= 6 * case.num).all()
        o.close()
        assert (table[0, 2] < table[0, 3]) == ("ci<cj" in case.name) or relation == "same"


# ---- weights that are exactly 0 or 1 --------------------------------------------------------------------------------------------
def test_weights_exactly_zero_or_one(gpu):
    """Points on a cell face, edge and vertex: r = 0 exactly, so 4, 6 and 7 of the 8 trilinear weights vanish and whole rows and columns of
    the lattice part are exactly zero.  The device's non-zero set must be the reference's set of entries with a non-zero addend."""
    for case in cases.exact_weight_cases():
        g, _ = _both(case, posed=False)
        val = g.points(0)["val"]
        kind = case.name.split()[1]
        if kind in ("face", "edge", "vertex"):
            assert np.count_nonzero(val[0]) == {"face": 4, "edge": 2, "vertex": 1}[kind] and (kind != "vertex" or val[0, 0] == 1.0)
        else:
            assert sorted(np.count_nonzero(val, axis=1).tolist()) == [1] * 4 + [2] * 8 + [4] * 8 + [8] * 10
        g.close()
        _check(case, dev_route=True)


# ---- lattices, fragments and lists ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(5))
def test_lattices(gpu, k):
    """Resolution 1 (one cell: every correspondence folds all 24 indices), 2, 3, 8, and a length whose unit is no float32 number."""
    case = cases.lattice_cases()[k]
    _, table = _check(case, dev_route=True)
    assert len(table) == 3 if case.res == 1 else len(table) > 3                      # one cell: one group per list


def test_fragment_and_list_structure(gpu):
    """Two fragments; five fragments with a list given as (3, 1), the pair (0, 1) listed twice (the rigid gauge term counts lists), an empty
    list between two non-empty ones, one row five times in a list and a fragment that holds a single point."""
    two, five = cases.list_cases()
    _check(two, dev_route=True)
    assert [(i, j, len(r)) for i, j, r in five.pairs] == [(0, 1, 60), (3, 1, 60), (0, 1, 60), (1, 2, 0), (2, 3, 60), (2, 4, 25)]
    assert len(five.frags[4][0]) == 1 and (five.pairs[4][2][9:14] == five.pairs[4][2][9]).all()
    _check(five, dev_route=True)
    g, _ = _both(five)
    g.SetCorrespondences(five.pairs)
    assert g.AssembleRigid()[0][0, 0] > 6.0 and g.n_pairs == 6                   # six lists, the empty one included, on the gauge diagonal
    g.close()


def test_fragment_whose_first_point_is_out_of_bounds(gpu):
    """SetCloud returns 0 and the cloud is empty; lists that name the fragment are refused on both routes; the others assemble as ever."""
    case = cases.cube_case("first point out of bounds", 3, 3, 3.0, 80, [(0, 2)], 70, 41)
    x1 = case.frags[1][0].copy()
    x1[0, 1] = np.float32(case.length)                                              # exactly the upper bound: outside [0, length)
    g, o = FragmentOptimizer(3, 3, 3.0), FoptOracle(3, 3, 3.0)
    for f, (x, n) in enumerate(case.frags):
        assert g.SetCloud(f, x1 if f == 1 else x, n) == (0 if f == 1 else -1)
        g.UpdatePose(f, case.poses[f])
        if f != 1:
            assert o.set_cloud(f, x, n) == -1
            o.update_pose(f, case.poses[f])
    assert g.points(1)["p"].shape == (0, 3)
    bad = [(0, 1, np.array([[0, 0]], np.int32))]
    with pytest.raises(_ffi.ErError, match="out of range"):
        g.SetCorrespondences(case.pairs + bad)
    with pytest.raises(_ffi.ErError, match="without a cloud"):
        _set_dev(g, case.pairs + bad)
    ref = fs.reference_sums(o, case.pairs, case.Rt, WEIGHT)
    for route in ("host", "device"):
        ng = g.SetCorrespondences(case.pairs) if route == "host" else _set_dev(g, case.pairs)
        assert ng > 10
        _compare(case, _assembled(g, case), ref, route)
    g.close()


# ---- point state at block edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [1, 3])
def test_point_state_at_block_edges(gpu, res):
    """k_fopt_update_pose / k_fopt_update_pn run 256 threads per block: clouds of 1, 255, 256 and 257 points, the last of them just under
    the upper bound of the cube, followed by one AT the bound (out of bounds: loading stops there).  Bit-exact against the oracle after
    SetCloud, UpdatePose, UpdateAllPointPN and UpdateAllNormal."""
    length, sizes = 3.0, (1, 255, 256, 257)
    rng = np.random.default_rng(60 + res)
    g, o = FragmentOptimizer(len(sizes), res, length), FoptOracle(len(sizes), res, length)
    poses = [cases.small_pose(70 + f) for f in range(len(sizes))]

    def same():
        for f, m in enumerate(sizes):
            a, b = g.points(f), o.points(f)
            assert a["p"].shape == (m, 3) and b["p"].shape[0] == m + 1            # (the oracle keeps the rejected point's slot)
            for key in ("idx0", "val", "nval", "p", "n"):
                assert np.array_equal(a[key].view(np.uint32), b[key][:m].view(np.uint32)), (res, m, key)

    for f, m in enumerate(sizes):
        x, n = cases.cube_points(rng, length, m + 1), cases.unit_normals(rng, m + 1)
        x[m - 1, f % 3] = np.nextafter(np.float32(length), np.float32(0))          # the last point that is inside
        x[m, (f + 1) % 3] = np.float32(length)                                     # the first one that is not
        assert g.SetCloud(f, x, n) == m and o.set_cloud(f, x, n) == m
        assert g.points(f)["idx0"][m - 1] // 3 // (res + 1) ** (f % 3) % (res + 1) == res - 1
    same()
    for f in range(len(sizes)):
        g.UpdatePose(f, poses[f])
        o.update_pose(f, poses[f])
    same()
    ctr = lattice_ctr(len(sizes), res, length, [P.astype(np.float64) for P in poses], 0.003, rng)
    g.UpdateAllPointPN(ctr)
    for f in range(len(sizes)):
        o.update_point_pn(f, ctr[f * o.nper:(f + 1) * o.nper])
    same()
    ctr = lattice_ctr(len(sizes), res, length, [np.eye(4)] * len(sizes), 0.004, rng)
    g.UpdateAllNormal(ctr)
    for f in range(len(sizes)):
        o.update_normals(f, ctr[f * o.nper:(f + 1) * o.nper])
    same()
    g.close()
    o.close()


# ---- the solve against its own matrix -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,num,res,unknowns", cases.SOLVE_SIZES)
def test_solve_residual_against_numpy(gpu, monkeypatch, mode, num, res, unknowns):
    """A x = b is asserted: the regularised system is built on the host from the REFERENCE sums (fopt_sums.slac_system / nonrigid_system),
    factored on the device by FactorSLAC(Rt, 1000) / FactorNonrigid(1) -- dense, and block-sparse with ER_FOPT_DENSE_MAX=0 -- and three
    random right-hand sides (SLAC: a fourth with add_data_jb) are solved.  The sizes are those at which potrf_rec's split
    n1 = ceil(n / 2 / 64) * 64 meets its edges (fopt_cases.SOLVE_SIZES: n = 36 is one block with jb < 64, 93 = 64 + 29,
    129 = 64 + (64 + 1), 204 = 128 + 76, 72 = 64 + 8, 243 = 128 + 115; block-sparse 3 x 24 and 3 x 81 = 3 x (64 + 17)).
    eta(x) = |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf) in longdouble must not exceed 8 x the eta of numpy's float64 Cholesky solve of the
    same matrix (blocked against unblocked elimination order), with a floor of n 2^-53 for a numpy that happens to be exact."""
    fs.require_longdouble()
    case = cases.solve_case(mode, num, res)
    g, o = _both(case)
    ref = fs.reference_sums(o, case.pairs, case.Rt, 1.0)
    A = fs.slac_system(ref["slac"]["JJ"], num, res, 1000.0) if mode == "slac" else fs.nonrigid_system(ref["nonrigid"]["AA"], num, res)
    assert A.shape == (unknowns, unknowns)
    cond = np.linalg.cond(A)
    assert cond < 1e10, "cond_2 = %.3g: the residual would say nothing" % cond
    Lc = np.linalg.cholesky(A)
    rng = np.random.default_rng(unknowns)
    g.SetCorrespondences(case.pairs)
    for layout in (("dense",) if mode == "slac" else ("dense", "blocked")):
        monkeypatch.setenv("ER_FOPT_DENSE_MAX", "0" if layout == "blocked" else "1000000")
        if mode == "slac":
            dataJb, _ = g.FactorSLAC(case.Rt, 1000.0)
            fs.compare_dense(ref["slac"]["Jb"], dataJb, case.name + ": dataJb of FactorSLAC")
        else:
            g.FactorNonrigid(1.0)
        for k in range(4 if mode == "slac" else 3):
            b = rng.normal(size=unknowns)
            x = g.Solve(b, add_data_jb=(k == 3))
            if k == 3:
                b = b + dataJb                                                     # what k_fopt_axpy forms: one float64 addition per entry
            xn = np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
            eta, eta_np = fs.scaled_residual(A, x, b), fs.scaled_residual(A, xn, b)
            print("%-26s %-8s n = %3d cond_2 = %.2g rhs %d: eta device %.3g  numpy %.3g  (n u = %.3g)" % (
                case.name, layout, unknowns, cond, k, eta, eta_np, unknowns * fs.U))
            # measured on one MI355X: SLAC eta <= 5.2e-18 (numpy 5.8e-18), non-rigid <= 3.2e-16 (numpy 2.7e-16), dense and blocked alike;
            # the largest ratio device / numpy over the 28 solves was 3.2
            assert np.isfinite(x).all() and eta <= max(8.0 * eta_np, unknowns * fs.U), (case.name, layout, k, eta, eta_np)
    g.close()
    o.close()
