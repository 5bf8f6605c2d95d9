"""The longdouble reference of tests/fopt_sums.py is not its own judge: its sums must agree, entry by entry, with the sequential
float64 sums of oracle/fopt_oracle.cpp (pinned to the reference program by tests/test_fopt_oracle.py) within 2 n u A -- n additions
and n rounded products of relative error u = 2^-53 each -- and exactly where there is nothing to round (n = 0: both 0.0; n = 1: the
product itself).  The regularised systems the solve tests are built on are checked by their properties: the host-side assembly of
FragmentOptimizer.OptimizeSLAC / OptimizeNonrigid cannot be reached without a device (the data term comes from the GPU)."""
import numpy as np
import pytest

import fopt_cases as cases
import fopt_sums as fs
from fopt_helpers import make_scene
from oracle.pyoracle import FoptOracle

WEIGHT = 1.7


def posed_oracle(case):
    o = FoptOracle(case.num, case.res, case.length)
    for f, (x, n) in enumerate(case.frags):
        assert o.set_cloud(f, x, n) == -1
        o.update_pose(f, case.poses[f])
    o.set_pairs(case.pairs)
    return o


def _scene_case():
    sc = make_scene(num=3, n=6000)
    c = cases.Case("room scene", sc["num"], sc["res"], sc["length"], sc["frags"], sc["pairs"], 1)
    c.poses = [P.astype(np.float32) for P in sc["init"]]
    c.Rt = np.stack([P[:3, :3].T.reshape(9) for P in sc["init"]])
    return c


CASES = {
    "scene": _scene_case,
    "group_sizes": lambda: cases.group_size_case()[0],
    "five_fragments": lambda: cases.list_cases()[1],
}


@pytest.mark.parametrize("which", sorted(CASES))
def test_reference_sums_agree_with_the_sequential_oracle(which):
    fs.require_longdouble()
    case = CASES[which]()
    assert case.rows() > 200
    o = posed_oracle(case)
    ref = fs.reference_sums(o, case.pairs, case.Rt, WEIGHT)
    worst = {}
    JJ, Jb, s = o.assemble_rigid()
    worst["rigid JJ"] = fs.compare_dense(ref["rigid"]["JJ"], JJ, "rigid JJ")
    worst["rigid Jb"] = fs.compare_dense(ref["rigid"]["Jb"], Jb, "rigid Jb")
    worst["rigid score"] = fs.compare_dense(ref["rigid"]["score"], [s], "rigid score")
    JJ, Jb, s = o.assemble_slac(case.Rt)
    worst["SLAC JJ"] = fs.compare_dense(ref["slac"]["JJ"], JJ, "SLAC JJ")
    worst["SLAC Jb"] = fs.compare_dense(ref["slac"]["Jb"], Jb, "SLAC Jb")
    worst["SLAC score"] = fs.compare_dense(ref["slac"]["score"], [s], "SLAC score")
    r, c, v = o.assemble_nonrigid(WEIGHT)
    AA = ref["nonrigid"]["AA"]
    assert np.array_equal(r * AA.shape[1] + c, AA.keys)                       # the oracle holds exactly the touched entries
    worst["non-rigid AA"] = fs.compare(AA, r * AA.shape[1] + c, v, "non-rigid AA")
    print("%s: %d rows, worst error / bound %s" % (case.name, case.rows(), ", ".join("%s %.3f" % kv for kv in worst.items())))
    # the counts are what the placement rule says they are
    T = case.rows()
    assert ref["rigid"]["score"].n.tolist() == [T] and ref["slac"]["score"].n.tolist() == [T]
    assert ref["rigid"]["JJ"].n.sum() == 144 * T + 6 * len(case.pairs) and ref["slac"]["JJ"].n.sum() == 1830 * T
    assert ref["rigid"]["Jb"].n.sum() == 12 * T and ref["slac"]["Jb"].n.sum() == 60 * T and AA.n.sum() == 3 * 576 * T
    o.close()


def test_compare_rejects_what_it_should():
    """The comparison itself: a single-addend entry off by one ulp, an entry off by one part in 10^9, a value where there is no addend."""
    fs.require_longdouble()
    case = cases.relation_cases(2, "face")[0]                       # one row: single-addend entries, and folded ones on the shared face
    o = posed_oracle(case)
    ref = fs.reference_sums(o, case.pairs, case.Rt, WEIGHT)["slac"]["JJ"]
    JJ = o.assemble_slac(case.Rt)[0]
    fs.compare_dense(ref, JJ, "as computed")
    S, A, n = ref.dense()
    one, many, none = np.argwhere(n == 1)[0], np.argwhere(n > 1)[0], np.argwhere(n == 0)[-1]
    for at, value in ((one, np.nextafter(JJ[tuple(one)], np.inf)), (many, JJ[tuple(many)] * (1 + 1e-9)), (none, 1e-300)):
        B = JJ.copy()
        B[tuple(at)] = value
        with pytest.raises(AssertionError):
            fs.compare_dense(ref, B, "perturbed")
    o.close()


@pytest.mark.parametrize("res", [1, 2, 3])
def test_lattice_laplacian_properties(res):
    L = fs.lattice_laplacian(res)
    assert np.array_equal(L, L.T) and not L.sum(1).any()                      # symmetric, zero row sums: constants are its null space
    n1 = res + 1
    deg = np.array([sum((x > 0) + (x < res) for x in (i, j, k)) for k in range(n1) for j in range(n1) for i in range(n1)])
    assert np.array_equal(np.diag(L)[::3], 2.0 * deg)                         # every edge is visited from both ends
    assert np.linalg.eigvalsh(L).min() > -1e-12 and np.linalg.matrix_rank(L) == L.shape[0] - 3
    from elasticreconstruction_amd.fopt import Lattice
    assert np.array_equal(L, Lattice(res, 3.0).laplacian())                   # the product's host-side regulariser says the same


@pytest.mark.parametrize("mode,num,res,unknowns", cases.SOLVE_SIZES)
def test_regularised_systems_are_well_posed(mode, num, res, unknowns):
    """The systems the device solve is checked on: symmetric, positive definite, cond_2 < 1e10 (so that a scaled residual near the unit
    roundoff means a solution with digits left), and of the size whose potrf_rec split the GPU test states."""
    fs.require_longdouble()
    case = cases.solve_case(mode, num, res)
    o = posed_oracle(case)
    ref = fs.reference_sums(o, case.pairs, case.Rt, 1.0)
    A = fs.slac_system(ref["slac"]["JJ"], num, res, 1000.0) if mode == "slac" else fs.nonrigid_system(ref["nonrigid"]["AA"], num, res)
    assert A.shape == (unknowns, unknowns) and np.array_equal(A, A.T)
    w = np.linalg.eigvalsh(A)
    print("%s: n = %d, eigenvalues %.3g .. %.3g, cond_2 = %.3g" % (case.name, unknowns, w[0], w[-1], w[-1] / w[0]))
    assert w[0] > 0 and w[-1] / w[0] < 1e10
    # the pose block carries the data term and the gauge's 1 on the first six diagonal entries, nothing of the regulariser
    if mode == "slac":
        B = fs.slac_system(ref["slac"]["JJ"], num, res, 1000.0)
        oracle_JJ = o.assemble_slac(case.Rt)[0]
        D = oracle_JJ + np.triu(oracle_JJ, 1).T
        assert np.abs((B - D)[:6 * num, :6 * num] - np.diag(np.r_[np.ones(6), np.zeros(6 * num - 6)])).max() <= 1e-12 * np.abs(D).max()
    o.close()
