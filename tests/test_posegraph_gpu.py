"""The pose graph optimiser on the GPU (er_pgo_*, csrc/er_pgo.hip) against the numpy restatement (tests/posegraph_restatement.py) on
the fixtures of tests/posegraph_cases.py: N = 2 without a loop, N = 3 with one, N = 6 and 10, N = 12 (dimension 66: one 64-wide block and two
more rows), N = 33 (192), N = 65 with 316 loops (384: several panels, a trailing update of more than one workgroup), a vertex on no loop, two
loops on one pair, loops with id1 > id2, identity information.  The pin is the restatement, not g2o.

Linearisation: every entry of H, b and chi2 within C_LIN 2^-53 sum|terms|.  The terms are taken down to the inputs (tests/posegraph_bounds.py,
input_terms), not at the level of a block's contributions: a contribution is itself a sum that cancels -- exactly, where
dt/dq_j = 0 makes an entry a structural zero, and almost, in the residual, which is what is left (1e-3, or 1e-17 on an odometry edge at the
initial state) of isometry entries of size 1 -- so only the absolute values of what is added bound how two correct evaluations can differ.
The two sides add a block's contributions in the same order but form each one in another order (numpy's products against the kernel's
unrolled sums).  At the perturbed state, where no residual is pure rounding, the contribution-level bound (posegraph_bounds.contribution_terms)
is asserted as well for b and chi2, with its own measured constant C_CONTRIB.  MEASURED on one MI355X: see the constants below.
"""
import numpy as np
import pytest

import fopt_sums as fs
import posegraph_bounds as pb
import posegraph_cases as pc
import posegraph_restatement as pr
from elasticreconstruction_amd import _ffi
from elasticreconstruction_amd.posegraph import PoseGraph

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
# Worst ratio |device - restatement| / (2^-53 sum|terms|) over H, b and chi2 of all fixtures, at both states and both lambdas, measured on one
# MI355X: 0.8 (an entry of H of the N = 2 graph at its initial state; b and chi2 stay below 0.1, the first-order bound is loose for them).
# C_LIN is four times that: the per-edge products are associated differently as well.
MEASURED_RATIO = 0.85
C_LIN = 4.0 * MEASURED_RATIO
# The same ratio against the contribution-level terms for b and chi2, at the perturbed state only (both lambdas), measured on one MI355X: 269.1
# for b (N = 33), 64.7 for chi2 (N = 65) -- the conditioning of the residual (1e-2 left of entries of size 1), not a summation order; C_CONTRIB is
# four times it.  For H the contribution level says nothing even there (measured 5e2 .. 6e5, and 1e15 .. 4e16 on n2, n3 and lonely): an entry of a
# contribution J^T Om J is itself a sum of products that cancel, so H is printed against it and asserted against the input-level terms only.
MEASURED_CONTRIB = 270.0
C_CONTRIB = 4.0 * MEASURED_CONTRIB
ALL = list(pc.CASES)
EM_CASES = [n for n in ALL if n != "n2"]                     # every fixture with a loop


def handle(name):
    c = pc.case(name)
    return PoseGraph(c["odo_T"], (c["loop_ids"], c["loop_T"]), c["odo_info"], c["loop_info"])


def perturb(g, seed=3):
    """the restatement graph g moved off its initial state: poses by about 0.01, switches into (0.1, 1)"""
    rng = np.random.RandomState(seed)
    g.sw = rng.uniform(0.1, 1.0, g.K)
    for v in range(1, g.N):
        g.poses[v] = pr.product(g.poses[v], pr.from_mqt(rng.normal(size=6) * 0.01))


_ratios, _contrib = {}, {}


def _ratio(got, want, terms):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(terms > 0, np.abs(got - want) / (U * terms), np.where(got == want, 0.0, np.inf)).max())


@pytest.mark.parametrize("name", ALL)
def test_linearisation(gpu, name):
    g, h = pc.graph(name), handle(name)
    worst, worst_c = 0.0, 0.0
    for state in ("initial", "perturbed"):
        if state == "perturbed":
            perturb(g)
            h.state(g.poses, g.sw)
        for lam in (0.0, 0.37):
            Hr, br, chi2r, recs = g.linearize(1.0, lam)
            H, b, chi2 = h.linearize(1.0, lam)
            ratios = [_ratio(x, y, t) for x, y, t in zip((H, b, chi2), (Hr, br, chi2r), pb.input_terms(g, 1.0, lam))]
            print("%-9s %-9s lambda %.2f: worst ratio to the input-level terms H %.2f  b %.2f  chi2 %.2f" % ((name, state, lam) + tuple(ratios)))
            worst = max([worst] + ratios)
            if state == "perturbed":
                ratios = [_ratio(x, y, t) for x, y, t in zip((H, b, chi2), (Hr, br, chi2r), pb.contribution_terms(g, recs))]
                print("%-9s %-9s lambda %.2f: worst ratio to the contribution-level terms H %.1f  b %.1f  chi2 %.1f" % ((name, state, lam) + tuple(ratios)))
                worst_c = max([worst_c] + ratios[1:])                                # b and chi2 (H: see C_CONTRIB)
    _ratios[name], _contrib[name] = round(worst, 2), round(worst_c, 1)
    print("worst ratios so far: input level", _ratios, "contribution level", _contrib)
    h.close()
    assert worst <= C_LIN, (name, worst)
    assert worst_c <= C_CONTRIB, (name, worst_c)


@pytest.mark.parametrize("name", ALL)
def test_one_trial(gpu, name):
    """er_pgo_trial from the restatement's perturbed state: dx solves the device's own (H + lambda I) dx = -b by the scaled residual (the bar of
    tests/test_fopt_shapes_gpu.py: eta <= max(8 eta of numpy's Cholesky solve, n 2^-53)); dx, ds and F_new against the restatement at 1e-9.
    Observed on one MI355X: eta 1.2e-17 .. 6.5e-17 (numpy 2.4e-17 .. 1.5e-16); dx within 1.7e-13, ds 4.5e-15, F_new 2.8e-12."""
    g, h = pc.graph(name), handle(name)
    perturb(g)
    h.state(g.poses, g.sw)
    lam = g.lambda0(1.0, True) * 3.0
    H, b, _ = h.linearize(1.0, lam)
    dx, ds, F_new, status = h.trial(1.0, lam)
    P, S = h.state()
    assert np.array_equal(P, g.poses) and np.array_equal(S, g.sw), "a trial must leave the current state alone"
    assert status == 0
    A = H + lam * np.eye(len(b))
    Lc = np.linalg.cholesky(A)
    xn = np.linalg.solve(Lc.T, np.linalg.solve(Lc, -b))
    eta, eta_np = fs.scaled_residual(A, dx, -b), fs.scaled_residual(A, xn, -b)
    t = g.trial(1.0, lam)
    rel = lambda a, b_: float(np.abs(a - b_).max() / max(np.abs(b_).max(), 1e-300)) if np.size(b_) else 0.0
    print("%-9s n = %3d: eta device %.3g numpy %.3g (n u %.3g); dx %.3g  ds %.3g  F_new %.3g relative to the restatement" % (
        name, len(b), eta, eta_np, len(b) * U, rel(dx, t[0]), rel(ds, t[1]), abs(F_new - t[4]) / t[4]))
    h.close()
    assert eta <= max(8.0 * eta_np, len(b) * U)
    assert rel(dx, t[0]) <= 1e-9 and rel(ds, t[1]) <= 1e-9 and abs(F_new - t[4]) <= 1e-9 * t[4]


def compare_runs(name, method, o, ref):
    """trace while the restatement still moves, then the end state"""
    c = pc.case(name)
    g = pc.graph(name)
    floor = 1e-24 * sum(np.trace(Om) for Om in g.Om)           # an F below the rounding of its own residuals (2^-53 of entries of size 1, squared) says nothing
    compared = 0
    for k, (lam, F, F_new, ok) in enumerate(ref["trace"]):
        if not (np.isfinite(F_new) and F > floor and abs(F - F_new) > 1e-9 * F):
            break
        assert k < len(o["trace"])
        row = o["trace"][k]
        assert bool(row[3]) == ok, (name, method, k)
        assert abs(row[0] - lam) <= 1e-9 * lam and abs(row[1] - F) <= 1e-9 * F and abs(row[2] - F_new) <= 1e-9 * abs(F_new), (name, method, k, row, (lam, F, F_new))
        compared += 1
    dp, dv = np.abs(o["poses"] - ref["poses"]).max(), (np.abs(o["values"] - ref["values"]).max() if len(ref["values"]) else 0.0)
    print("%-9s %-10s %d of %d trials compared (device made %d); end state: poses %.3g, %s %.3g off the restatement's" % (
        name, method, compared, len(ref["trace"]), o["trials"], dp, "switches" if method == "switchable" else "weights", dv))
    assert np.array_equal(o["kept"], ref["kept"])
    assert dp <= 1e-6 and dv <= 1e-6
    return c


@pytest.mark.parametrize("name", ALL)
def test_switchable_trace_and_end_state(gpu, name):
    """Accept / reject, lambda and F equal the restatement's to 1e-9 while its own relative decrease exceeds 1e-9; then kept set equal and poses and
    switches within 1e-6 per entry (DESIGN.md 2's bar for iterated solves).  Observed on one MI355X: 4 .. 6 trials compared per graph; poses within
    2.8e-10 and switches within 7.2e-9 of the restatement's (the worst: identity information and N = 33)."""
    h = handle(name)
    o = h.optimize("switchable", 1.0, 100)
    h.close()
    c = compare_runs(name, "switchable", o, pc.solved(name, "switchable"))
    # Without .info files (the identity fixture) the pruning cannot tell these false loops from the true ones: a loop 0.5 m off costs 0.25 against
    # the prior's w = 1, so its switch stays at 0.80 .. 0.95 and it is kept (tests/test_posegraph_cpu.py asserts exactly that outcome on the
    # restatement).  There the device is held to the restatement's kept set (compare_runs), everywhere else also to the true set.
    assert np.array_equal(o["kept"], c["is_true"]) or name == "identity"


@pytest.mark.parametrize("name", EM_CASES)
def test_em_trace_and_end_state(gpu, name):
    """The same for the EM mode (40 rounds) on every fixture with a loop: k_pgo_estep, the sqrt(l) Omega scaling and a fresh lambda_0 per round on
    systems of one block (n3 .. n10) up to six (n65).  (The identity fixture: see test_switchable_trace_and_end_state.)"""
    h = handle(name)
    o = h.optimize("em", 1.0, pc.EM_ROUNDS)
    h.close()
    c = compare_runs(name, "em", o, pc.solved(name, "em"))
    assert o["iterations"] == pc.EM_ROUNDS
    assert np.array_equal(o["kept"], c["is_true"]) or name == "identity"


def test_reproducible(gpu):
    """Two runs on one handle and a run on a second handle of the same graph: the same bits in poses, switches, trace and H."""
    a, b = handle("n33"), handle("n33")
    o1, o2, o3 = a.optimize(), a.optimize(), b.optimize()
    Ha, Hb = a.linearize(1.0, 0.1)[0], b.linearize(1.0, 0.1)[0]
    a.close()
    b.close()
    for o in (o2, o3):
        assert np.array_equal(o1["poses"], o["poses"]) and np.array_equal(o1["values"], o["values"]) and np.array_equal(o1["trace"], o["trace"])
    assert np.array_equal(Ha, Hb)


def test_a_failed_factorisation_inside_optimize_is_a_rejected_trial(gpu):
    """The reject path of k_pgo_decide with a bad pivot, inside er_pgo_optimize: with every information matrix negated H is negative definite, so
    lambda_0 = 1e-5 max(0, max diag H) = 0 and no pivot of any trial is positive.  All 10 trials of the first iteration are rejected, the run
    ends there, and the state is the initial one bit for bit -- in the restatement (numpy's LinAlgError) and on the device (the status word)."""
    c = pc.case("n6")
    h = PoseGraph(c["odo_T"], (c["loop_ids"], c["loop_T"]), -c["odo_info"], -c["loop_info"])
    start = h.optimize("switchable", 1.0, 0)
    o = h.optimize("switchable", 1.0, 100)
    h.close()
    ref = pr.Graph(c["odo_T"], c["loop_ids"], c["loop_T"], -c["odo_info"], -c["loop_info"]).optimize("switchable", 1.0, 100)
    assert ref["iterations"] == 1 and ref["trials"] == 10 and not any(t[3] for t in ref["trace"])
    assert o["iterations"] == 1 and o["trials"] == 10 and not o["trace"][:, 3].any() and not o["trace"][:, 0].any()
    assert start["trials"] == 0 and np.array_equal(o["poses"], start["poses"]) and np.array_equal(o["values"], np.ones(len(c["is_true"])))
    assert np.abs(o["poses"] - ref["poses"]).max() <= 1e-12


def test_refusals(gpu):
    c = pc.case("n6")
    ids, T, info = c["loop_ids"].copy(), c["loop_T"].copy(), c["loop_info"].copy()

    def refused(match, odo=c["odo_T"], ids=ids, T=T, oi=c["odo_info"], li=info):
        with pytest.raises(_ffi.ErError, match=match):
            PoseGraph(odo, (ids, T), oi, li)

    bad = ids.copy()
    bad[3] = (2, 2)
    refused("loop entry 3: id1 == id2 == 2", ids=bad)
    bad = ids.copy()
    bad[4] = (1, 6)
    refused(r"loop entry 4: ids \(1, 6\) are out of range for 6 poses", ids=bad)
    bad[4] = (-1, 3)
    refused(r"loop entry 4: ids \(-1, 3\)", ids=bad)
    bad = T.copy()
    bad[5, 1, 3] = np.nan
    refused("loop entry 5: the transform is not finite", T=bad)
    bad = info.copy()
    bad[6, 2, 2] = np.inf
    refused("loop entry 6: the information matrix is not finite", li=bad)
    bad = c["odo_T"].copy()
    bad[2, 0, 0] = np.inf
    refused("odometry entry 2: the transform is not finite", odo=bad)
    bad = c["odo_info"].copy()
    bad[1, 5, 0] = np.nan
    refused("odometry entry 1: the information matrix is not finite", oi=bad)
    refused("loop information has 9 entries, the loops 10", li=info[:9])
    refused("odometry information has 4 entries, the odometry 5", oi=c["odo_info"][:4])
    with pytest.raises(_ffi.ErError, match=r"1 poses \(2 \.\. 1024"):
        PoseGraph(np.zeros((0, 4, 4)), None)
    h = handle("n6")
    with pytest.raises(_ffi.ErError, match="weight"):
        h.optimize("switchable", 0.0, 5)
    # a pose that is not finite: no pivot is positive and finite, the trial reports it and nothing worse happens
    P, S = h.state()
    P[3, 0, 3] = np.nan
    h.state(P, S)
    dx, ds, F_new, status = h.trial(1.0, 1e-3)
    assert status == 1 and not np.isfinite(F_new)
    o = h.optimize("switchable", 1.0, 100)                    # optimize starts from the odometry chain again, whatever the state was
    h.close()
    assert np.abs(o["poses"] - pc.solved("n6", "switchable")["poses"]).max() <= 1e-6
