"""The pose graph optimiser without a GPU: the numpy restatement (tests/posegraph_restatement.py) against its own central
differences and against the full system with explicit switch variables, csrc/er_pgo_math.h compiled for the host against the restatement,
the fixtures (tests/posegraph_cases.py) and what both modes make of them, the output files, and the refusals.  Nothing here is checked against
g2o: the reference tree cannot build it.

The restatement on the fixtures (seed 1, weight 1; switchable 100 iterations, EM 40 rounds), measured on the CPU:
    n6   10 loops, 2 false: true switches >= 0.9904, false <= 0.00033, poses within 1.2e-3 of the truth, 8 iterations;  EM weights >= 0.444 / <= 0.0004
    n10  25 loops, 5 false: true switches >= 0.9917, false <= 0.0024,  poses within 1.5e-3, 11 iterations;               EM weights >= 0.635 / <= 0.0026
    n33  221 loops, 44 false: >= 0.983 / <= 0.0124, 1.8e-3, 15 iterations;   n65  316 loops, 63 false: >= 0.982 / <= 0.0068, 3.0e-3, 11 iterations
The EM mode's fixed point is a robust estimate, not an outlier-free one (sqrt(l) Omega makes a far-off edge's cost grow like |r|, so it keeps
pulling): its poses are 0.016 .. 0.12 off the truth on these graphs (true weights >= 0.444, the lowest at n6; false <= 0.012).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import posegraph_cases as pc
import posegraph_restatement as pr
from elasticreconstruction_amd import _ffi, formats, posegraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}
WITH_INFO = [n for n in pc.CASES if n != "identity"]
EM_CASES = [n for n in pc.CASES if n != "n2"]              # every fixture with a loop


def hostlib():
    if "lib" not in _cache:
        src = os.path.join(ROOT, "tests", "hostcheck", "pgo_math_check.cpp")
        inc = os.path.join(ROOT, "elasticreconstruction_amd", "csrc")
        out = os.path.join(ROOT, "tests", "hostcheck", "_build", "libpgo_math_check.so")
        deps = [src, os.path.join(inc, "er_pgo_math.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I" + inc, src, "-o", out], check=True)
        L = C.CDLL(out)
        L.pgo_edge_cost.restype = C.c_double
        L.pgo_edge_cost.argtypes = [C.c_double, C.c_int, C.c_double, C.c_double]
        _cache["lib"] = L
    return _cache["lib"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def random_edges(n, seed):
    """Z, Xi, Xj [n, 4, 4] with rotations up to pi (the product q_A q_B has a negative w for about half of them), Om [n, 6, 6]"""
    rng = np.random.RandomState(seed)
    Z, Xi, Xj = (np.stack([pc.rigid(rng, np.pi, 2.0) for _ in range(n)]) for _ in range(3))
    Om = np.stack([pc.information(rng) for _ in range(8)])[rng.randint(0, 8, n)]
    return rng, Z, Xi, Xj, Om


def test_analytic_jacobians_equal_central_differences():
    """h = 1e-7: the truncation error is about h^2 |r'''| / 6 ~ 1e-14, the rounding error about 2^-53 |r| / h ~ 1e-9 for |t| of a few metres."""
    rng, Z, Xi, Xj, _ = random_edges(300, 11)
    worst, negative = 0.0, 0
    for e in range(300):
        r, Ji, Jj = pr.jacobians(Z[e], Xi[e], Xj[e])
        Ni, Nj = pr.numeric_jacobians(Z[e], Xi[e], Xj[e])
        worst = max(worst, np.abs(Ji - Ni).max(), np.abs(Jj - Nj).max())
        qa, qb = pr.quaternion(pr.inverse(Z[e])), pr.quaternion(pr.product(pr.inverse(Xi[e]), Xj[e]))
        negative += qa[3] * qb[3] - qa[:3] @ qb[:3] < 0
    print("worst |analytic - central difference| = %.3g; q_A q_B has w < 0 in %d of 300" % (worst, negative))
    assert negative > 50, "the sign of the quaternion product is not exercised"
    assert worst < 5e-8


def test_host_math_equals_the_restatement():
    """er_pgo_math.h on the host: residual, Jacobians, the reduced contribution and delta_s on 3000 random edges, s = 0 and s = 1 included.
    Both sides are float64 sums of at most 6 x 6 x 2 products in different orders: entries agree to a few 2^-53 of the largest term,
    asserted at 1e-12 of the largest entry of the quantity (the Schur term cancels at most one digit here)."""
    n = 3000
    rng, Z, Xi, Xj, Om = random_edges(n, 5)
    scale = np.where(rng.uniform(size=n) < 0.5, 1.0, rng.uniform(0.01, 1.0, n))
    switchable = (rng.uniform(size=n) < 0.7).astype(np.int32)
    s = rng.uniform(0, 1, n)
    s[:200] = 0.0
    s[200:400] = 1.0
    switchable[:400] = 1
    w, lam = 1.7, 0.3
    L = hostlib()
    assert L.pgo_record_size() == 176
    r, Ji, Jj, rec = np.zeros((n, 6)), np.zeros((n, 36)), np.zeros((n, 36)), np.zeros((n, 176))
    L.pgo_edges(n, _p(Z), _p(Xi), _p(Xj), _p(Om), _p(scale), _p(switchable), _p(s), C.c_double(w), C.c_double(lam), _p(r), _p(Ji), _p(Jj), _p(rec))
    r2 = np.zeros((n, 6))
    L.pgo_residuals(n, _p(Z), _p(Xi), _p(Xj), _p(r2))
    assert np.array_equal(r, r2)
    dx = rng.normal(size=(n, 12)) * 0.01
    ds, hd = np.zeros(n), np.zeros(n)
    L.pgo_delta_s(n, _p(rec), _p(dx), _p(ds), _p(hd))
    worst = dict(r=0.0, J=0.0, H=0.0, g=0.0, hps=0.0, scalars=0.0, ds=0.0)
    rel = lambda a, b, scale_of: np.abs(a - b).max() / max(np.abs(scale_of).max(), 1e-300)
    for e in range(n):
        re, Jie, Jje = pr.jacobians(Z[e], Xi[e], Xj[e])
        R = pr.edge_record(scale[e] * Om[e], re, Jie, Jje, bool(switchable[e]), s[e], w, lam)
        worst["r"] = max(worst["r"], rel(r[e], re, re))
        worst["J"] = max(worst["J"], rel(Ji[e].reshape(6, 6), Jie, Jie), rel(Jj[e].reshape(6, 6), Jje, Jje))
        worst["H"] = max(worst["H"], rel(rec[e, :144].reshape(12, 12), R["H"], R["Hfull"]))
        worst["g"] = max(worst["g"], rel(rec[e, 144:156], R["g"], R["gfull"]))
        worst["hps"] = max(worst["hps"], rel(rec[e, 156:168], R["hps"], R["hps"]))
        worst["scalars"] = max(worst["scalars"], rel(rec[e, 168:171], np.array([R["hss"], R["bs"], R["chi2"]]), np.array([R["hss"], R["chi2"]])))
        want = (-R["bs"] - R["hps"] @ dx[e]) / R["hss"]
        worst["ds"] = max(worst["ds"], abs(ds[e] - want) / max(abs(R["bs"]) + np.abs(R["hps"] * dx[e]).sum(), 1e-300) * R["hss"])
        c = L.pgo_edge_cost(R["chi2"], int(switchable[e]), s[e], w)
        want_c = s[e] ** 2 * R["chi2"] + w * (1 - s[e]) ** 2 if switchable[e] else R["chi2"]
        assert abs(c - want_c) <= 1e-14 * max(abs(want_c), 1.0)
    print("worst relative differences:", worst)
    assert all(v < 1e-12 for v in worst.values()), worst
    # fromMQT: the unit-sphere rule included
    d = rng.normal(size=(50, 6))
    d[:25, 3:] *= 0.3
    D = np.zeros((50, 16))
    L.pgo_from_mqt(50, _p(d), _p(D))
    assert max(np.abs(D[k].reshape(4, 4) - pr.from_mqt(d[k])).max() for k in range(50)) < 1e-14
    assert (np.linalg.norm(d[25:, 3:], axis=1) > 1).any()


@pytest.mark.parametrize("name", ["n3", "n6", "duplicate", "reverse"])
def test_the_reduced_system_solves_the_full_one(name):
    """The 1 x 1 Schur complements are exact: (dx, ds) of a trial equal the solution of the damped (6 (N - 1) + K) system with explicit switches."""
    g = pc.graph(name)
    rng = np.random.RandomState(3)
    g.sw = rng.uniform(0.1, 1.0, g.K)
    for v in range(1, g.N):
        g.poses[v] = pr.product(g.poses[v], pr.from_mqt(rng.normal(size=6) * 0.01))
    w, lam = 1.0, 0.37
    H, b = g.full_system(w)
    full = np.linalg.solve(H + lam * np.eye(len(b)), -b)
    dx, ds, _, _, _, denom = g.trial(w, lam)
    err = max(np.abs(dx - full[:g.n]).max(), np.abs(ds - full[g.n:]).max()) / np.abs(full).max()
    print("relative difference %.3g; condition number %.3g" % (err, np.linalg.cond(H + lam * np.eye(len(b)))))
    assert err < 1e-9
    assert abs(denom - full @ (lam * full - b)) <= 1e-9 * abs(denom)           # the predicted decrease, over poses and switches


@pytest.mark.parametrize("name", list(pc.CASES))
def test_fixture_margins_and_switchable_result(name):
    """No final switch in (0.25, 0.75): a threshold test must not rest on a coin flip.  With information matrices the kept set is the true set and
    every pose entry is within one measurement's noise of the truth: 0.002 rad at the graph's extent plus 0.002 m."""
    c, o = pc.case(name), pc.solved(name, "switchable")
    v = o["values"]
    assert not ((v > 0.25) & (v < 0.75)).any(), v
    if name == "identity":
        # Without information matrices the pruning does not separate these false loops: 0.5 m off costs 0.25 against the prior's w = 1, so the
        # switch settles near 1 / (1 + 0.25) and the edge is kept.  That is the model's answer, asserted as it is.
        assert (~c["is_true"]).sum() == 5 and o["kept"].all() and v[~c["is_true"]].min() > 0.75
    if name in WITH_INFO:
        assert np.array_equal(o["kept"], c["is_true"])
        err = np.abs(o["poses"] - c["truth"]).max()
        bound = 0.002 * max(np.abs(c["truth"][:, :3, 3]).max(), 1.0) + 0.002
        print("%s: %d loops, worst pose entry %.3g off the truth (bound %.3g), %d iterations, %d trials" % (name, len(v), err, bound, o["iterations"], o["trials"]))
        assert err < bound


@pytest.mark.parametrize("name", EM_CASES)
def test_fixture_margins_and_em_result(name):
    """No final EM weight in (0.15, 0.35) on any fixture; the kept set is the true set (with identity information every loop is kept, as in the
    switchable mode).  The poses are a robust estimate only (module docstring): they must be closer to the truth than the smallest offset of a
    false loop (0.3 x 0.5 m), that is, no false loop was followed."""
    c, o = pc.case(name), pc.solved(name, "em")
    v = o["values"]
    print("%s: EM weights of the true loops >= %.3f, of the false ones <= %.3f" % (name, v[c["is_true"]].min(), v[~c["is_true"]].max() if (~c["is_true"]).any() else 0.0))
    assert not ((v > 0.15) & (v < 0.35)).any(), v
    if name == "identity":
        assert o["kept"].all()
        return
    assert np.array_equal(o["kept"], c["is_true"])
    err = np.abs(o["poses"] - c["truth"]).max()
    print("%s: worst pose entry %.3g off the truth" % (name, err))
    assert err < 0.15


def test_output_files(tmp_path):
    """opt_output.log: entry i = (i, i, i + 1, X_i).  loop_remain.log: the kept entries unchanged.  refine.log: every odometry entry, then the kept
    entries with id1 + 1 < id2 (a reversed entry has id1 > id2 and stays out, as in the reference)."""
    c, o = pc.case("reverse"), pc.solved("reverse", "switchable")
    paths = pc.write_files(c, tmp_path)
    odo, loops = formats.load_log(paths["odometry"]), formats.load_log(paths["loop"])
    out = {k: str(tmp_path / k) for k in ("pose", "keep", "refine")}
    posegraph.write_outputs(odo, loops, o["poses"], o["kept"], out["pose"], out["keep"], out["refine"])
    pose, keep, refine = (formats.load_log(out[k]) for k in ("pose", "keep", "refine"))
    assert [(t.id1, t.id2, t.frame) for t in pose] == [(i, i, i + 1) for i in range(c["N"])]
    assert max(np.abs(t.T - X).max() for t, X in zip(pose, o["poses"])) < 1e-8
    kept = [t for t, k in zip(loops, o["kept"]) if k]
    same = lambda a, b: (a.id1, a.id2, a.frame) == (b.id1, b.id2, b.frame) and np.array_equal(a.T, b.T)
    assert len(keep) == len(kept) == int(c["is_true"].sum()) and all(same(a, b) for a, b in zip(keep, kept))
    far = [t for t in kept if t.id1 + 1 < t.id2]
    assert any(t.id1 > t.id2 for t in kept) and any(t.id1 + 1 == t.id2 for t in kept) and 0 < len(far) < len(kept)
    assert len(refine) == len(odo) + len(far) and all(same(a, b) for a, b in zip(refine, list(odo) + far))
    for k in out:                                                              # the round trip through formats is the identity on the bytes
        again = str(tmp_path / (k + "_again"))
        formats.save_log(again, formats.load_log(out[k]))
        assert open(again, "rb").read() == open(out[k], "rb").read()
    posegraph.write_outputs(odo, loops, o["poses"], o["kept"], out["pose"], out["keep"], None)     # the EM mode leaves refine.log alone
    assert len(formats.load_log(out["refine"])) == len(refine)


def test_refusals_that_need_no_device(tmp_path):
    """An .info list of another length than its .log is refused by name before any device is asked for; without a device every entry refuses."""
    c = pc.case("n6")
    with pytest.raises(_ffi.ErError, match="odometry information has 4 entries, the odometry 5"):
        posegraph.PoseGraph(c["odo_T"], (c["loop_ids"], c["loop_T"]), c["odo_info"][:4], c["loop_info"])
    with pytest.raises(_ffi.ErError, match="loop information has 3 entries, the loops 10"):
        posegraph.PoseGraph(c["odo_T"], (c["loop_ids"], c["loop_T"]), c["odo_info"], c["loop_info"][:3])
    paths = pc.write_files(c, tmp_path)
    formats.save_info(paths["loopinfo"], formats.load_info(paths["loopinfo"])[:-1])
    with pytest.raises(_ffi.ErError, match="result.info has 9 entries"):
        posegraph.graph_optimizer(paths["odometry"], paths["loop"], paths["odometryinfo"], paths["loopinfo"])
    exe = os.path.join(ROOT, "elasticreconstruction_amd", "bin", "GraphOptimizer")
    r = subprocess.run([exe, "--loop", "result.txt", "--loopinfo", "result.info"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "result.info has 9 entries, result.txt has 10" in r.stderr and not (tmp_path / "opt_output.log").exists()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--odometryinfo" in r.stdout
    r = subprocess.run([exe, "--odometry", "nothing.log"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not (tmp_path / "opt_output.log").exists()     # a missing odometry log: no work
    L = _ffi.lib()
    if L.er_device_count() <= 0:
        with pytest.raises(_ffi.ErError, match="no HIP device"):
            posegraph.PoseGraph(c["odo_T"], (c["loop_ids"], c["loop_T"]))
        for fn, args in ((L.er_pgo_optimize, (None, 0, 1.0, 1, None, None, None, None, None)), (L.er_pgo_set_state, (None, None, None)),
                         (L.er_pgo_get_state, (None, None, None)), (L.er_pgo_linearize, (None, 1.0, 0.0, None, None, None)),
                         (L.er_pgo_trial, (None, 1.0, 0.0, None, None, None, None))):
            assert fn(*args) != 0 and b"no HIP device" in L.er_last_error()
        formats.save_info(paths["loopinfo"], formats.load_info(paths["loopinfo"]) + formats.load_info(paths["loopinfo"])[:1])
        r = subprocess.run([exe, "--loop", "result.txt", "--loopinfo", "result.info"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "no HIP device" in r.stderr and not (tmp_path / "opt_output.log").exists()
