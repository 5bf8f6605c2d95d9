"""What two correct float64 evaluations of the linearisation of tests/posegraph_restatement.py can differ by, in units of 2^-53: sums of
absolute values of what is added.  Test bookkeeping, kept out of the model's restatement.

    input_terms         taken down to the inputs.  r is what is left of isometry entries of size 1 and translations of size tt (the 1-norms of the
                        three translations involved), so a translation entry of r carries tt and a quaternion entry 1 whatever its own size; a
                        Jacobian entry carries 1 (rotation and quaternion entries; dt/dq_i = R_A 2 [t_B]x another 2 tt) unless it is a structural
                        zero; the Schur terms carry the errors of Hps, bs and Hss.  Meaningful at any state.
    contribution_terms  the absolute values of the edges' contributions to an entry's block, and sum |r_a Om_ab r_b| for chi2: the bound of two
                        ORDERS of adding the contributions.  It says nothing where a contribution is itself a cancelled sum (a structural zero, or
                        the residual of an odometry edge at the initial state, which is pure rounding; an entry of J^T Om J at any state): use it for b and chi2
                        at a perturbed state.
"""
import numpy as np

import posegraph_restatement as pr


def _assemble(g, Hs, gs):
    H, b = np.zeros((g.n, g.n)), np.zeros(g.n)
    for e in range(g.E):
        v = [g.ids[e][0] - 1, g.ids[e][1] - 1]
        for p in range(2):
            if v[p] < 0:
                continue
            b[6 * v[p]:6 * v[p] + 6] += gs[e][6 * p:6 * p + 6]
            for q in range(2):
                if v[q] >= 0:
                    H[6 * v[p]:6 * v[p] + 6, 6 * v[q]:6 * v[q] + 6] += Hs[e][6 * p:6 * p + 6, 6 * q:6 * q + 6]
    return H, b


def contribution_terms(g, recs):
    """(Ha [n, n], ba [n], chi2a [E]) from the records of g.linearize at g's state"""
    Ha, ba = _assemble(g, [np.abs(R["H"]) for R in recs], [np.abs(R["g"]) for R in recs])
    ca = np.zeros(g.E)
    for e in range(g.E):
        r = pr.residual(g.Z[e], g.poses[g.ids[e][0]], g.poses[g.ids[e][1]])
        ca[e] = np.abs(np.outer(r, r) * (g.scale[e] * g.Om[e])).sum()
    return Ha, ba, ca


def input_terms(g, w, lam, switchable=True):
    """(Ha [n, n], ba [n], chi2a [E]) at g's state"""
    Hs, gs, ca = [], [], np.zeros(g.E)
    for e in range(g.E):
        i, j = g.ids[e]
        r, Ji, Jj = pr.jacobians(g.Z[e], g.poses[i], g.poses[j])
        tt = np.abs(g.Z[e][:3, 3]).sum() + np.abs(g.poses[i][:3, 3]).sum() + np.abs(g.poses[j][:3, 3]).sum()
        is_sw = switchable and e >= g.n_odo
        s = g.sw[e - g.n_odo] if is_sw else 1.0
        Oa = np.abs(g.scale[e] * g.Om[e])
        rh = np.abs(r) + np.array([tt, tt, tt, 1.0, 1.0, 1.0])
        Jh = np.abs(np.hstack([Ji, Jj]))
        Jh[:3, 3:6] += 2.0 * tt
        for rows, cols in ((0, 0), (3, 3), (0, 6), (3, 9)):      # every block that is not a structural zero is made of rotation entries of size 1
            Jh[rows:rows + 3, cols:cols + 3] += 1.0
        Jh *= s
        gh, c2h = Jh.T @ Oa @ rh, rh @ Oa @ rh
        ca[e] = c2h
        if not is_sw:
            Hs.append(Jh.T @ Oa @ Jh)
            gs.append(gh)
            continue
        chi2 = r @ (g.scale[e] * g.Om[e]) @ r
        hss = chi2 + w + lam
        bsh = s * c2h + w * (1.0 - s)
        Hs.append(Jh.T @ Oa @ Jh + np.outer(gh, gh) / hss * (1.0 + c2h / hss))
        gs.append(s * gh + gh * bsh / hss * (1.0 + c2h / hss))
    return _assemble(g, Hs, gs) + (ca,)
