"""Pose graph optimisation on the GPU (include/er_hip.h er_pgo_*, csrc/er_pgo.hip): GraphOptimizer's switchable-constraint
and EM modes (GraphOptimizer/OptApp.cpp) -- GlobalRegistration's candidate loop closures in, pruned closures and fragment poses out.
There is no CPU fallback."""
import ctypes as C
import os

import numpy as np

from . import _ffi, formats

METHODS = {"switchable": 0, "em": 1}      # ER_PGO_SWITCHABLE, ER_PGO_EM
KEEP = {"switchable": 0.5, "em": 0.25}    # an edge is kept when its switch / EM weight is above this (OptApp.cpp:142, 260)
TRIALS = 10                               # trials per LM iteration: the trace has at most TRIALS * max_iteration rows


def _stack(a, shape, what):
    a = np.ascontiguousarray(a, np.float64)
    if a.size == 0:
        return np.zeros((0,) + shape, np.float64)
    if a.size % int(np.prod(shape)):
        raise ValueError("%s must be a list of %s matrices" % (what, "x".join(str(s) for s in shape)))
    return np.ascontiguousarray(a.reshape((-1,) + shape))


class PoseGraph:
    """er_pgo_create.  odometry: [N - 1, 4, 4], edge i joins poses i and i + 1; loops: (ids [K, 2], T [K, 4, 4]);
    odometry_info / loop_info: [.., 6, 6] or None for the identity."""

    def __init__(self, odometry, loops, odometry_info=None, loop_info=None, device=0):
        self._lib = _ffi.lib()
        self._h = None
        odo = _stack(odometry, (4, 4), "odometry")
        ids, lt = loops if loops is not None else (np.zeros((0, 2), np.int32), np.zeros((0, 4, 4)))
        ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1, 2))
        lt = _stack(lt, (4, 4), "loops")
        if len(ids) != len(lt):
            raise _ffi.ErError("PoseGraph: %d loop id pairs for %d loop transforms" % (len(ids), len(lt)))
        oi = None if odometry_info is None else _stack(odometry_info, (6, 6), "odometry_info")
        li = None if loop_info is None else _stack(loop_info, (6, 6), "loop_info")
        if oi is not None and len(oi) != len(odo):
            raise _ffi.ErError("PoseGraph: the odometry information has %d entries, the odometry %d" % (len(oi), len(odo)))
        if li is not None and len(li) != len(lt):
            raise _ffi.ErError("PoseGraph: the loop information has %d entries, the loops %d" % (len(li), len(lt)))
        self.n_poses, self.n_loops, self.device = len(odo) + 1, len(lt), int(device)
        self.n = 6 * (self.n_poses - 1)
        h = C.c_void_p()
        p = lambda a: None if a is None or a.size == 0 else _ffi.ptr(a)
        _ffi.check(self._lib.er_pgo_create(self.n_poses, self.n_loops, p(odo), p(oi), p(ids), p(lt), p(li), self.device, C.byref(h)), "er_pgo_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.er_pgo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def optimize(self, method="switchable", weight=1.0, max_iteration=100):
        """er_pgo_optimize.  dict(poses [N, 4, 4], values [K] (switches, or the EM weights), kept [K] bool, iterations, trials,
        trace [trials, 4] = (lambda, F, F of the candidate, accepted))."""
        if method not in METHODS:
            raise ValueError("method must be 'switchable' or 'em'")
        poses = np.zeros((self.n_poses, 4, 4))
        values = np.zeros(max(self.n_loops, 1))
        trace = np.zeros((TRIALS * max(int(max_iteration), 0) + 1, 4))
        its, trials = C.c_int(0), C.c_int(0)
        _ffi.check(self._lib.er_pgo_optimize(self._h, METHODS[method], float(weight), int(max_iteration), _ffi.ptr(poses), _ffi.ptr(values), C.byref(its),
                                             C.byref(trials), _ffi.ptr(trace)), "er_pgo_optimize")
        values = values[:self.n_loops]
        return dict(poses=poses, values=values, kept=values > KEEP[method], iterations=its.value, trials=trials.value, trace=trace[:trials.value].copy())

    def profile(self, on=None):
        """er_pgo_set_profiling(on) if given; returns er_pgo_get_profile: the milliseconds of the last optimize by stage, summed over its trials."""
        if on is not None:
            _ffi.check(self._lib.er_pgo_set_profiling(self._h, int(bool(on))), "er_pgo_set_profiling")
        ms = np.zeros(5)
        _ffi.check(self._lib.er_pgo_get_profile(self._h, _ffi.ptr(ms)), "er_pgo_get_profile")
        return dict(zip(("linearise", "assemble", "factor", "solve", "evaluate"), ms))

    def state(self, poses=None, switches=None):
        """er_pgo_set_state for what is given, then er_pgo_get_state: (poses [N, 4, 4], switches [K])."""
        if poses is not None or switches is not None:
            P = None if poses is None else np.ascontiguousarray(poses, np.float64).reshape(self.n_poses, 16)
            S = None if switches is None else np.ascontiguousarray(switches, np.float64).reshape(self.n_loops)
            _ffi.check(self._lib.er_pgo_set_state(self._h, None if P is None else _ffi.ptr(P), None if S is None or S.size == 0 else _ffi.ptr(S)),
                       "er_pgo_set_state")
        P, S = np.zeros((self.n_poses, 4, 4)), np.zeros(max(self.n_loops, 1))
        _ffi.check(self._lib.er_pgo_get_state(self._h, _ffi.ptr(P), _ffi.ptr(S)), "er_pgo_get_state")
        return P, S[:self.n_loops]

    def linearize(self, weight=1.0, lam=0.0):
        """er_pgo_linearize at the current state: (H [n, n], b [n], chi2 [N - 1 + K])."""
        H, b, chi2 = np.zeros((self.n, self.n)), np.zeros(self.n), np.zeros(self.n_poses - 1 + self.n_loops)
        _ffi.check(self._lib.er_pgo_linearize(self._h, float(weight), float(lam), _ffi.ptr(H), _ffi.ptr(b), _ffi.ptr(chi2)), "er_pgo_linearize")
        return H, b, chi2

    def trial(self, weight=1.0, lam=0.0):
        """er_pgo_trial from the current state, which stays: (dx [n], ds [K], F_new, status)."""
        dx, ds = np.zeros(self.n), np.zeros(max(self.n_loops, 1))
        F, status = C.c_double(0.0), C.c_int(0)
        _ffi.check(self._lib.er_pgo_trial(self._h, float(weight), float(lam), _ffi.ptr(dx), _ffi.ptr(ds), C.byref(F), C.byref(status)), "er_pgo_trial")
        return dx, ds[:self.n_loops], F.value, status.value


def graph_optimizer(odometry_log, loop_log, odometry_info=None, loop_info=None, pose="opt_output.log", keep="loop_remain.log", refine="refine.log",
                    method="switchable", weight=1.0, iteration=100, device=0):
    """The file route of GraphOptimizer (GraphOptimizer.cpp, COptApp::Init / OptimizeSwitchable / OptimizeEM): reads the .log / .info files that
    bin/GlobalRegistration writes, and writes pose (entry i is (i, i, i + 1, X_i)), keep (the kept loop entries, unchanged) and, in the switchable
    mode, refine (every odometry entry, then the kept loop entries with id1 + 1 < id2) -- the file BuildCorrespondence --reg_traj reads.
    Missing .info files mean identity information; a missing or empty odometry log means no work (returns None)."""
    odo = formats.load_log(odometry_log) if odometry_log and os.path.exists(odometry_log) else []
    if not odo:
        return None
    loops = formats.load_log(loop_log) if loop_log and os.path.exists(loop_log) else []
    oi = formats.load_info(odometry_info) if odometry_info and os.path.exists(odometry_info) else []
    li = formats.load_info(loop_info) if loop_info and os.path.exists(loop_info) else []
    if oi and len(oi) != len(odo):
        raise _ffi.ErError("graph_optimizer: %s has %d entries, %s has %d" % (odometry_info, len(oi), odometry_log, len(odo)))
    if li and len(li) != len(loops):
        raise _ffi.ErError("graph_optimizer: %s has %d entries, %s has %d" % (loop_info, len(li), loop_log, len(loops)))
    g = PoseGraph(np.stack([t.T for t in odo]), (np.array([(t.id1, t.id2) for t in loops], np.int32).reshape(-1, 2),
                                                 np.stack([t.T for t in loops]) if loops else np.zeros((0, 4, 4))),
                  np.stack([i.info for i in oi]) if oi else None, np.stack([i.info for i in li]) if li else None, device=device)
    try:
        out = g.optimize(method, weight, iteration)
    finally:
        g.close()
    write_outputs(odo, loops, out["poses"], out["kept"], pose, keep, refine if method == "switchable" else None)
    return out


def write_outputs(odo, loops, poses, kept, pose, keep, refine=None):
    """The three files of COptApp::OptimizeSwitchable (OptApp.cpp:133-158; OptimizeEM writes the first two): pose -- entry i is
    (i, i, i + 1, X_i); keep -- the kept loop entries as they were read; refine -- every odometry entry, then the kept loop entries with
    id1 + 1 < id2."""
    formats.save_log(pose, [formats.FramedTransformation(i, i, i + 1, X) for i, X in enumerate(poses)])
    remain = [t for t, k in zip(loops, kept) if k]
    formats.save_log(keep, remain)
    if refine is not None:
        formats.save_log(refine, list(odo) + [t for t in remain if t.id1 + 1 < t.id2])
