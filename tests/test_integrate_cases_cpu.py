"""The conditions on the fixtures of tests/integrate_cases.py, proven without a GPU on the host twin of k_integrate (tests/hostcheck, patch
shape 3 = the kernel's 8 x 4 x 8 wave box, with the path tally): every fixture is bit-identical to the oracle frame by frame, no verdict is
violated, the walk through the kernel's frame loop ends in the replay's bits, and every path event a fixture declares is reached -- in the plain
build and with a box-verdict reciprocal that is off by 1 and 2 ulps either way, so that the device's v_rcp_f32 cannot take a fixture off its path.
These are conditions, not measurements: a fixture that misses an event is changed, not the list.  tests/test_integrate_paths_gpu.py then holds the
kernel to the same references on the same inputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
import integrate_cases as IC
import prepass_restatement as R
from elasticreconstruction_amd import tsdf
from integrate_restatement import RestatedVolume
from oracle.pyoracle import OracleVolume

HERE = os.path.dirname(os.path.abspath(__file__))
vp = C.c_void_p
CASES = IC.all_cases()
ULPS = [0, -2, -1, 1, 2]


def load_hostcheck(ulps, out_dir):
    """tests/hostcheck built the way tests/test_hostcheck.py builds it; ulps != 0: -DER_FAST_CULL_HOSTSIM=(ulps)."""
    src = os.path.join(HERE, "hostcheck", "tsdf_hostcheck.cpp")
    out = os.path.join(str(out_dir), "libhc_cases_%d.so" % ulps)
    extra = ["-DER_FAST_CULL_HOSTSIM=(%d)" % ulps] if ulps else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"] + extra + [src, "-o", out], check=True)
    L = C.CDLL(out)
    L.hc_create.restype = vp
    L.hc_create.argtypes = [C.c_int, C.c_int, vp]
    L.hc_destroy.argtypes = [vp]
    L.hc_integrate_frames.argtypes = [vp, C.c_int, vp, vp, vp]
    L.hc_unit_count.argtypes = [vp]
    L.hc_unit_keys.argtypes = [vp, vp]
    L.hc_read_unit.argtypes = [vp, C.c_int, vp, vp]
    L.hc_write_unit.restype = None
    L.hc_write_unit.argtypes = [vp, C.c_int, vp, vp]
    L.hc_events.restype = None
    L.hc_events.argtypes = [vp, vp]
    L.hc_event_name.restype = C.c_char_p
    L.hc_event_name.argtypes = [C.c_int]
    for name in ("hc_inside_violations", "hc_full_violations", "hc_sure_violations", "hc_walk_violations", "hc_inside", "hc_full", "hc_sure", "hc_culled", "hc_kept"):
        getattr(L, name).restype = C.c_long
        getattr(L, name).argtypes = [vp]
    L.hc_set_patch_shape.restype = None
    L.hc_set_patch_shape.argtypes = [C.c_int]
    L.hc_set_patch_shape(3)                                 # (a library of this module's own: the setting stays)
    return L


def event_names(L):
    return [L.hc_event_name(e).decode() for e in range(L.hc_event_count())]


class Replay:
    """One fixture on the host twin: frame by frame against a reference (call by call for the tally), as the library cuts the stream."""

    def __init__(self, L, case):
        self.L, self.case = L, case
        cam = np.ascontiguousarray(case["cam"], np.float32)
        self.h = vp(L.hc_create(case["cols"], case["rows"], cam.ctypes.data_as(vp)))
        self.events = np.zeros(L.hc_event_count(), np.int64)
        for k, (sdf, w) in (case["preset"] or {}).items():
            s, ww = np.ascontiguousarray(sdf, np.float32), np.ascontiguousarray(w, np.float32)
            L.hc_write_unit(self.h, int(k), s.ctypes.data_as(vp), ww.ctypes.data_as(vp))

    def integrate(self, a, b):
        depth = np.ascontiguousarray(self.case["depth"][a:b])
        T = np.ascontiguousarray(self.case["poses"][a:b], np.float64).reshape(-1, 16)
        Ti = np.ascontiguousarray(np.stack([tsdf._inverse(t) for t in T.reshape(-1, 4, 4)]).reshape(-1, 16))
        assert self.L.hc_integrate_frames(self.h, b - a, depth.ctypes.data_as(vp), T.ctypes.data_as(vp), Ti.ctypes.data_as(vp)) == 0
        ev = np.zeros(self.L.hc_event_count(), C.c_long)
        self.L.hc_events(self.h, ev.ctypes.data_as(vp))
        self.events += ev

    def run(self):
        for a, b in library_batches(self.case):
            self.integrate(a, b)
        return self

    def unit_keys(self):
        k = np.empty(self.L.hc_unit_count(self.h), np.int32)
        self.L.hc_unit_keys(self.h, k.ctypes.data_as(vp))
        return k

    def read_unit(self, key):
        s, w = np.empty(64 ** 3, np.float32), np.empty(64 ** 3, np.float32)
        assert self.L.hc_read_unit(self.h, int(key), s.ctypes.data_as(vp), w.ctypes.data_as(vp)) == 0
        return s, w

    def violations(self):
        return {n: getattr(self.L, "hc_%s_violations" % n)(self.h) for n in ("inside", "full", "sure", "walk")}

    def close(self):
        self.L.hc_destroy(self.h)


def library_batches(case):
    """The launches of k_integrate: the fixture's calls, each cut at 64 frames."""
    return [(a + x, a + y) for a, b in case["calls"] for x, y in IC.batches(b - a)]


def reference(case):
    """The volume the fixture must end in: the oracle from the empty state, the restatement from a preset one."""
    if case["preset"] is None:
        ref = OracleVolume(case["cols"], case["rows"], case["cam"])
    else:
        ref = RestatedVolume(case["cols"], case["rows"], case["cam"], case["preset"])
    for f in range(case["depth"].shape[0]):
        ref.Integrate(case["depth"][f], case["poses"][f])
    return ref


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("hc_cases")
    return {u: load_hostcheck(u, d) for u in ULPS}


@pytest.fixture(scope="module")
def tallies(libs):
    """{(case name, ulps): events} of every fixture in every build, computed once."""
    out = {}
    for case in CASES:
        for u in ULPS:
            rp = Replay(libs[u], case).run()
            assert rp.violations() == dict(inside=0, full=0, sure=0, walk=0), (case["name"], u, rp.violations())
            out[(case["name"], u)] = dict(zip(event_names(libs[u]), (int(e) for e in rp.events)))
            rp.close()
    return out


def fresh_reference(case):
    if case["preset"] is None:
        return OracleVolume(case["cols"], case["rows"], case["cam"])
    return RestatedVolume(case["cols"], case["rows"], case["cam"], case["preset"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_replay_equals_reference_frame_by_frame(libs, case):
    """Host replay at the kernel's box == the reference, bit for bit and with equal key sets: handed over frame by frame and compared after every
    frame, and handed over in the launches the library makes of the fixture's calls and compared after every launch.  No inside / full / sure
    verdict violated; the walk through the kernel's frame loop ends in the replay's bits."""
    n = case["depth"].shape[0]
    ways = [[(f, f + 1) for f in range(n)], library_batches(case)]
    if case["preset"] is not None:
        # One launch only: the planted weight 2^24 - 1 saturates in frame 0, and a LAUNCH that starts at 2^24 is outside k_integrate's domain
        # ("apply_full"): a band frame then moves sdf_ in the reference while weight_ stays, and the store predicate W != W0 drops the
        # row.  Handed over frame by frame the walk reports exactly that (64 voxels behind the 0.95 m surface) -- it is how the limit was measured.
        ways = ways[1:]
    for launches in ways:
        rp, ref = Replay(libs[0], case), fresh_reference(case)
        for a, b in launches:
            rp.integrate(a, b)
            for f in range(a, b):
                ref.Integrate(case["depth"][f], case["poses"][f])
            helpers.assert_volumes_identical(rp, ref, "%s after frame %d" % (case["name"], b - 1))
        assert rp.violations() == dict(inside=0, full=0, sure=0, walk=0)
        rp.close()


def test_far_100_sees_depth_beyond_64_m():
    """The scaled depth k_integrate<false> alone may see: above voxel_classify's 64 m bound, in frames that are band for some box."""
    case = next(c for c in CASES if c["name"] == "far-100")
    sc = R.scale_depth(case["depth"], case["cam"], case["cols"], case["rows"])
    assert (sc.max(axis=1) > 64.0).sum() == 2 and (sc.min(axis=1) > 0).all()
    ref = reference(case)
    S, W = ref.read_unit(IC.key(260, 260, 428))
    assert ((W > 0) & (S < 1)).any()                          # the 64.5 m frame left band values


def test_preset_states_meet_the_runs_they_are_planted_for():
    """Every planted box is in front of every surface for frames 0 .. 3 (a run of four full frames) and in the band later: the reference holds
    W + 12 there where that is exact, and the saturated 2^24 where W started at 2^24 - 1."""
    case = next(c for c in CASES if c["name"] == "preset")
    S, W = reference(case).read_unit(IC.K_MID)
    W = W.reshape(64, 64, 64)
    for (i0, j0, k0), (s, w) in IC.PRESET_STATES:
        box = W[i0:i0 + 8, j0:j0 + 4, k0:k0 + 8]
        assert (box == (np.float32(w) + np.float32(12) if w < 2 ** 24 - 1 else np.float32(2 ** 24))).all(), (i0, j0, k0, np.unique(box))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_declared_event_is_reached_in_every_build(tallies, case):
    for u in ULPS:
        t = tallies[(case["name"], u)]
        missing = [e for e in case["events"] if t[e] < 1]
        assert not missing, "%s (reciprocal %+d ulps) misses %s: %s" % (case["name"], u, missing, t)
        if float(case["cam"][5]) >= 64.0:
            assert all(t[e] == 0 for e in IC.SURE_EVENTS), (case["name"], t)


def test_union_of_events(tallies, libs):
    names = event_names(libs[0])
    for u in ULPS:
        every = {e for c in CASES for e in names if tallies[(c["name"], u)][e] > 0}
        assert every == set(names), sorted(set(names) - every)
        nosure = {e for c in IC.no_sure_cases(CASES) for e in names if tallies[(c["name"], u)][e] > 0}
        assert nosure == set(names) - set(IC.SURE_EVENTS), (u, sorted(set(names) - nosure), sorted(nosure & set(IC.SURE_EVENTS)))
    declared = {e for c in CASES for e in c["events"]}
    assert declared == set(names), sorted(set(names) - declared)
    assert {e for c in IC.no_sure_cases(CASES) for e in c["events"]} == set(names) - set(IC.SURE_EVENTS)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_units_stay_in_their_masks(case):
    """What k_prepare must hand over (tests/prepass_restatement.py): the unit keys and frame masks the fixture says, batch by batch."""
    bs = library_batches(case)
    assert len(bs) == len(case["masks"])
    for (a, b), want in zip(bs, case["masks"]):
        if not want:                                        # a call without a depth pixel
            assert not case["depth"][a:b].any()
            continue
        p = R.products(case["depth"][a:b], case["poses"][a:b], case["cam"], case["cols"], case["rows"])
        got = {int(k): int(m) for k, m in zip(p["keys"], p["masks"])}
        assert got == want and p["out_of_range"] == 0, (case["name"], a, b, got)


@pytest.mark.parametrize("case", [c for c in CASES if c["preset"] is None], ids=lambda c: c["name"])
def test_restatement_reproduces_the_oracle_from_the_empty_state(case):
    res, ora = RestatedVolume(case["cols"], case["rows"], case["cam"]), OracleVolume(case["cols"], case["rows"], case["cam"])
    for f in range(case["depth"].shape[0]):
        res.Integrate(case["depth"][f], case["poses"][f])
        ora.Integrate(case["depth"][f], case["poses"][f])
    helpers.assert_volumes_identical(res, ora, "restatement / " + case["name"])
    assert res.sum_weight() == ora.sum_weight()
