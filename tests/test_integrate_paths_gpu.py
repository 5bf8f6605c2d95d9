"""k_integrate, both instantiations, on the crafted fixtures of tests/integrate_cases.py: TSDFVolume.IntegrateFrames, handed over in the fixture's
calls, against OracleVolume.Integrate frame by frame (a preset state: against tests/integrate_restatement.py) -- bit patterns of sdf_ and weight_
and equal key sets, as everywhere in path A; no tolerance.  tests/test_integrate_cases_cpu.py proves on the host twin which paths of the frame
loop each fixture walks (pipeline exits, runs of full frames, both branches of apply_full, the sure test, the zero pad, mask bit 63) and that the
device's one-ulp reciprocal cannot take it off them; here er_tsdf_prepass_trace shows that the device hands k_integrate the unit keys and frame
masks those proofs start from.  The paths are proven on the CPU, the GPU is held to the values."""
import numpy as np
import pytest

import helpers
import integrate_cases as IC
from elasticreconstruction_amd.tsdf import TSDFVolume
from integrate_restatement import RestatedVolume
from oracle.pyoracle import OracleVolume

pytestmark = pytest.mark.gpu

CASES = IC.all_cases()
_refs = {}


def reference(case):
    """Computed once per input (the three cuts share theirs), never written again."""
    name = "cuts" if case["name"].startswith("cuts-") else case["name"]
    if name not in _refs:
        if case["preset"] is None:
            ref = OracleVolume(case["cols"], case["rows"], case["cam"])
        else:
            ref = RestatedVolume(case["cols"], case["rows"], case["cam"], case["preset"])
        for f in range(case["depth"].shape[0]):
            ref.Integrate(case["depth"][f], case["poses"][f])
        _refs[name] = ref
    return _refs[name]


def plant(vol, preset):
    """The preset state through er_tsdf_import_raw, the route by which the multi-GPU paths hand units over."""
    import torch
    keys = np.array(sorted(preset), np.int32)
    raw = np.stack([np.stack([preset[int(k)][0], preset[int(k)][1]]) for k in keys]).astype(np.float32)
    buf = torch.from_numpy(raw).to("cuda:0")
    torch.cuda.synchronize()
    vol.import_raw(keys, buf.data_ptr())
    vol.synchronize()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_bit_identical_to_reference(gpu, case):
    cols, rows, cam = case["cols"], case["rows"], case["cam"]
    vol = TSDFVolume(cols, rows, cam, max_units=16)
    if case["preset"] is not None:
        plant(vol, case["preset"])
    for a, b in case["calls"]:
        vol.IntegrateFrames(case["depth"][a:b], case["poses"][a:b])
    vol.synchronize()
    ref = reference(case)
    helpers.assert_volumes_identical(vol, ref, case["name"])
    assert vol.status() == (0, 0)
    assert vol.sum_weight() == ref.sum_weight()
    vol.close()
    # the fixture arrives at k_integrate as designed: the device's unit keys and frame masks, launch by launch
    launches = [(a + x, a + y) for a, b in case["calls"] for x, y in IC.batches(b - a)]
    assert len(launches) == len(case["masks"])
    tv = TSDFVolume(cols, rows, cam, max_units=16)
    for (a, b), want in zip(launches, case["masks"]):
        tr = tv.prepass_trace(case["depth"][a:b], case["poses"][a:b])
        assert {int(k): int(m) for k, m in zip(tr["keys"], tr["masks"])} == want, (case["name"], a, b)
    assert tv.status() == (0, 0)
    tv.close()


def test_both_instantiations_are_among_the_fixtures():
    """er_tsdf.hip picks k_integrate<true> for integration_trunc < 64 and k_integrate<false> from 64 on: fixtures on both sides of the bound, at
    the bound and at the largest float below it."""
    t = sorted({float(c["cam"][5]) for c in CASES})
    assert t == [2.5, IC.TRUNC_BELOW_64, 64.0, 100.0] and IC.TRUNC_BELOW_64 < 64.0
