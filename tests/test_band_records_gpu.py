"""The band-record kernels of the frame-split merge (k_band_count, k_band_pack, k_band_merge, k_band_import behind er_tsdf_band_sizes /
export_band / merge_band / import_band / drop_units) against the numpy restatement of tests/band_restatement.py, bit for bit: every voxel and
every defined word of every record.  The only words not compared are the padding behind the last weight and the last sdf value, which
k_band_pack does not write (band_restatement.defined_bits).  The only tolerance in this file is the project's 1e-5 for the sdf of a merged
volume against ONE volume that integrated the same frames, in the two-phase merge at the end.

Every record fed to import_band / merge_band comes from band_restatement.pack (checked on the CPU by tests/test_band_restatement.py) or from
export_band: a malformed record makes the kernels read outside it, and no test here builds one."""
import functools

import numpy as np
import pytest
import torch

import band_restatement as br
import helpers
from elasticreconstruction_amd import _ffi, parallel, synth
from elasticreconstruction_amd.tsdf import TSDFVolume
from oracle.pyoracle import OracleVolume
from test_oriented_gpu import fragment_volume, volume_from_units

pytestmark = pytest.mark.gpu
GUARD = 0x5a5a5a5a
PER = 100                                                          # frames per rank of the two-phase merge (two halves)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_unit(got, want, what):
    ns, nw = int((bits(got[0]) != bits(want[0])).sum()), int((bits(got[1]) != bits(want[1])).sum())
    assert ns == 0 and nw == 0, "%s: %d sdf and %d weight voxels differ in their bits" % (what, ns, nw)


def to_device(words):
    t = torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def to_host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def upload_records(recs):
    """Records back to back in one device block (each is a whole number of 8 bytes): (block, [device pointer of each])."""
    off = np.concatenate([[0], np.cumsum([r.size for r in recs])]).astype(np.int64)
    assert all(r.size % 2 == 0 for r in recs)
    block = to_device(np.concatenate(recs))
    return block, [block.data_ptr() + 4 * int(o) for o in off[:-1]]


def export_units(vol, keys):
    """band_sizes + export_band of `keys` in one call: (host words, sizes, device block, pointers).  Two guard words behind the block must survive."""
    sizes = vol.band_sizes(keys)
    total = int(sizes.astype(np.int64).sum())
    block = torch.full((total + 2,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    vol.export_band(keys, sizes, block.data_ptr())
    host = to_host(block)
    assert host[total] == GUARD and host[total + 1] == GUARD, "export_band wrote behind its block"
    off = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    return host[:total], sizes, block, [block.data_ptr() + 4 * int(o) for o in off[:-1]]


def split(host, sizes):
    off = np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))])
    return [host[int(off[i]):int(off[i + 1])] for i in range(len(sizes))]


@functools.lru_cache(maxsize=None)
def crafted():
    """{key: (name, unit, tags, record, what a record restores)} of the crafted units."""
    table = br.crafted_units()
    keys = br.crafted_keys(len(table))
    out = {}
    for k, (name, u, tags) in zip(keys, table):
        rec = br.pack(*u)
        out[k] = (name, u, tags, rec, br.unpack(rec))
    return out


def assert_crafted_inputs(c):
    """What the crafted units are for, on the inputs, before any device call."""
    head = [(int(v[3][0] & 1), int(v[3][1]), int(v[3][2])) for v in c.values()]
    assert {h[0] for h in head} == {0, 1}, "both weight formats"
    assert {h[1] % 4 for h in head if not h[0] and h[1] > 1000} == {0, 1, 2, 3} and {h[2] % 2 for h in head if h[1] > 1000} == {0, 1}
    assert {h[1] % 2 for h in head if h[0]} == {0, 1}, "wide records of odd and even counts"
    assert any(h[1] == 0 for h in head) and any(h[1] == br.UNIT_VOX and h[2] == 0 for h in head) and any(h[2] == br.UNIT_VOX for h in head)
    assert 0 in c and br.unit_key(511, 511, 511) in c
    assert any("moved_only" in v[2] for v in c.values()) and any("raw" in v[2] for v in c.values())


def test_export_band_equals_the_restatement(gpu):
    """(a) crafted units -> band_sizes -> export_band: every record, at its back-to-back offset, equals pack(u) in every defined bit; all units in one
    call, one call per unit, and the key list out of order (the block follows the caller's order)."""
    c = crafted()
    assert_crafted_inputs(c)
    vol = volume_from_units({k: v[1] for k, v in c.items()}, max_units=64)
    rng = np.random.default_rng(3)
    asc = sorted(c)
    for order in (asc, asc[::-1], [asc[int(i)] for i in rng.permutation(len(asc))]):
        sizes = vol.band_sizes(order)
        assert [int(s) for s in sizes] == [c[k][3].size for k in order] == [br.record_words(*c[k][1]) for k in order]
        host, sizes, _, _ = export_units(vol, order)
        for k, rec in zip(order, split(host, sizes)):
            bad = br.same_record(rec, c[k][3])
            assert bad == 0, "%s (key %d): %d words of the exported record differ from the restatement" % (c[k][0], k, bad)
    for k in asc:                                                   # one call per unit
        host, sizes, _, _ = export_units(vol, [k])
        assert host.size == c[k][3].size and br.same_record(host, c[k][3]) == 0, c[k][0]
    vol.close()


def test_import_band_restores_the_unit(gpu):
    """(b) pack(u) uploaded -> import_band into an empty volume, over a unit of the same key whose every voxel holds other data, and into a volume
    that dropped the key: read_unit equals unpack(pack(u)), and the volume lists the key."""
    c = crafted()
    assert_crafted_inputs(c)
    keys = sorted(c)
    rng = np.random.default_rng(4)
    order = [keys[int(i)] for i in rng.permutation(len(keys))]
    block, ptrs = upload_records([c[k][3] for k in order])
    stale = (rng.uniform(-1, 1, br.UNIT_VOX).astype(np.float32), np.full(br.UNIT_VOX, 7.0, np.float32))
    assert (stale[1] != 0).all()
    empty = TSDFVolume(max_units=64)
    other = volume_from_units({k: stale for k in keys}, max_units=64)
    dropped = volume_from_units({k: c[k][1] for k in keys}, max_units=64)
    dropped.drop_units(keys[::2])
    assert dropped.unit_count() == len(keys) - len(keys[::2])
    for what, vol, ks, ps in (("empty volume", empty, order, ptrs), ("over other data", other, order, ptrs),
                              ("dropped keys", dropped, [k for k in order if k in keys[::2]], [p for k, p in zip(order, ptrs) if k in keys[::2]])):
        vol.import_band(ks, ps)
        assert vol.unit_count() == len(keys) and [int(k) for k in vol.unit_keys()] == keys, what
        for k in ks:
            assert_same_unit(vol.read_unit(k), c[k][4], "%s, %s (key %d)" % (what, c[k][0], k))
    for k in keys[1::2]:                                            # the units next to the re-imported ones kept their bits
        assert_same_unit(dropped.read_unit(k), c[k][1], "neighbour of a re-imported unit, " + c[k][0])
    for v in (empty, other, dropped):
        v.close()
    del block


def units_of(vol):
    return {int(k): vol.read_unit(int(k)) for k in vol.unit_keys()}


def real_volume_with_an_unobserved_unit():
    vol, _ = fragment_volume(3, 50, frames=3, noise_mm=2.0)
    units = units_of(vol)
    if any(not u[1].any() for u in units.values()):
        return vol, units
    vol.close()                                                     # the scene that is known to allocate far units it never updates
    cam = np.array([517.3, 516.5, 318.6, 255.3, 2.5, 1.2], np.float32)
    poses = synth.circle_trajectory(3000)[7::500][:3]
    depth = synth.to_numpy_u16(synth.render_depth(poses, cam=tuple(cam[:4])))
    vol = TSDFVolume(camera=cam, max_units=256)
    vol.IntegrateFrames(depth, poses)
    return vol, units_of(vol)


def test_records_move_units_between_volumes_bit_for_bit(gpu):
    """(c) volume A -> export_band -> import_band of volume B straight from A's block: B's units are A's, for the crafted units (NaN, infinity
    included) and for a volume that came out of integration and holds an allocated, never-updated unit."""
    c = crafted()
    a = volume_from_units({k: v[1] for k, v in c.items()}, max_units=64)
    keys = sorted(c)
    _, _, block, ptrs = export_units(a, keys)
    b = TSDFVolume(max_units=64)
    b.import_band(keys, ptrs)
    assert [int(k) for k in b.unit_keys()] == keys
    for k in keys:
        got = a.read_unit(k)
        assert_same_unit(got, c[k][1], "import_raw / read_unit, " + c[k][0])
        assert_same_unit(b.read_unit(k), c[k][4] if "raw" in c[k][2] else got, "device to device, " + c[k][0])
    a.close()
    b.close()
    vol, units = real_volume_with_an_unobserved_unit()
    keys = sorted(units)
    zero_units = sum(1 for u in units.values() if not u[1].any())
    assert len(keys) >= 40 and zero_units >= 1, (len(keys), zero_units)
    assert [int(s) for s in vol.band_sizes(keys)] == [br.record_words(*units[k]) for k in keys]
    host, sizes, block, ptrs = export_units(vol, keys)
    for k, rec in zip(keys, split(host, sizes)):
        assert br.same_record(rec, br.pack(*units[k])) == 0, "unit %d of the integrated volume" % k
    b = TSDFVolume(max_units=1024)
    b.import_band(keys, ptrs)
    assert [int(k) for k in b.unit_keys()] == keys
    for k in keys:
        assert_same_unit(b.read_unit(k), units[k], "integrated volume, unit %d" % k)
    print("device to device: %d units of an integrated volume, %d of them never updated" % (len(keys), zero_units))
    vol.close()
    b.close()


def test_merge_band_equals_the_owners_sum(gpu):
    """(d) one owner volume, records from pack, merge_band against band_restatement.merge: nsrc in {0, 1, 2, 3, 7, 15, 16} x self_pos in
    {0, nsrc // 2, nsrc}, narrow and wide records in one sum, wide owners, disjoint / nested / identical / empty sources, weights that cancel,
    totals beyond 65535; six units with different nsrc and self_pos in one call, twelve in another.  The merged units then leave as records
    (wide where a total crossed 65535) and come back bit for bit."""
    pool, cases = br.merge_cases()
    recs = [br.pack(*u) for u in pool]
    want = {}
    for cs in cases:
        p = cs["self_pos"]
        want[cs["key"]] = br.merge(cs["own"], [recs[i] for i in cs["src"][:p]], [recs[i] for i in cs["src"][p:]])
    # the inputs hold what this test is for
    wide = [bool(r[0] & 1) for r in recs]
    assert sorted((len(cs["src"]), cs["self_pos"]) for cs in cases) == sorted((n, p) for n in (0, 1, 2, 3, 7, 15, 16) for p in {0, n // 2, n})
    assert max(len(cs["src"]) for cs in cases) == 16
    first = [cs for cs in cases if cs["call"] == 0]
    assert len(first) >= 5 and len({len(cs["src"]) for cs in first}) == len(first) == len({cs["self_pos"] for cs in first})
    assert any({wide[i] for i in cs["src"]} == {True, False} for cs in cases) and any(br.classify(*cs["own"])[2] for cs in cases)
    assert any(int(r[1]) == 0 for r in recs)
    crossing = [k for k, (s, w) in want.items() if w.max() > 65535]
    assert len(crossing) >= 3 and all(br.classify(*want[k])[2] for k in crossing)
    cancelled = [cs["key"] for cs in cases if 8 in cs["src"] and cs["own"][1][br.RESERVED].any()]
    assert len(cancelled) >= 2
    for k in cancelled:
        own = [cs for cs in cases if cs["key"] == k][0]["own"]
        gone = np.flatnonzero(own[1][br.RESERVED] == 3.0) + br.RESERVED.start
        assert gone.size == 16 and (bits(want[k][0])[gone] == 0).all() and (bits(want[k][1])[gone] == 0).all()
    assert all(np.isfinite(u[0]).all() and np.isfinite(u[1]).all() for u in pool + [cs["own"] for cs in cases])
    # the device
    owner = volume_from_units({cs["key"]: cs["own"] for cs in cases}, max_units=32)
    block, ptrs = upload_records(recs)
    state = {cs["key"]: cs["own"] for cs in cases}
    for call in (0, 1):
        batch = [cs for cs in cases if cs["call"] == call]
        owner.merge_band([cs["key"] for cs in batch], [[ptrs[i] for i in cs["src"]] for cs in batch], [cs["self_pos"] for cs in batch])
        for cs in batch:
            state[cs["key"]] = want[cs["key"]]
        for cs in cases:                                            # the merged ones and the ones this call had no business with
            assert_same_unit(owner.read_unit(cs["key"]), state[cs["key"]],
                             "call %d, unit with %d records, own position %d" % (call, len(cs["src"]), cs["self_pos"]))
    # the sums leave as records and come back
    keys = [cs["key"] for cs in cases]
    assert [int(s) for s in owner.band_sizes(keys)] == [br.record_words(*want[k]) for k in keys]
    host, sizes, out_block, out_ptrs = export_units(owner, keys)
    for k, rec in zip(keys, split(host, sizes)):
        assert br.same_record(rec, br.pack(*want[k])) == 0, "record of merged unit %d" % k
        assert bool(rec[0] & 1) == br.classify(*want[k])[2]
    assert all(split(host, sizes)[keys.index(k)][0] & 1 for k in crossing)
    back = TSDFVolume(max_units=32)
    back.import_band(keys, out_ptrs)
    for k in keys:
        assert_same_unit(back.read_unit(k), want[k], "merged unit %d after export_band -> import_band" % k)
    owner.close()
    back.close()
    del block, out_block


def test_band_calls_refuse_what_they_cannot_do(gpu):
    """(e) each refusal by its message."""
    c = crafted()
    keys = sorted(c)[:6]
    vol = volume_from_units({k: c[k][1] for k in keys}, max_units=8)
    absent = br.unit_key(300, 300, 300)
    assert absent not in c
    block = torch.zeros(1 << 20, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(_ffi.ErError, match="holds no unit"):
        vol.band_sizes([keys[0], absent])
    with pytest.raises(_ffi.ErError, match="holds no unit"):
        vol.export_band([absent], [16644], block.data_ptr())
    sizes = vol.band_sizes(keys[:2])
    with pytest.raises(_ffi.ErError, match="the caller planned for"):
        vol.export_band(keys[:2], [int(sizes[0]), int(sizes[1]) + 2], block.data_ptr())
    vol.drop_units([keys[1]])
    with pytest.raises(_ffi.ErError, match="holds no unit"):
        vol.band_sizes([keys[1]])
    with pytest.raises(_ffi.ErError, match="holds no unit"):
        vol.export_band([keys[0], keys[1]], [int(sizes[0]), int(sizes[1])], block.data_ptr())
    with pytest.raises(_ffi.ErError, match="handed to its owner"):
        vol.read_unit(keys[1])
    rec_block, ptrs = upload_records([c[keys[2]][3]])
    before = vol.read_unit(keys[0])
    with pytest.raises(_ffi.ErError, match=r"has 17 records \(at most 16\)"):
        vol.merge_band([keys[0]], [ptrs * 17], [0])
    with pytest.raises(_ffi.ErError, match=r"has 2 records \(at most 16\), own position 3"):
        vol.merge_band([keys[0]], [ptrs * 2], [3])
    with pytest.raises(_ffi.ErError, match="the owner holds no unit"):
        vol.merge_band([absent], [ptrs], [0])
    assert_same_unit(vol.read_unit(keys[0]), before, "a refused merge_band")
    vol.close()
    full = volume_from_units({k: c[k][1] for k in keys[:2]}, max_units=2)
    assert full.unit_count() == 2
    with pytest.raises(_ffi.ErError, match="pool exhausted"):
        full.import_band([keys[2]], ptrs)
    full.close()
    del block, rec_block


def test_dropped_units_until_the_next_integrated_frame(gpu):
    """(f) drop_units: the units leave unit_count / unit_keys / read_unit / band_sizes / the extractions, export_raw of them yields zeros.  The next
    er_tsdf_integrate_frames call with a frame brings ALL of them back, zeroed: the ones the frame touches hold that frame alone (the oracle's
    result on an empty volume), the others are allocated, never-updated units, as far units are after any integration."""
    poses = synth.circle_trajectory(3000)[7::500][:3]
    depth = synth.to_numpy_u16(synth.render_depth(poses, device="cuda:0"))
    vol, ora, alone = TSDFVolume(max_units=512), OracleVolume(), OracleVolume()
    vol.IntegrateFrames(depth, poses)
    for i in range(3):
        ora.Integrate(depth[i], poses[i])
    alone.Integrate(depth[0], poses[0])
    helpers.assert_volumes_identical(vol, ora, "three frames")
    keys = [int(k) for k in vol.unit_keys()]
    first = set(int(k) for k in alone.unit_keys())
    drop = keys[::2]
    touched, untouched = [k for k in drop if k in first], [k for k in drop if k not in first]
    assert len(touched) >= 3 and len(untouched) >= 3, (len(touched), len(untouched))
    kept = {k: vol.read_unit(k) for k in keys if k not in drop}
    vol.drop_units(drop)
    assert vol.unit_count() == len(keys) - len(drop) and [int(k) for k in vol.unit_keys()] == sorted(kept)
    for k in (touched[0], untouched[0]):
        with pytest.raises(_ffi.ErError, match="handed to its owner"):
            vol.read_unit(k)
        with pytest.raises(_ffi.ErError, match="holds no unit"):
            vol.band_sizes([k])
    raw = torch.full((len(drop), 2, br.UNIT_VOX), 1.5, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    vol.export_raw(drop, raw.data_ptr())
    vol.synchronize()
    assert int(torch.count_nonzero(raw.view(torch.int32))) == 0, "export_raw of dropped units"
    rest = volume_from_units(kept, max_units=512)                   # a volume that never held them extracts the same
    for f in ("extract_surface", "extract_world", "extract_mesh"):
        got, want = getattr(vol, f)(), getattr(rest, f)()
        assert got.shape == want.shape and got.shape[0] > 1000 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), f
    rest.close()
    # one more frame: frame 0 again
    vol.IntegrateFrames(depth[:1], poses[:1])
    ora.Integrate(depth[0], poses[0])
    assert [int(k) for k in vol.unit_keys()] == keys and vol.unit_count() == len(keys)
    zero = (np.zeros(br.UNIT_VOX, np.float32), np.zeros(br.UNIT_VOX, np.float32))
    for k in keys:
        if k in untouched:
            assert_same_unit(vol.read_unit(k), zero, "dropped unit %d, not touched by the frame" % k)
        elif k in touched:
            assert_same_unit(vol.read_unit(k), alone.read_unit(k), "dropped unit %d, touched by the frame" % k)
        else:
            assert_same_unit(vol.read_unit(k), ora.read_unit(k), "unit %d, never dropped" % k)
    assert sum(1 for k in touched if alone.read_unit(k)[1].any()) >= 3, "the frame must update dropped units, not only allocate them"
    assert [int(s) for s in vol.band_sizes(untouched)] == [br.HEADER] * len(untouched)
    vol.close()


@functools.lru_cache(maxsize=None)
def merge_scene():
    return helpers.merge_blocks(4, PER, [0, 0, 0, 0])


def integrate_part(vol, sc, lo, hi):
    part = sc["depth"][lo:hi]
    vol.IntegrateFrames(None, sc["traj"][lo:hi], synth.warp_arrays(sc, lo, hi), device_ptr=part.data_ptr())
    vol.synchronize()


@pytest.mark.parametrize("root", [-2, -1], ids=["then--2", "then--1"])
@pytest.mark.parametrize("order", ["first halves first", "alternating"])
def test_second_merge_on_live_volumes(gpu, order, root):
    """(f) four loopback ranks integrate one half of their blocks, merge distributed, integrate the other half on top and merge again (left
    distributed, or onto every rank).  Every unit two or more ranks held before the second merge -- the zeroed units a rank got back when it
    integrated after handing them over count -- is the rank-ordered float32 sum of the read-back states, bit for bit; every unit one rank held
    is untouched; and against ONE volume that integrated the same frames the key set and the weights are equal, the sdf within 1e-5.
    "first halves first": every rank starts with the first half of its block.  The halves of neighbouring ranks are then 50 frames apart and share
    no unit, so the first merge has nothing to sum or hand over.  "alternating": the even ranks start with their second half, which borders the odd
    ranks' first half, so the first merge sums and hands units over, and the second one meets the copies that came back zeroed."""
    blocks = merge_scene()
    G, half = 4, PER // 2
    part = lambda r, phase: (half, PER) if (phase == 1) != (order == "alternating" and r % 2 == 0) else (0, half)
    full = TSDFVolume(max_units=2048)
    vols = [TSDFVolume(max_units=2048) for _ in range(G)]
    comms = parallel.LoopbackComms(G)
    try:
        for phase in (0, 1):
            for r, (sc, _) in enumerate(blocks):
                integrate_part(full, sc, *part(r, phase))
        for r, (v, (sc, _)) in enumerate(zip(vols, blocks)):
            integrate_part(v, sc, *part(r, 0))
        n1 = comms.allreduce(vols, root=parallel.MERGE_DISTRIBUTED)
        after1 = [set(int(k) for k in v.unit_keys()) for v in vols]
        assert sum(len(s) for s in after1) == len(set().union(*after1)) == n1, "a distributed merge leaves every unit on one rank"
        handed = [comms.merge_stats(r)["units_handed_over"] for r in range(G)]
        if order == "alternating":
            assert sum(handed) >= 3, handed
        for r, (v, (sc, _)) in enumerate(zip(vols, blocks)):
            integrate_part(v, sc, *part(r, 1))
        before = [units_of(v) for v in vols]
        for r in range(G):                                          # what a rank handed over came back with the next frame
            assert len(before[r]) >= len(after1[r]) + handed[r]
        touch = {}
        for r, b in enumerate(before):
            for k in b:
                touch.setdefault(k, []).append(r)
        multi = sorted(k for k, t in touch.items() if len(t) >= 2)
        single = sorted(k for k, t in touch.items() if len(t) == 1)
        full_keys = [int(k) for k in full.unit_keys()]
        assert sorted(touch) == full_keys
        assert len(multi) >= 20 and len(single) >= 100, (len(multi), len(single))
        returned = sum(1 for k in multi for r in touch[k] if not before[r][k][1].any())
        assert returned >= sum(handed), (returned, handed)          # a handed-over unit is back, zeroed, next to its owner's copy
        n2 = comms.allreduce(vols, root=root)
        assert n2 == len(touch)
        have = [set(int(k) for k in v.unit_keys()) for v in vols]
        assert set().union(*have) == set(full_keys)
        worst = 0.0
        for k in full_keys:
            holders = [r for r in range(G) if k in have[r]]
            if root == parallel.MERGE_DISTRIBUTED:
                assert len(holders) == 1 and holders[0] in touch[k], "unit %d lives on ranks %s" % (k, holders)
            else:
                assert holders == list(range(G)), "unit %d lives on ranks %s" % (k, holders)
            if len(touch[k]) == 1:
                want = before[touch[k][0]][k]
            else:
                t = touch[k]
                want = br.merge(before[t[0]][k], [], [before[r][k] for r in t[1:]])
            for r in holders:
                assert_same_unit(vols[r].read_unit(k), want, "unit %d held by ranks %s, on rank %d" % (k, touch[k], r))
            sf, wf = full.read_unit(k)
            assert np.array_equal(wf, want[1]), "weights of unit %d differ from the single volume" % k
            worst = max(worst, float(np.abs(sf - want[0]).max()))
        print("second merge (%s, root %d, %d frames per rank): the first merge handed over %d units; %d units, %d held by several ranks (%d zeroed "
              "copies among them), %d by one; worst |sdf - single volume| = %.3g"
              % (order, root, PER, sum(handed), len(touch), len(multi), returned, len(single), worst))
        assert worst <= 1e-5, "merged tsdf differs by %.3g" % worst
    finally:
        comms.close()
        full.close()
        for v in vols:
            v.close()
