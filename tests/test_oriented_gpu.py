"""Oriented surface extraction on the GPU (k_surface_normals behind er_tsdf_extract_oriented) and the device hand-off to ICP
(er_cloud_create_from_tsdf): the kernel against the numpy restatement of tests/test_oriented_cpu.py bit for bit, against synth.kinfu_fragment
(the independent dense-grid statement), the cloud built on the device against the one built from the same rows through host memory, and
bin/Integrate --save_fragment against TSDFVolume.SaveFragment."""
import os
import subprocess

import numpy as np
import pytest
import torch

from elasticreconstruction_amd import formats, synth
from elasticreconstruction_amd.icp import Cloud, count_inliers, find_correspondence, icp_align
from elasticreconstruction_amd.tsdf import TSDFVolume
from test_oriented_cpu import compare_with_synth, nearest_voxel, oriented_oracle
from test_tsdf_gpu import _surface_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "elasticreconstruction_amd", "bin")


def fragment_volume(i, num, frames=50, noise_mm=0.0, length=3.0):
    """The volume synth.kinfu_fragment(i, num, frames=frames, noise_mm=noise_mm) integrates (same sweep, same depth images, same camera file),
    left open.  Returns (TSDFVolume, world_T_fragment)."""
    W = synth.kinfu_camera_path(i, num, frames)
    F = W[0] @ np.linalg.inv(synth.basepose(length))
    Finv = np.linalg.inv(F)
    seg = np.stack([Finv @ W[j] for j in range(frames)])
    depth = synth.render_depth(W, device="cuda:0")
    if noise_mm > 0:
        g = torch.Generator(device="cuda:0")
        g.manual_seed(int(synth.SEED) + 104729 * i + 17)
        d32 = depth.view(torch.int16).to(torch.int32) & 0xffff
        noisy = torch.round(d32.to(torch.float32) + noise_mm * torch.randn(d32.shape, generator=g, device="cuda:0")).clamp(1, 65535).to(torch.int32)
        d16 = torch.where(d32 > 0, noisy, d32).to(torch.int16)
        depth = d16 if depth.dtype == torch.int16 else d16.view(depth.dtype)
    torch.cuda.synchronize()
    cam = np.array([synth.CAM[0], synth.CAM[1], synth.CAM[2], synth.CAM[3], 2.5, 4.0], np.float32)
    vol = TSDFVolume(640, 480, cam, max_units=1024)
    vol.IntegrateFrames(None, seg, None, device_ptr=depth.data_ptr())
    vol.synchronize()
    return vol, F


def volume_from_units(units, max_units=64):
    """A TSDFVolume holding exactly `units` = {key: (sdf[262144], weight[262144])} (er_tsdf_import_raw)."""
    keys = np.array(sorted(units), np.int32)
    raw = np.stack([np.stack([units[int(k)][0], units[int(k)][1]]) for k in keys]).astype(np.float32)
    buf = torch.from_numpy(raw).to("cuda:0")
    torch.cuda.synchronize()
    vol = TSDFVolume(max_units=max_units)
    vol.import_raw(keys, buf.data_ptr())
    vol.synchronize()
    return vol


def check_against_restatement(vol, units, what):
    """extract_oriented: the points are extract_surface's, the normals the restatement's, bit for bit, NaN positions included.
    Returns the NaN share of the rows."""
    surf = vol.extract_surface()
    pts, nrm = vol.extract_oriented()
    assert pts.shape == surf.shape and nrm.shape == (surf.shape[0], 3) and nrm.dtype == np.float32
    assert np.array_equal(pts.view(np.uint32), surf.view(np.uint32)), what + ": points differ from er_tsdf_extract_surface"
    assert np.array_equal(surf.view(np.uint32), _surface_oracle(units).view(np.uint32)), what + ": point list differs from its restatement"
    want = oriented_oracle(units, surf)
    nan_g, nan_w = np.isnan(nrm), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), "%s: NaN positions differ on %d rows" % (what, int((nan_g != nan_w).any(axis=1).sum()))
    fin = ~nan_w.any(axis=1)
    bad = (nrm[fin].view(np.uint32) != want[fin].view(np.uint32)).any(axis=1)
    assert not bad.any(), "%s: %d of %d finite normals differ in their bits (max |d| %.3g)" % (
        what, int(bad.sum()), int(fin.sum()), float(np.abs(nrm[fin][bad] - want[fin][bad]).max()))
    v = nearest_voxel(surf)
    lower = np.floor(surf[:, :3].astype(np.float64) / (3.0 / 512.0) + 1e-9).astype(np.int64)
    print("%s: %d crossings, %.1f %% NaN normals, nearest voxel = upper end of the edge on %.1f %% of the rows"
          % (what, surf.shape[0], 100 * (~fin).mean(), 100 * (v != lower).any(axis=1).mean()))
    return float((~fin).mean())


def test_oriented_extraction_of_a_fragment_volume_matches_the_restatement(gpu):
    """(a) the 3-frame noisy fragment volume: several dozen units, every crossing's normal against the numpy restatement."""
    vol, _ = fragment_volume(3, 50, frames=3, noise_mm=2.0)
    units = {int(k): vol.read_unit(k) for k in vol.unit_keys()}
    assert len(units) > 50
    share = check_against_restatement(vol, units, "3-frame fragment")
    assert 0.005 < share < 0.5
    vol.close()


def hand_made_units(seed, base, holes=0.1):
    """A 2 x 2 x 2 block of units at unit index `base` (per axis) with random sdf values of random sign, a share `holes` of unobserved voxels,
    and one of the eight units absent."""
    rng = np.random.default_rng(seed)
    absent = int(rng.integers(0, 8))
    units = {}
    for c in range(8):
        if c == absent:
            continue
        xi, yi, zi = base[0] + (c & 1), base[1] + ((c >> 1) & 1), base[2] + (c >> 2)
        sdf = rng.uniform(-1.0, 1.0, 64 ** 3).astype(np.float32)
        w = (rng.random(64 ** 3) >= holes).astype(np.float32) * rng.integers(1, 50, 64 ** 3).astype(np.float32)
        units[xi << 18 | yi << 9 | zi] = (sdf, w)
    return units


@pytest.mark.parametrize("name,base", [("middle", (256, 255, 300)), ("far corner", (510, 510, 510)), ("near corner", (0, 0, 0))])
def test_oriented_extraction_of_hand_made_volumes_matches_the_restatement(gpu, name, base):
    """(b) random signs, random holes, an absent unit, in the middle of the lattice and against its far (unit index 511) and near (index 0)
    corners: every border branch of the fetch runs -- own unit, neighbouring unit through the hash map, unit that does not exist, outside
    the lattice.  Hole density 0.1: a normal needs five more observed voxels than its crossing does, 0.9^5 = 59 % finite."""
    units = hand_made_units(1234 + base[0], base)
    # the restatement alone, on the CPU: both kinds of rows are well represented
    surf = _surface_oracle(units)
    nan = np.isnan(oriented_oracle(units, surf)).any(axis=1)
    assert nan.mean() >= 0.10 and (~nan).mean() >= 0.10, nan.mean()
    vol = volume_from_units(units)
    share = check_against_restatement(vol, units, "hand-made volume, " + name)
    assert share >= 0.10 and 1.0 - share >= 0.10
    if name == "middle":
        # a unit handed over with er_tsdf_drop_units is absent: no points from it, its voxels unobserved for the neighbours' normals
        gone = sorted(units)[2]
        vol.drop_units([gone])
        rest = {k: u for k, u in units.items() if k != gone}
        check_against_restatement(vol, rest, "hand-made volume, one unit dropped")
    vol.close()


def test_oriented_extraction_agrees_with_the_kinfu_fragment_generator(gpu):
    """synth.kinfu_fragment (50 frames, the real generator: dense torch grid, central differences there) against extract_oriented on the same
    volume rebuilt through TSDFVolume: same points, same NaN pattern wherever the generator's grid reaches, normals within 1e-6."""
    i = 3
    x, n, F, st = synth.kinfu_fragment(i, 50, target_points=10 ** 9, density="tsdf")
    vol, F2 = fragment_volume(i, 50)
    assert np.array_equal(F, F2)
    pts, nrm = vol.extract_oriented()
    assert pts.shape[0] == st["zero_crossings"]
    fig = compare_with_synth(pts, nrm, x, n)
    assert fig["inside"] == st["inside_cube"] > 150000
    vol.close()


def host_route(vol, length, grid_cell=0.03):
    pts, nrm = vol.extract_oriented()
    x = pts[:, :3]
    ok = ~np.isnan(nrm[:, 0])
    if length > 0:
        ok &= ((x >= np.float32(0.0)) & (x < np.float32(length))).all(axis=1)
    return Cloud(np.ascontiguousarray(x[ok]), np.ascontiguousarray(nrm[ok]), grid_cell), int(ok.sum()), pts.shape[0]


def test_cloud_from_volume_equals_the_cloud_built_through_host_memory(gpu):
    """Cloud.from_volume (er_cloud_create_from_tsdf: filter and cloud build on the device) against Cloud(x[ok], n[ok]) from extract_oriented
    filtered on the host, for two overlapping kinfu-like fragments and a guess <= 2 deg / 2 cm off the ground truth: identical input rows must
    give identical results -- the search is exact and the ICP sums are exact fixed-point integers."""
    va, Fa = fragment_volume(3, 50)                                         # (sweeps 7.2 degrees apart; a third of their crossings lie outside the cube)
    vb, Fb = fragment_volume(4, 50, noise_mm=2.0)
    da, db = Cloud.from_volume(va), Cloud.from_volume(vb)
    (ha, na, ta), (hb, nb, tb) = host_route(va, 3.0), host_route(vb, 3.0)
    assert len(da) == len(ha) == na > 150000 and len(db) == len(hb) == nb > 150000
    T = np.linalg.inv(Fa) @ Fb @ synth.perturbation(700, 2.0, 0.02)
    cd, ch = count_inliers(db, da, T, 0.03), count_inliers(hb, ha, T, 0.03)
    assert cd == ch > 40000, (cd, ch)
    Td, itd, cvd, _ = icp_align(db, da, T.astype(np.float32))
    Th, ith, cvh, _ = icp_align(hb, ha, T.astype(np.float32))
    assert (itd, cvd) == (ith, cvh) and itd >= 1
    assert np.array_equal(Td.view(np.uint32), Th.view(np.uint32)), "final transforms differ by %.3g" % np.abs(Td - Th).max()
    pd_, idv = find_correspondence(db, da, Td.astype(np.float64), 0.015, 0.8660, want_info=True)
    ph, ihv = find_correspondence(hb, ha, Th.astype(np.float64), 0.015, 0.8660, want_info=True)
    assert pd_.shape[0] > 10000 and np.array_equal(pd_, ph) and np.array_equal(idv, ihv)
    assert np.abs(Td.astype(np.float64) - np.linalg.inv(Fa) @ Fb).max() < 2e-2
    # mixed use: a device-built source against a host-built target
    assert count_inliers(db, ha, T, 0.03) == cd
    # cube_length <= 0 keeps the points outside the cube
    whole = Cloud.from_volume(va, length=0.0)
    hw, nw, _ = host_route(va, 0.0)
    assert len(whole) == len(hw) == nw > na
    assert count_inliers(db, whole, T, 0.03) == count_inliers(hb, hw, T, 0.03) >= cd
    # another cube
    small = Cloud.from_volume(va, length=1.5)
    hs, ns, _ = host_route(va, 1.5)
    assert len(small) == ns and 0 < ns < na
    assert count_inliers(db, small, T, 0.03) == count_inliers(hb, hs, T, 0.03)
    for c in (da, db, ha, hb, whole, hw, small, hs):
        c.close()
    va.close()
    vb.close()


def test_cloud_from_a_volume_without_crossings_is_the_empty_cloud(gpu):
    x, n = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)
    tgt_x = (np.random.default_rng(5).random((5000, 3)) * 2 + 0.2).astype(np.float32)
    tgt = Cloud(tgt_x, np.tile(np.array([0, 0, 1], np.float32), (5000, 1)), 0.03)
    ref = Cloud(x, n, 0.03)
    fresh = TSDFVolume(max_units=8)                                           # no units at all
    free = volume_from_units({256 << 18 | 256 << 9 | 256: (np.ones(64 ** 3, np.float32), np.ones(64 ** 3, np.float32))}, 8)   # observed free space
    for vol in (fresh, free):
        pts, nrm = vol.extract_oriented()
        assert pts.shape == (0, 4) and nrm.shape == (0, 3)
        c = Cloud.from_volume(vol)
        assert len(c) == len(ref) == 0
        assert count_inliers(c, tgt, np.eye(4), 0.03) == count_inliers(ref, tgt, np.eye(4), 0.03) == 0
        assert count_inliers(tgt, c, np.eye(4), 0.03) == count_inliers(tgt, ref, np.eye(4), 0.03) == 0
        Tc, itc, cvc, _ = icp_align(c, tgt, np.eye(4, dtype=np.float32))
        Tr, itr, cvr, _ = icp_align(ref, tgt, np.eye(4, dtype=np.float32))
        assert (itc, cvc) == (itr, cvr) and np.array_equal(Tc, Tr)
        c.close()
        vol.close()


def test_integrate_program_save_fragment_equals_the_python_mirror(gpu, tmp_path):
    """bin/Integrate --save_fragment against TSDFVolume.SaveFragment on the same frames (rigid mode, raw stream): equal files; world.pcd is not
    touched by the option; refused with --gpus 2; and the finite normals point where the scene says (sphere outward, walls into the room)."""
    d = str(tmp_path)
    W = synth.kinfu_camera_path(3, 50, 50)[::10]                              # five frames of one sweep
    F = W[0] @ np.linalg.inv(synth.basepose())
    seg = [np.linalg.inv(F) @ w for w in W]
    depth = synth.to_numpy_u16(synth.render_depth(W))
    formats.save_log(os.path.join(d, "traj.log"), [formats.FramedTransformation(i, i, i + 1, seg[min(i, 4)]) for i in range(6)])
    depth.tofile(os.path.join(d, "frames.raw"))
    args = [os.path.join(BIN, "Integrate"), "--ref_traj", "traj.log", "-oni", "frames.raw", "--max_units", "512"]
    r0 = subprocess.run(args + ["--save_to", "w0.pcd"], cwd=d, capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    r1 = subprocess.run(args + ["--save_to", "w1.pcd", "--save_fragment", "frag.pcd"], cwd=d, capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stdout + r1.stderr
    assert open(os.path.join(d, "w0.pcd"), "rb").read() == open(os.path.join(d, "w1.pcd"), "rb").read()
    assert [l for l in r1.stdout.splitlines() if "fragment points have been written" not in l] == r0.stdout.splitlines()   # one more line, nothing else
    r2 = subprocess.run(args + ["--save_to", "w2.pcd", "--save_fragment", "frag2.pcd", "--gpus", "2", "--same_device"], cwd=d, capture_output=True,
                        text=True, timeout=300)
    assert r2.returncode != 0 and "--save_fragment" in r2.stderr and "--gpus" in r2.stderr, r2.stderr
    assert not os.path.exists(os.path.join(d, "w2.pcd")) and not os.path.exists(os.path.join(d, "frag2.pcd"))
    logged = formats.load_log(os.path.join(d, "traj.log"))
    vol = TSDFVolume(max_units=512)
    vol.IntegrateFrames(depth, np.stack([logged[f].T for f in range(5)]))
    m = vol.SaveFragment(os.path.join(d, "frag_py.pcd"))
    vol.close()
    a, b = formats.load_pcd(os.path.join(d, "frag.pcd")), formats.load_pcd(os.path.join(d, "frag_py.pcd"))
    names = ("x", "y", "z", "normal_x", "normal_y", "normal_z")
    A, B = np.stack([a[k] for k in names], 1).astype(np.float32), np.stack([b[k] for k in names], 1).astype(np.float32)
    assert A.shape == B.shape == (m, 6) and m > 50000 and "%d fragment points have been written." % m in r1.stdout
    assert np.array_equal(np.isnan(A), np.isnan(B)) and np.array_equal(A[~np.isnan(A)].view(np.uint32), B[~np.isnan(B)].view(np.uint32))
    x, n = A[:, :3], A[:, 3:]
    assert (x >= 0).all() and (x < 3.0).all()
    nan = np.isnan(n).any(axis=1)
    assert 0.005 < nan.mean() < 0.3 and np.isnan(n[nan]).all()                # kept in the file: CCorresApp::LoadData filters them
    ok = ~nan
    assert np.abs(np.linalg.norm(n[ok], axis=1) - 1).max() < 1e-5
    w = x[ok].astype(np.float64) @ F[:3, :3].T + F[:3, 3]
    nw = n[ok].astype(np.float64) @ F[:3, :3].T
    dw = np.minimum(np.abs(w - synth.ROOM_LO), np.abs(w - synth.ROOM_HI))
    ds = np.abs(np.linalg.norm(w - np.asarray(synth.SPHERE_C), axis=1) - synth.SPHERE_R)
    sph = ds < dw.min(axis=1)
    assert sph.sum() > 1000 and (~sph).sum() > 1000
    ns = w[sph] - np.asarray(synth.SPHERE_C)
    ns /= np.linalg.norm(ns, axis=1, keepdims=True)
    assert (nw[sph] * ns).sum(axis=1).mean() > 0.95
    ax = dw.argmin(axis=1)
    rows = np.arange(len(w))
    sgn = np.where(np.abs(w[rows, ax] - synth.ROOM_LO) < np.abs(w[rows, ax] - synth.ROOM_HI), 1.0, -1.0)
    assert (nw[rows, ax] * sgn)[~sph].mean() > 0.9
