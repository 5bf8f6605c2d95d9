"""The depth-odometry kernels (csrc/er_odom.hip, csrc/er_odom_math.h) at their shape, level and data edges, against the numpy
restatement (tests/odometry_restatement.py) built with the library's tables.  tests/test_odometry_gpu.py drives them with smooth renders at
two sizes, three levels and small motions; here:
  - launch geometry: a workgroup of k_odom_iter takes 1024 pixels and k_odom_final adds the partial vectors in 8 strided slices -- levels of
    exactly 1024 and of 1025 pixels, of 8 and of 9 workgroups, of less than one workgroup, less than one wave and of one pixel
    (odometry_cases.SHAPES);
  - levels 1, 2 and 4 (level 3 has offsets, intrinsics and an iteration count of its own), iteration counts of 0, a schedule of none;
  - the device build of the per-pixel header on noise, steps, holes, the last entry of the depth-weight table at the corner of the window
    and on every border, depths of 1 .. 3 and of 32767 | 32768 .. 65535 (from host uint16 and from device int16 frames);
  - poses that send a quarter to three quarters of the pixels out through one border, behind the camera, onto the mirrored pixel, and poses
    that are not finite;
  - a pair that is lost part-way (a comb frame: dense at level 2, no normal at levels 1 and 0) alone and between healthy pairs;
  - the 6 x 6 solve and the pose update alone, from the device's own sums, against a longdouble restatement.
tests/test_odometry_cpu.py checks on the restatement that every fixture is on the edge it is meant for.

Two borders of the header cannot show on the device and are pinned on its host build there: the model maps that k_odom_maps writes have no
normal in the last column and row (so `pu <= cols - 1` and `pu < cols - 1` match the same pixels), and the device's depth-weight table is zero
beyond its end (so reading the entry after the end adds +0).  Likewise whether a lost pair's workgroups run or return changes no output:
thread 0 of k_odom_final ignores the totals of a lost pair.

MEASURED on one MI355X (worst |device sum - restatement sum| / (count 2^-53 sum |terms|) over levels, poses and the 27 sums; the bound is 1):
    32 x 32   0.0034    41 x 25   0.0033    40 x 26   0.015     128 x 64  0.00035   129 x 64  0.00036   70 x 50   0.0030
    96 x 64   0.029     80 x 56   0.056     16 x 12   0.018     5 x 3     0 (4 matches)       1 x 1     0 (no match)
    border poses: 72 x 52  0.056, 129 x 64  0.0037
The solve alone (worst over the three sizes and the two guesses): e = |float64 step - longdouble step| = 1.83e-16 (7.6e-17 ..
1.83e-16 per case); |device - longdouble| = 1.83e-16 (6.5e-17 .. 1.83e-16), against a bar of 1.8e-15 per entry of magnitude 1."""
import numpy as np
import pytest

import odometry_cases as oc
import odometry_restatement as orr
from odometry_cases import same_bits, scaled_cam, scene
from test_odometry_gpu import device_odometry, restatement
from elasticreconstruction_amd import synth

pytestmark = pytest.mark.gpu
_cache = {}
IDS = ["%dx%d" % (c, r) for c, r, _ in oc.SHAPES]


def both(cols, rows, **params):
    cam = scaled_cam(cols)
    return device_odometry(cols, rows, cam, **params), restatement(cols, rows, cam, **params)


def rest_maps(cols, rows, frame_key, frame, **params):
    """The restatement's maps of a frame, computed once per process."""
    key = (cols, rows, frame_key, tuple(sorted(params.items())))
    if key not in _cache:
        _cache[key] = restatement(cols, rows, scaled_cam(cols), **params).maps(frame)
    return _cache[key]


def scene_maps(cols, rows, i, **params):
    return rest_maps(cols, rows, ("scene", i), scene(cols, rows)[0][i], **params)


def n_depth_w():
    from elasticreconstruction_amd import odometry
    return len(odometry.tables()[1])


def assert_maps_equal(cols, rows, frame, what, device_frame=None, **params):
    dev, ref = both(cols, rows, **params)
    want = ref.maps(frame)
    for level in range(ref.levels):
        dd, V, N = dev.maps(frame if device_frame is None else device_frame, level)
        wd, wV, wN = want[level]
        assert np.array_equal(dd, wd), (what, params, level)
        assert same_bits(V, wV) and same_bits(N, wN), (what, params, level)
    return want


def assert_linearization(dev, ref, frames, maps, level, T, what):
    """Count exact; every sum within count * 2^-53 * sum |terms|, the bound of two summation orders of exact products.  Returns the worst
    |difference| / bound."""
    sums, count = dev.linearize(frames[0], frames[1], level, T)
    want, wcount, wabs = ref.linearize(maps[0], maps[1], level, T, with_abs=True)
    assert count == wcount, (what, level, count, wcount)
    if wcount == 0:
        assert np.array_equal(sums, np.zeros(27)) and not np.signbit(sums).any(), (what, level)
        return 0.0
    bound = wcount * 2.0 ** -53 * wabs
    assert np.all(np.abs(sums - want) <= bound), (what, level, np.max(np.abs(sums - want) / bound))
    return float(np.max(np.abs(sums - want) / np.maximum(bound, 1e-300)))


def assert_steps(ref, maps, trace, n, guess=None):
    """Rows 0 .. n - 1 of a pair's trace: the count of every iteration equals the restatement's at the DEVICE's state, and the pose is
    within 1e-6 of one restatement step from that state.  Returns the state after row n - 1."""
    state = np.eye(4) if guess is None else np.asarray(guess, np.float64)
    for k, level in enumerate(ref.schedule()[:n]):
        s, count = ref.linearize(maps[0], maps[1], level, state)
        assert count == int(trace[k, 16]), (k, level, count, trace[k, 16])
        step, lost = ref.step(s, count, state)
        assert not lost and np.abs(step - trace[k, :16].reshape(4, 4)).max() <= 1e-6, (k, level)
        state = trace[k, :16].reshape(4, 4)
    return state


# ---- maps, bit for bit --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,rows,params", [(72, 52, {}), (41, 25, dict(levels=1))], ids=["72x52", "41x25"])
def test_maps_of_noisy_table_end_and_extreme_images_equal_the_restatement(gpu, cols, rows, params):
    import torch
    images = [("seeded %d" % s, oc.seeded_image(cols, rows, s)) for s in (1, 2, 3)]
    images += [("table end", oc.table_end_image(cols, rows, n_depth_w())), ("extreme", oc.extreme_image(cols, rows, 11))]
    for what, img in images:
        want = assert_maps_equal(cols, rows, img, what, **params)
        assert (want[0][0] > 0).sum() > cols * rows // 2 and np.isfinite(want[0][2]).any()
    ext = images[-1][1]
    assert (ext.astype(np.int16) < 0).any()
    assert_maps_equal(cols, rows, ext, "extreme, device int16", device_frame=torch.from_numpy(ext.astype(np.int16)).to(gpu), **params)


@pytest.mark.parametrize("cols,rows", [(5, 3), (1, 1)])
def test_maps_of_images_narrower_than_the_filter_window_equal_the_restatement(gpu, cols, rows):
    d = scene(cols, rows)[0]
    ramp = (1000 + 7 * np.arange(cols * rows)).reshape(rows, cols).astype(np.uint16)
    holed = ramp.copy()
    holed[rows // 2, cols // 2] = 0
    for what, img in (("render", d[0]), ("ramp", ramp), ("holed", holed), ("far", np.full((rows, cols), 65535, np.uint16))):
        want = assert_maps_equal(cols, rows, img, what, levels=1)
        assert np.isnan(want[0][2][-1]).all() and np.isnan(want[0][2][:, -1]).all()
    if cols > 1:
        assert np.isfinite(assert_maps_equal(cols, rows, ramp, "ramp", levels=1)[0][2][0, 0]).all()


def test_maps_of_four_levels_equal_the_restatement(gpu):
    cols, rows = 96, 64
    for what, img in (("seeded", oc.seeded_image(cols, rows, 4)), ("extreme", oc.extreme_image(cols, rows, 5)), ("render", scene(cols, rows)[0][0])):
        want = assert_maps_equal(cols, rows, img, what, levels=4)
        assert len(want) == 4 and want[3][0].shape == (8, 12) and np.isfinite(want[3][2]).any()


def test_depth_limit_cuts_between_two_values_that_are_present(gpu):
    cols, rows = 72, 52
    for what, img in (("seeded", oc.seeded_image(cols, rows, 6)), ("extreme", oc.extreme_image(cols, rows, 11))):
        # unfiltered: the limit is a value of the image itself (kept), the next larger one is cut
        vals = np.unique(img[img > 0])
        keep, cut = int(vals[len(vals) // 2]), int(vals[len(vals) // 2 + 1])
        want = assert_maps_equal(cols, rows, img, what, bilateral=0, max_depth_mm=keep)
        assert want[0][0].max() == keep and (img == cut).any() and not (want[0][0] == cut).any()
        # filtered: the same, with two values that are present AFTER the filter
        filtered = rest_maps(cols, rows, (what, "filtered"), img)[0][0]
        vals = np.unique(filtered[filtered > 0])
        keep, cut = int(vals[len(vals) // 2]), int(vals[len(vals) // 2 + 1])
        want = assert_maps_equal(cols, rows, img, what, max_depth_mm=keep)
        assert want[0][0].max() == keep and (filtered == cut).any() and not (want[0][0] == cut).any()
        assert np.array_equal(want[0][0], np.where(filtered > keep, 0, filtered))


# ---- one linearisation at every size of the table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,rows,params", oc.SHAPES, ids=IDS)
def test_linearize_at_every_shape_and_level(gpu, cols, rows, params):
    d, W, cam = scene(cols, rows)
    dev, ref = both(cols, rows, **params)
    maps = [scene_maps(cols, rows, i, **params) for i in (0, 1)]
    G = np.linalg.inv(W[0]) @ W[1]
    worst, counts = 0.0, []
    for what, T in (("identity", np.eye(4)), ("ground truth", G)):
        for level in range(ref.levels):
            worst = max(worst, assert_linearization(dev, ref, d[:2], maps, level, T, what))
            counts.append(ref.linearize(maps[0], maps[1], level, T)[1])
    print("%d x %d levels %d: counts %s, worst |difference| / bound %.3g" % (cols, rows, ref.levels, counts, worst))
    if cols >= 16:
        assert min(counts) > 0
    elif cols == 1:
        assert counts == [0, 0]                                # no normal in a 1 x 1 image: the sums must be exactly 0.0 (asserted above)
    else:
        assert 0 < max(counts) <= 8


@pytest.mark.parametrize("cols,rows,params", [(72, 52, {}), (129, 64, dict(levels=1))], ids=["72x52", "129x64"])
def test_linearize_at_poses_that_push_pixels_through_every_border_of_the_match(gpu, cols, rows, params):
    d, W, cam = scene(cols, rows)
    dev, ref = both(cols, rows, **params)
    maps = [scene_maps(cols, rows, i, **params) for i in (0, 1)]
    worst = 0.0
    for what, (T, border) in oc.border_poses().items():
        for level in range(ref.levels):
            worst = max(worst, assert_linearization(dev, ref, d[:2], maps, level, T, what))
        if what in ("nan", "inf"):                           # count 0 on every level (asserted against the restatement); the pair is lost at once
            assert ref.linearize(maps[0], maps[1], 0, T)[1] == 0
            Tout, status, trace = dev.align_pairs(d, [0], [1], guess=T[None], trace=True)
            assert status[0] == 1 and np.array_equal(Tout[0].view(np.uint64), T.view(np.uint64))
            assert not trace[0, :, 16].any() and all(np.array_equal(row[:16].view(np.uint64), T.reshape(16).view(np.uint64)) for row in trace[0])
    print("%d x %d border poses: worst |difference| / bound %.3g" % (cols, rows, worst))


def test_linearize_with_other_thresholds(gpu):
    cols, rows = 72, 52
    d, W, cam = scene(cols, rows)
    T = np.linalg.inv(W[0]) @ W[1] @ synth.perturbation(7, 3.0, 0.03)
    base = [restatement(cols, rows, cam).linearize(scene_maps(cols, rows, 0), scene_maps(cols, rows, 1), level, T)[1] for level in range(3)]
    changed = 0
    for params in (dict(dist_thresh=1e-3), dict(dist_thresh=0.02), dict(dist_thresh=10.0), dict(angle_thresh=0.01), dict(angle_thresh=2.0)):
        dev, ref = both(cols, rows, **params)
        maps = [scene_maps(cols, rows, i) for i in (0, 1)]                      # the maps do not depend on the thresholds
        counts = []
        for level in range(3):
            assert_linearization(dev, ref, d[:2], maps, level, T, params)
            counts.append(ref.linearize(maps[0], maps[1], level, T)[1])
        print(params, counts, "default", base)
        changed += counts != base
    assert changed >= 2


# ---- schedules ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [(0, 5, 4), (3, 0, 0)])
def test_a_level_with_no_iterations_is_skipped(gpu, iterations):
    cols, rows = 72, 52
    d, W, cam = scene(cols, rows)
    dev, ref = both(cols, rows, iterations=iterations)
    maps = [scene_maps(cols, rows, i) for i in (0, 1)]
    T, status, trace = dev.align_pairs(d, [0], [1], trace=True)
    n = sum(iterations)
    assert status[0] == 0 and trace.shape == (1, n, 17) and ref.schedule() == [2] * iterations[2] + [1] * iterations[1] + [0] * iterations[0]
    state = assert_steps(ref, maps, trace[0], n)
    assert np.array_equal(T[0], state) and not np.array_equal(state, np.eye(4))


def test_a_schedule_of_no_iterations_returns_the_guess(gpu):
    cols, rows = 72, 52
    d, W, cam = scene(cols, rows)
    dev, ref = both(cols, rows, iterations=(0, 0, 0))
    guess = np.linalg.inv(W[0]) @ W[1] @ synth.perturbation(5, 1.0, 0.01)
    for g in (None, guess[None]):
        T, status, trace, sums = dev.align_pairs(d, [0], [1], guess=g, trace=True, sums=True)
        assert status[0] == 0 and trace.shape == (1, 0, 17) and not sums.any()
        assert np.array_equal(T[0].view(np.uint64), (np.eye(4) if g is None else guess).view(np.uint64))
    T, status = dev.align_pairs(d, [0, 1, 2], [1, 2, 3], window=2)
    assert not status.any() and all(np.array_equal(t, np.eye(4)) for t in T)
    assert ref.schedule() == []


@pytest.mark.parametrize("cols,rows,params", oc.ALIGNABLE, ids=IDS[:len(oc.ALIGNABLE)])
def test_every_traced_iteration_at_every_shape_is_one_restatement_step_from_the_device_state(gpu, cols, rows, params):
    d, W, cam = scene(cols, rows)
    dev, ref = both(cols, rows, **params)
    maps = [scene_maps(cols, rows, i, **params) for i in (0, 1)]
    T, status, trace, sums = dev.align_pairs(d, [0], [1], trace=True, sums=True)
    n = len(ref.schedule())
    assert status[0] == 0 and trace.shape == (1, n, 17) and n == sum((10, 5, 4, 4)[:ref.levels])
    state = assert_steps(ref, maps, trace[0], n)
    assert np.array_equal(T[0], state)
    before = trace[0, -2, :16].reshape(4, 4) if n > 1 else np.eye(4)
    s, count, sabs = ref.linearize(maps[0], maps[1], 0, before, with_abs=True)                      # `sums`: the last iteration's
    assert np.all(np.abs(sums[0] - s) <= count * 2.0 ** -53 * sabs)


def test_an_empty_pair_with_min_valid_zero_is_lost_not_nan(gpu):
    cols, rows = 72, 52
    d, W, cam = scene(cols, rows)
    dev, ref = both(cols, rows, min_valid=0)
    depth = np.stack([d[0], np.zeros_like(d[0])])
    T, status, trace = dev.align_pairs(depth, [0, 1, 1], [1, 0, 1], trace=True)
    assert list(status) == [1, 1, 1] and np.isfinite(T).all() and np.isfinite(trace).all()
    assert all(np.array_equal(t, np.eye(4)) for t in T) and not trace[:, :, 16].any()
    assert ref.step(np.zeros(27), 0, np.eye(4))[1]                                                # the restatement: a zero matrix has no Cholesky factor


# ---- a pair that is lost part-way -----------------------------------------------------------------------------------------------------------------
def test_a_pair_lost_part_way_keeps_its_last_good_pose_alone_and_in_any_list(gpu):
    cols, rows = 72, 52
    d, W, cam = scene(cols, rows)
    dev, ref = both(cols, rows)
    depth = np.concatenate([d, oc.comb(d[1])[None], np.zeros((1, rows, cols), np.uint16)])       # frame 4: the comb; frame 5: all zero
    maps = {i: scene_maps(cols, rows, i) for i in range(4)}
    maps[4] = rest_maps(cols, rows, "comb 1", depth[4])
    guess = np.linalg.inv(W[1]) @ W[2] @ synth.perturbation(5, 1.0, 0.01)
    #        comb   healthy  comb    healthy  zero    healthy  comb    zero
    pairs = [(0, 4), (0, 1), (4, 0), (1, 2), (0, 5), (2, 3), (4, 4), (5, 1)]
    guesses = np.stack([np.eye(4)] * 3 + [guess] + [np.eye(4)] * 4)
    mi, fi = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    single = [dev.align_pairs(depth, [a], [b], guess=guesses[k:k + 1], trace=True, sums=True) for k, (a, b) in enumerate(pairs)]
    sT, sS, sTr, sSu = (np.concatenate([s[q] for s in single]) for q in range(4))
    assert list(sS) == [1, 0, 1, 0, 1, 0, 1, 1] and np.isfinite(sT).all() and np.isfinite(sTr).all()
    for k in (0, 2):                                          # the comb in either role: four good iterations on level 2, then no match on level 1
        a, b = pairs[k]
        assert sTr.shape[1] == 19 and [int(c) for c in sTr[k, :, 16]] == [176] * 4 + [0] * 15
        state = assert_steps(ref, (maps[a], maps[b]), sTr[k], 4)
        assert np.array_equal(sT[k].view(np.uint64), sTr[k, 3, :16].reshape(4, 4).view(np.uint64)) and np.array_equal(sT[k], state)
        assert all(np.array_equal(row[:16].view(np.uint64), sTr[k, 3, :16].view(np.uint64)) for row in sTr[k, 4:])
        assert 0.02 <= np.abs(sT[k] - np.eye(4)).max() <= 0.03
        want = ref.linearize(maps[a], maps[b], 1, state)
        assert want[1] == 0 and not sSu[k].any()                                   # `sums`: those of the iteration that lost the pair
    assert_steps(ref, (maps[0], maps[1]), sTr[1], 19)
    assert_steps(ref, (maps[1], maps[2]), sTr[3], 19, guess)
    order = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    for window in (2, 3, 5, 0):
        for perm in (np.arange(8), order):
            for run in range(2):
                T, S, Tr, Su = dev.align_pairs(depth, mi[perm], fi[perm], guess=guesses[perm], window=window, trace=True, sums=True)
                what = (window, list(perm), run)
                assert np.array_equal(S, sS[perm]), what
                assert np.array_equal(T.view(np.uint64), sT[perm].view(np.uint64)), what
                assert np.array_equal(Tr.view(np.uint64), sTr[perm].view(np.uint64)), what
                assert np.array_equal(Su.view(np.uint64), sSu[perm].view(np.uint64)), what


# ---- the solve and the pose update alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,rows", [(32, 32), (129, 64), (160, 120)])
def test_one_step_from_the_devices_own_sums_against_a_longdouble_restatement(gpu, cols, rows):
    """levels = 1, one iteration: the returned sums are that iteration's, so T is one step from them and the reduction's error is out of the
    comparison.  e = the worst entry difference between the restatement's float64 step (numpy.linalg) and the longdouble one; the device may
    be 8 e off the longdouble step, or 16 ulp of the entry (of 1 for entries below 1) where e is smaller than that."""
    d, W, cam = scene(cols, rows)
    dev, ref = both(cols, rows, levels=1, iterations=(1,))
    G = np.linalg.inv(W[0]) @ W[1]
    for what, guess in (("identity", np.eye(4)), ("perturbed", G @ synth.perturbation(7, 1.0, 0.01))):
        T, status, trace, sums = dev.align_pairs(d, [0], [1], guess=guess[None], trace=True, sums=True)
        assert status[0] == 0 and trace.shape == (1, 1, 17) and np.array_equal(T[0], trace[0, 0, :16].reshape(4, 4))
        count = int(trace[0, 0, 16])
        want = oc.step_longdouble(sums[0], guess)
        f64, lost = ref.step(sums[0], count, guess)
        assert not lost and count >= 50
        e = float(np.abs(f64.astype(np.longdouble) - want).max())
        err = np.abs(T[0].astype(np.longdouble) - want).astype(np.float64)
        bar = np.maximum(8.0 * e, 16.0 * 2.0 ** -53 * np.maximum(1.0, np.abs(want.astype(np.float64))))
        print("%d x %d %s: count %d, e = %.3g, |device - longdouble| = %.3g" % (cols, rows, what, count, e, err.max()))
        assert np.all(err <= bar), (what, err.max(), e)
        assert np.abs(T[0] - guess).max() > 1e-4                                  # a real step, not the guess handed back
