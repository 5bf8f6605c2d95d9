"""er_ransac_align_batch (icp.ransac_align_batch): the pair loop of GlobalRegistration's do_all as one call.  The reference for every pair
of every list is ransac_align on that pair alone; equal means same_result of tests/test_ransac_shapes_gpu.py -- every bit of T, converged,
n_inliers, error and the stats -- and, for the information matrices, every bit of what ransac_inliers returns at the winning T.  No
tolerance anywhere.
Scene: rr.common_scene(3, points=600, noise=0.02, outlier_frac=0.0), the scene of tests/test_ransac_shapes_gpu.py with a third fragment,
grid cell 0.075, inlier_fraction 0.05, seed 1, 20 000 iterations, the other parameters alignment.config's (4 samples, k = 2, similarity
0.9) unless a test says otherwise.
What the numpy restatement and the CPU oracle's getFitness give for the six ordered pairs (source, target) of this scene, without a GPU
(rr.align, as tests/test_ransac_align_cpu.py runs it): all six converge --
    (0,1) 85 inliers of 45 scored, (0,2) 79 / 57, (1,0) 82 / 54, (1,2) 108 / 162, (2,0) 32 / 65, (2,1) 127 / 135
-- so the equality tests compare real poses; test_all_ordered_pairs_in_one_call asserts at least 3 of 6 about the single calls.
The two pairs built to end without a result (restatement, 20 000 iterations): a target with all-zero descriptors leaves 0 polygon
survivors for each of (1,0), (2,1), (0,2); a target with negated normals leaves 66 / 163 / 73 survivors and 0 accepted."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ransac_restatement as rr
from elasticreconstruction_amd import _ffi
from elasticreconstruction_amd.icp import Cloud, Features, global_registration, ransac_align, ransac_align_batch, ransac_inliers
from test_ransac_shapes_gpu import same_result

pytestmark = pytest.mark.gpu
FMAX = float(np.finfo(np.float32).max)
CELL = 0.075
KW = dict(max_iterations=20000, seed=1, inlier_fraction=0.05)
ORDERED = list(itertools.permutations(range(3), 2))
_cache = {}


def scene():
    """(restatement scene, clouds, features) of the three fragments."""
    if "sc" not in _cache:
        sc = rr.common_scene(3, points=600, noise=0.02, outlier_frac=0.0)
        _cache["sc"] = (sc, [Cloud(x, n, CELL) for x, n, _, _ in sc], [Features(f) for _, _, _, f in sc])
    return _cache["sc"]


def single(s, t, **kw):
    """ransac_align of fragment s onto fragment t, once per parameter set."""
    key = (s, t, tuple(sorted(kw.items())))
    if key not in _cache:
        _, cl, ft = scene()
        _cache[key] = ransac_align(cl[s], cl[t], ft[s], ft[t], **dict(KW, **kw))
    return _cache[key]


def batch(pairs, **kw):
    _, cl, ft = scene()
    return ransac_align_batch([cl[s] for s, _ in pairs], [cl[t] for _, t in pairs], [ft[s] for s, _ in pairs], [ft[t] for _, t in pairs],
                              **dict(KW, **kw))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def check_info(r, src, tgt):
    if r.converged:
        _, _, _, info_s, info_t = ransac_inliers(src, tgt, r.T, CELL)
        assert info_s.any() and info_t.any()
        assert same_bits(r.info_source, info_s) and same_bits(r.info_target, info_t)
    else:
        assert not r.info_source.any() and not r.info_target.any()


def test_all_ordered_pairs_in_one_call(gpu):
    _, cl, ft = scene()
    ref = [single(s, t) for s, t in ORDERED]
    print("single calls:", [(p, r.converged, r.n_inliers, r.stats["scored"]) for p, r in zip(ORDERED, ref)])
    assert sum(r.converged for r in ref) >= 3, "the scene must give poses to compare, not identities"
    out = batch(ORDERED)
    assert len(out) == 6 and all(r.info_source is None and r.info_target is None and r.aux is None for r in out)
    for p, a, b in zip(ORDERED, ref, out):
        assert same_result(a, b), p
    out = batch(ORDERED, want_info=True)
    for (s, t), a, b in zip(ORDERED, ref, out):
        assert same_result(a, b), (s, t)
        check_info(b, cl[s], cl[t])


def test_pairs_of_different_sizes(gpu):
    """Sources of 257, 255 and exactly nr_samples points next to one of 600: every grid of the wave is sized for the 600, so workgroups
    of the small pairs find no point of theirs (k_ransac_score leaves them before its first barrier).  Every target is a full fragment,
    the largest cloud of the list."""
    sc, cl, ft = scene()
    cut = {}
    for frag, m in ((1, 257), (2, 255), (1, 4)):
        x, n, _, f = sc[frag]
        cut[(frag, m)] = (Cloud(x[:m], n[:m], CELL), Features(f[:m]))
    lst = [(cut[(1, 257)], 0), (cut[(2, 255)], 0), (cut[(1, 4)], 2), ((cl[0], ft[0]), 1), (cut[(2, 255)], 1)]
    kw = dict(KW, inlier_fraction=0.02)
    ref = [ransac_align(c, cl[t], f, ft[t], **kw) for (c, f), t in lst]
    print("sizes:", [(len(c), r.converged, r.n_inliers, r.stats["scored"]) for ((c, _), _), r in zip(lst, ref)])
    assert sum(r.stats["scored"] > 0 for r in ref) >= 3 and sum(r.converged for r in ref) >= 2
    for order in (range(5), (4, 2, 3, 0, 1)):                                               # the 600 in the middle of the wave and at its end
        sub = [lst[i] for i in order]
        out = ransac_align_batch([c for (c, _), _ in sub], [cl[t] for _, t in sub], [f for (_, f), _ in sub], [ft[t] for _, t in sub],
                                 want_info=True, **kw)
        for i, b in zip(order, out):
            assert same_result(ref[i], b), i
            check_info(b, lst[i][0][0], cl[lst[i][1]])


def test_pairs_without_a_survivor_between_pairs_that_converge(gpu):
    """Two pairs that end with nothing, each between pairs that converge.  The first has no polygon survivor in any chunk: its target,
    fragment 0 moved 50 m away, carries all-zero descriptors, so every source point is matched to target points 0 and 1 and every
    polygon of four has an edge of length zero.  (The search is invariant under a translation of the target and `similarity` belongs to
    the whole list, so neither the 50 m nor a similarity of 0.9999 can single out one pair.)  The second has survivors and none accepted:
    its target is fragment 1 with its normals negated, every hypothesis fails the normal test.  n_surv == 0 and n_acc == 0 are what the
    one-workgroup kernels and the scoring grid of such a pair see while their neighbours work."""
    sc, cl, ft = scene()
    x0, n0, _, f0 = sc[0]
    x1, n1, _, f1 = sc[1]
    far, far_f = Cloud(x0 + np.float32(50.0), n0, CELL), Features(np.zeros_like(f0))
    flip = Cloud(x1, -n1, CELL)
    lst = [(cl[2], cl[1], ft[2], ft[1]), (cl[1], far, ft[1], far_f), (cl[0], cl[2], ft[0], ft[2]), (cl[2], flip, ft[2], ft[1]),
           (cl[1], cl[0], ft[1], ft[0])]
    ref = [ransac_align(s, t, fs, ftg, **KW) for s, t, fs, ftg in lst]
    assert ref[0].converged and ref[2].converged and ref[4].converged
    assert ref[1].stats["polygon_rejections"] == 20000 and ref[1].stats["scored"] == 0
    assert ref[3].stats["normal_rejections"] > 0 and ref[3].stats["scored"] == 0
    for chunk in (0, 4096):
        out = ransac_align_batch([p[0] for p in lst], [p[1] for p in lst], [p[2] for p in lst], [p[3] for p in lst], want_info=True,
                                 chunk_iterations=chunk, **KW)
        for i, (a, b) in enumerate(zip(ref, out)):
            assert same_result(a, b), (chunk, i)
            check_info(b, lst[i][0], lst[i][1])
        for dead in (out[1], out[3]):
            assert not dead.converged and np.array_equal(dead.T, np.eye(4, dtype=np.float32)) and dead.error == FMAX and dead.n_inliers == 0
            assert not dead.info_source.any() and not dead.info_target.any()


def test_max_concurrent_and_the_make_up_of_the_list_are_not_part_of_the_result(gpu):
    pairs = ORDERED[:5]
    ref = [single(s, t) for s, t in pairs]
    for mc in (1, 2, 5, 0):
        for a, b in zip(ref, batch(pairs, max_concurrent=mc)):
            assert same_result(a, b), mc
    one = batch([ORDERED[3]])
    assert len(one) == 1 and same_result(single(*ORDERED[3]), one[0])
    three = batch([ORDERED[3]] * 3, want_info=True)
    assert all(same_result(single(*ORDERED[3]), r) for r in three)
    assert all(same_bits(r.info_source, three[0].info_source) and same_bits(r.info_target, three[0].info_target) for r in three)
    assert batch([]) == []


def test_chunk_edges_under_batching(gpu):
    """20 001 iterations in chunks of 4096: the last chunk is one iteration.  Chunks of one iteration: one lane, one mask word, mostly
    nothing to list.  chunk_iterations is not part of the single call's result either, so the reference is the default chunk's."""
    pairs = [(1, 0), (2, 1), (0, 2)]
    for iters, chunk in ((20001, 4096), (300, 1)):
        ref = [single(s, t, max_iterations=iters) for s, t in pairs]
        for mc in (0, 2):
            for a, b in zip(ref, batch(pairs, max_iterations=iters, chunk_iterations=chunk, max_concurrent=mc)):
                assert same_result(a, b), (iters, chunk, mc)
    assert sum(single(s, t, max_iterations=20001).converged for s, t in pairs) >= 2


@pytest.mark.parametrize("ns,k,sim,iters", ((3, 1, 0.9, 20000), (6, 1, 0.9, 20000), (3, 8, 0.7, 20000), (6, 8, 0.3, 200000)))
def test_every_instantiation_through_the_pair_axis(gpu, ns, k, sim, iters):
    """Similarity and length per (nr_samples, k) as in COMBOS of tests/test_ransac_shapes_gpu.py, whose restatement counts 988, 35, 79
    and 13 accepted hypotheses for the pair (1, 0)."""
    pairs = [(1, 0), (0, 2)]
    kw = dict(nr_samples=ns, k_correspondences=k, similarity=sim, max_iterations=iters)
    ref = [single(s, t, **kw) for s, t in pairs]
    assert ref[0].stats["scored"] >= 5
    for a, b in zip(ref, batch(pairs, **kw)):
        assert same_result(a, b)


def test_per_pair_seeds(gpu):
    pairs, seeds = [(1, 0), (2, 1), (1, 0)], [0, 1, 0xffffffff]
    ref = [single(s, t, seed=sd) for (s, t), sd in zip(pairs, seeds)]
    assert not same_result(ref[0], ref[2])                                                  # the seed is seen
    out = batch(pairs, seeds=seeds, seed=77)                                                # (p->seed is not used once there are seeds)
    for a, b in zip(ref, out):
        assert same_result(a, b)


def test_two_runs_give_the_same_bits(gpu):
    a, b = batch(ORDERED, want_info=True), batch(ORDERED, want_info=True)
    for x, y in zip(a, b):
        assert same_result(x, y) and same_bits(x.info_source, y.info_source) and same_bits(x.info_target, y.info_target)


def _raw(n, src, tgt, sf, tf, max_concurrent=0, **kw):
    """er_ransac_align_batch through the C ABI with arrays that may be NULL: (return code, message)."""
    L = _ffi.lib()
    d = dict(dict(max_iterations=20000, nr_samples=4, k_correspondences=2, similarity=0.9, max_corr_dist=0.075, inlier_fraction=0.05, inlier_number=30000,
                  angle_diff=0.52359878, seed=1, chunk_iterations=0), **kw)
    p = _ffi.ErRansacParams(d["max_iterations"], d["nr_samples"], d["k_correspondences"], d["similarity"], d["max_corr_dist"], d["inlier_fraction"],
                            d["inlier_number"], d["angle_diff"], d["seed"], d["chunk_iterations"])
    arr = lambda v: None if v is None else (C.c_void_p * len(v))(*[c._h for c in v])
    m = max(n, 1)
    T, conv = np.full((m, 16), 7, np.float32), np.full(m, 7, np.int32)
    rc = L.er_ransac_align_batch(n, arr(src), arr(tgt), arr(sf), arr(tf), C.byref(p), None, max_concurrent, _ffi.ptr(T), _ffi.ptr(conv), None, None,
                                 None, None, None)
    return rc, L.er_last_error().decode(), T, conv


def test_refusals_name_the_pair_and_leave_the_handles_usable(gpu):
    sc, cl, ft = scene()
    pairs = [(1, 0), (2, 1), (0, 2)]
    ref = [single(s, t) for s, t in pairs]

    def still_fine():
        for a, b in zip(ref, batch(pairs)):
            assert same_result(a, b)

    def refused(match, **kw):
        with pytest.raises(_ffi.ErError, match=match):
            batch(pairs, **kw)
        still_fine()

    refused(r"pair 0: nr_samples = 2 is refused", nr_samples=2)
    refused(r"pair 0: .*cell", max_corr_dist=0.2)                                           # a radius the targets' grids (cell 0.075) cannot serve
    refused(r"max_concurrent = -1", max_concurrent=-1)
    short = Features(sc[1][3][:599])                                                        # 599 descriptors for 600 points
    S, Tg = [cl[1], cl[2], cl[0]], [cl[0], cl[1], cl[2]]
    with pytest.raises(_ffi.ErError, match=r"pair 1: the target points and target feature points .* 600 vs 599"):
        ransac_align_batch(S, Tg, [ft[1], ft[2], ft[0]], [ft[0], short, ft[2]], **KW)
    still_fine()
    with pytest.raises(_ffi.ErError, match=r"pair 2: the source points and source feature points .* 600 vs 599"):
        ransac_align_batch(S, Tg, [ft[1], ft[2], short], [ft[0], ft[1], ft[2]], **KW)
    still_fine()
    big = Cloud(sc[0][0], sc[0][1], 0.05)                                                   # one target of the list with a finer grid than the radius
    with pytest.raises(_ffi.ErError, match=r"pair 2: "):
        ransac_align_batch(S, [cl[0], cl[1], big], [ft[1], ft[2], ft[0]], [ft[0], ft[1], ft[0]], **KW)
    still_fine()
    if _ffi.lib().er_device_count() > 1:                                                    # clouds and features on different devices
        other = Features(sc[2][3], device=1)
        with pytest.raises(_ffi.ErError, match=r"pair 1: .*different devices"):
            ransac_align_batch(S, Tg, [ft[1], other, ft[0]], [ft[0], ft[1], ft[2]], **KW)
        still_fine()
    for args in ((3, None, Tg, S, Tg), (3, S, None, S, Tg), (3, S, Tg, None, Tg), (3, S, Tg, S, None)):
        rc, msg, T, conv = _raw(*args)
        assert rc != 0 and "NULL array" in msg and (T == 7).all() and (conv == 7).all()
    rc, msg, T, conv = _raw(-1, S, Tg, S, Tg)
    assert rc != 0 and "n_pairs = -1" in msg
    rc, msg, T, conv = _raw(0, None, None, None, None, max_concurrent=-5)                   # nothing to do: nothing is looked at
    assert rc == 0 and (T == 7).all() and (conv == 7).all()
    still_fine()


def test_global_registration_batch_equals_the_loop(gpu):
    """The three fragments as they are (equal sizes: no pair is turned round), without smart_swap, and with a middle fragment of 400 points,
    which smart_swap makes the source of both its pairs: the entries then carry the inverse and information_target_."""
    sc, cl, ft = scene()
    x, n, _, f = sc[1]
    sub, subf = [cl[0], Cloud(x[:400], n[:400], CELL), cl[2]], [ft[0], Features(f[:400]), ft[2]]
    for clouds, feats, swap, frac, least in ((cl, ft, True, 0.05, 2), (cl, ft, False, 0.05, 2), (sub, subf, True, 0.02, 1)):
        kw = dict(KW, inlier_fraction=frac)
        a = global_registration(clouds, feats, smart_swap=swap, **kw)
        b = global_registration(clouds, feats, smart_swap=swap, batch=True, **kw)
        assert len(a[0]) == len(a[1]) == len(b[0]) == len(b[1]) >= least
        for ta, ia, tb, ib in zip(a[0], a[1], b[0], b[1]):
            assert (ta.id1, ta.id2, ta.frame) == (tb.id1, tb.id2, tb.frame) == (ia.id1, ia.id2, ia.frame) == (ib.id1, ib.id2, ib.frame)
            assert same_bits(ta.T, tb.T) and same_bits(ia.info, ib.info) and ia.info.any()
