"""Seeded synthetic pose graphs for the GraphOptimizer tests.

    truth      a random walk from the identity, up to 0.5 rad and 0.4 m per step
    odometry   the truth's steps perturbed by up to 0.002 rad / 0.002 m
    true loops all (i, i + 1) and `density` of the other pairs, perturbed by up to 0.0015 rad / 0.001 m
    false loops a quarter as many as the true ones, on pairs drawn from the rest, off by up to 1 rad / 0.5 m (at least 0.3 of either)
    information sum A^T A, A = [I | -2 [p]x] (BuildCorrespondence/CorresApp.cpp:192-204), over 400 points of a 0.5 .. 2.5 m box, scaled to
               300 .. 2000 correspondences
"""
import numpy as np


def rigid(rng, max_rot, max_trans, least=0.0):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = max_rot * rng.uniform(least, 1.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    t = rng.normal(size=3)
    T[:3, 3] = t / np.linalg.norm(t) * max_trans * rng.uniform(least, 1.0)
    return T


def information(rng):
    p = rng.uniform(0.5, 2.5, size=(400, 3))
    ATA = np.zeros((6, 6))
    for x, y, z in p:
        A = np.array([[1, 0, 0, 0, 2 * z, -2 * y], [0, 1, 0, -2 * z, 0, 2 * x], [0, 0, 1, 2 * y, -2 * x, 0]], np.float64)
        ATA += A.T @ A
    return ATA * (rng.uniform(300, 2000) / 400.0)


def make_case(N, seed=7, density=0.3, info=True, lonely=None, duplicate=False, reverse=False):
    """dict(truth [N, 4, 4], odo_T, odo_info | None, loop_ids [K, 2], loop_T, loop_info | None, is_true [K]).
    lonely: a vertex that no loop touches.  duplicate: the first true loop a second time, with its own noise.  reverse: every third loop is
    stored as (id2, id1) with the inverse transform."""
    rng = np.random.RandomState(seed)
    truth = [np.eye(4)]
    for _ in range(N - 1):
        truth.append(truth[-1] @ rigid(rng, 0.5, 0.4, 0.3))
    truth = np.stack(truth)
    rel = lambda i, j: np.linalg.inv(truth[i]) @ truth[j]
    odo_T = np.stack([rel(i, i + 1) @ rigid(rng, 0.002, 0.002) for i in range(N - 1)])
    pairs = [(i, j) for i in range(N) for j in range(i + 1, N)]
    true_pairs, rest = [], []
    for (i, j) in pairs:
        if lonely is not None and lonely in (i, j):
            continue
        if j == i + 1 or rng.uniform() < density:
            true_pairs.append((i, j))
        else:
            rest.append((i, j))
    if duplicate and true_pairs:
        true_pairs.append(true_pairs[0])
    n_false = min(len(rest), int(round(0.25 * len(true_pairs))))
    false_pairs = [rest[k] for k in sorted(rng.choice(len(rest), n_false, replace=False))] if n_false else []
    entries = [(i, j, rel(i, j) @ rigid(rng, 0.0015, 0.001), True) for (i, j) in true_pairs]
    entries += [(i, j, rel(i, j) @ rigid(rng, 1.0, 0.5, 0.3), False) for (i, j) in false_pairs]
    entries.sort(key=lambda t: (t[0], t[1]))                                 # the order of GlobalRegistration's result.txt
    ids, Ts, flags = [], [], []
    for k, (i, j, T, ok) in enumerate(entries):
        if reverse and k % 3 == 1:
            i, j, T = j, i, np.linalg.inv(T)
        ids.append((i, j))
        Ts.append(T)
        flags.append(ok)
    K = len(ids)
    return dict(N=N, truth=truth, odo_T=odo_T, odo_info=np.stack([information(rng) for _ in range(N - 1)]) if info else None,
                loop_ids=np.array(ids, np.int32).reshape(K, 2), loop_T=np.stack(Ts) if K else np.zeros((0, 4, 4)),
                loop_info=(np.stack([information(rng) for _ in range(K)]) if K else np.zeros((0, 6, 6))) if info else None,
                is_true=np.array(flags, bool))


def write_files(case, d, n_frames=None):
    """odometry.log / odometry.info / result.txt / result.info in directory d, as bin/GlobalRegistration writes them.  Returns the paths."""
    import os
    from elasticreconstruction_amd import formats
    N = case["N"]
    fr = N if n_frames is None else n_frames
    paths = {k: os.path.join(str(d), v) for k, v in dict(odometry="odometry.log", odometryinfo="odometry.info", loop="result.txt", loopinfo="result.info").items()}
    formats.save_log(paths["odometry"], [formats.FramedTransformation(i, i + 1, fr, T) for i, T in enumerate(case["odo_T"])])
    formats.save_log(paths["loop"], [formats.FramedTransformation(a, b, fr, T) for (a, b), T in zip(case["loop_ids"], case["loop_T"])])
    if case["odo_info"] is not None:
        formats.save_info(paths["odometryinfo"], [formats.FramedInformation(i, i + 1, fr, I) for i, I in enumerate(case["odo_info"])])
        formats.save_info(paths["loopinfo"], [formats.FramedInformation(a, b, fr, I) for (a, b), I in zip(case["loop_ids"], case["loop_info"])])
    return paths


# The fixtures of the tests, by name: make_case arguments.  N = 12 is dimension 66 (just past one 64-wide block of the factorisation), N = 33
# dimension 192, N = 65 dimension 384 with 316 loops (several panels, a trailing update of more than one workgroup).
# The seed is 1, not the 7 of the first prototype of the model: with this generator seed 7 leaves the N = 10 graph with a true loop whose EM weight
# ends at 0.265, inside the band (0.15, 0.35) that no fixture may touch (tests/test_posegraph_cpu.py); seed 1 clears it at N = 6 and N = 10
# (0.444 and 0.635).  N = 65 has a seed and density of its own for the same reason (seed 1 at density 0.1: 0.312; seeds 2, 3, 4, 11, 12 and 13 drop a true loop or end inside the band as well, seed 5 ends at 0.536).
SEED = 1
CASES = {
    "n2": dict(N=2, density=0.0, chain_only=True),
    "n3": dict(N=3, density=1.0, one_loop=True),
    "n6": dict(N=6),
    "n10": dict(N=10),
    "n12": dict(N=12),
    "n33": dict(N=33),
    "n65": dict(N=65, density=0.1, seed=5),
    "lonely": dict(N=8, lonely=4),
    "duplicate": dict(N=7, duplicate=True),
    "reverse": dict(N=9, reverse=True),
    "identity": dict(N=8, info=False),
}
_cases, _solved = {}, {}


def case(name):
    """the fixture `name` (made once)"""
    if name not in _cases:
        spec = dict(CASES[name])
        chain_only, one_loop = spec.pop("chain_only", False), spec.pop("one_loop", False)
        c = make_case(seed=spec.pop("seed", SEED), **spec)
        if chain_only or one_loop:                                           # N = 2 without a loop; N = 3 with the one loop (0, 2)
            keep = [k for k, (a, b) in enumerate(c["loop_ids"]) if one_loop and (a, b) == (0, 2)]
            c["loop_ids"], c["loop_T"], c["is_true"] = c["loop_ids"][keep], c["loop_T"][keep], c["is_true"][keep]
            c["loop_info"] = c["loop_info"][keep]
        _cases[name] = c
    return _cases[name]


def graph(name):
    import posegraph_restatement as pr
    c = case(name)
    return pr.Graph(c["odo_T"], c["loop_ids"], c["loop_T"], c["odo_info"], c["loop_info"])


EM_ROUNDS = 40      # the EM runs of the tests: its fixed point is reached after 20 .. 35 accepted rounds on these graphs


def solved(name, method):
    """the restatement's optimize() of the fixture (computed once per process, shared by the CPU and the GPU tests; never modified)"""
    if (name, method) not in _solved:
        _solved[(name, method)] = graph(name).optimize(method, 1.0, 100 if method == "switchable" else EM_ROUNDS)
    return _solved[(name, method)]
