"""Crafted inputs that walk k_integrate (csrc/er_tsdf_int.hip) through every path of its frame loop, in both instantiations.

One fixed camera pose and per-frame CONSTANT depth images: with the camera at (1.7, 1.7, 0.2) looking along +z, a 96 x 64 image and fx = fy = 260,
a frame of constant depth d mm is a fronto-parallel surface at z = 0.2 + d / 1000, and every d in 930 .. 1290 touches the same three units (the
image is wider than one unit at that distance).  Inside a unit the wave boxes in front of the surface by more than the truncation are FULL for that
frame, the boxes around it are PROJECTED (band) and the boxes behind it are CULLED -- so a list of depths is a script of the verdicts each box
sees, frame by frame.  A zero pixel in a 16-pixel tile turns "full" into "free, but not provably so from the tile minima": the sure path.

Each fixture is a dict: name, cols, rows, cam (fx, fy, cx, cy, icp_trunc, integration_trunc), poses float64[n, 4, 4], depth uint16[n, rows * cols],
calls (the (start, stop) frame ranges the stream is handed over in; the library cuts a call at 64 frames itself), preset (None, or
{unit key: (sdf, weight)} the volume holds before the first frame), masks (per library batch of <= 64 frames: {unit key: frame mask}, what
k_prepare must hand to k_integrate) and events (the path events of tests/hostcheck's tally the fixture exists for).
tests/test_integrate_cases_cpu.py proves on the CPU twin that every fixture reaches its events -- also with the device's one-ulp reciprocal in
the box verdicts -- and tests/test_integrate_paths_gpu.py holds the kernel to the oracle on them, bit for bit.  Nothing here is random."""
import numpy as np

COLS, ROWS = 96, 64
TRUNC_BELOW_64 = float(np.nextafter(np.float32(64.0), np.float32(0.0)))

# unit keys ((xi * 512 + yi) * 512 + zi): the three x-neighbours the standard pose sees at 1.13 .. 1.49 m
def key(xi, yi, zi):
    return (xi * 512 + yi) * 512 + zi


K_LEFT, K_MID, K_RIGHT = key(259, 260, 259), key(260, 260, 259), key(261, 260, 259)
RUNS = [1250, 1250, 1000, 1250, 950, 1250, 1290, 1100, 1250, 960, 1250, 1250]
BEYOND = 65535                                             # a depth whose scaled value exceeds every integration_trunc used here but 100


def camera(trunc=2.5, f=260.0, cols=COLS, rows=ROWS):
    return np.array([f, f, (cols - 1) / 2.0, (rows - 1) / 2.0, 2.5, trunc], np.float32)


def pose(tx, ty, tz, yaw=0.0):
    T = np.eye(4)
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(yaw), np.sin(yaw), -np.sin(yaw), np.cos(yaw)
    T[:3, 3] = tx, ty, tz
    return T


POSE0 = pose(1.7, 1.7, 0.2)


def constant_frames(depths, cols=COLS, rows=ROWS):
    return np.repeat(np.asarray(depths, np.uint16)[:, None], cols * rows, axis=1)


def batches(n):
    """The library's own cut of a call: 64 frames at a time."""
    return [(a, min(a + 64, n)) for a in range(0, n, 64)]


def standard_masks(depths, calls, left_from=1200):
    """The masks of a stream of constant-depth frames from POSE0, per launch: the middle and the right unit are in every frame that has depth, the
    left one -- the image's left edge crosses into it 1.11 m from the camera at 96 columns -- in the frames of at least `left_from` mm."""
    assert not any(1100 < d < left_from for d in depths)
    out = []
    for a, b in calls:
        for x, y in batches(b - a):
            m = {K_LEFT: sum(1 << f for f, d in enumerate(depths[a + x:a + y]) if d >= left_from),
                 K_MID: sum(1 << f for f, d in enumerate(depths[a + x:a + y]) if d > 0)}
            m[K_RIGHT] = m[K_MID]
            out.append({k: v for k, v in m.items() if v})
    return out


def case(name, depth, events, cam=None, poses=None, calls=None, preset=None, masks=None, cols=COLS, rows=ROWS, left_from=1200):
    depth = np.ascontiguousarray(depth, np.uint16)
    n = depth.shape[0]
    calls = [(0, n)] if calls is None else calls
    if masks is None:
        masks = standard_masks([int(d) for d in depth.max(axis=1)], calls, left_from)
    return dict(name=name, cols=cols, rows=rows, cam=camera(cols=cols, rows=rows) if cam is None else cam,
                poses=np.stack([POSE0] * n) if poses is None else np.asarray(poses, np.float64), depth=depth,
                calls=calls, preset=preset, masks=masks, events=tuple(events))


# ---- the families ----------------------------------------------------------------------------------------------------------------------
def steps(n):
    """n frames that are band for the same boxes: exactly n projected frames, leaving through the dpb exit for even n."""
    ev = ["E_PROJ_%d" % n if n < 5 else "E_PROJ_5PLUS", "E_ALL_CULLED", "E_PROJ_INSIDE", "E_ROW_STORED", "E_ROW_UNCHANGED"]
    return case("steps-%d" % n, constant_frames([1250, 1252, 1249, 1251, 1250][:n]), ev)


RUN_EVENTS = ("E_RUN_BEFORE_FIRST", "E_RUN_BETWEEN", "E_RUN_AFTER_LAST", "E_RUN_LEN_GE2", "E_FULL_TRIVIAL", "E_FULL_DIVIDE",
              "E_FULL_DIVIDE_LEN_GE2", "E_PROJ_1", "E_PROJ_2", "E_PROJ_3", "E_PROJ_INSIDE", "E_PROJ_TESTED", "E_ROW_STORED", "E_ROW_UNCHANGED")
SURE_EVENTS = ("E_SURE_TAKEN", "E_SURE_DECLINED_UNSURE", "E_SURE_DECLINED_NONTRIVIAL")


def runs(trunc=2.5, name="runs", cols=COLS, rows=ROWS):
    """Full frames before, between and after the projected ones; frame 0 is band for boxes that are full from frame 6 on (the division loop)."""
    return case(name, constant_frames(RUNS, cols, rows), RUN_EVENTS + (SURE_EVENTS[:2] if trunc < 64.0 else ()), camera(trunc, cols=cols, rows=rows),
                cols=cols, rows=rows, left_from=1200 if cols == COLS else 1100)      # (100 columns: the left edge crosses 1.08 m out)


def full_only():
    """Surfaces at 1.40 .. 1.41 m: the front boxes of the units only ever see full frames, the boxes behind 1.44 m none at all."""
    return case("full-only", constant_frames([1200, 1205, 1210, 1200]), ("E_FULL_ONLY", "E_ALL_CULLED", "E_FULL_TRIVIAL", "E_RUN_LEN_GE2"))


def holes(trunc=2.5, name="holes"):
    """runs with holes: frames whose tile minima cannot prove "full" although every voxel is in free space, an empty frame, a pixel beyond the
    truncation (it touches a unit of its own, far away, in which nothing can be updated)."""
    d = constant_frames(RUNS[:6] + [0] + RUNS[6:]).reshape(13, ROWS, COLS)
    one = [(27, 37)]                                                       # (row, column): 16-pixel tile (1, 2) of 32-pixel tile (0, 1)
    four = [(10, 36), (10, 52), (26, 36), (26, 52)]                        # one in each 16-pixel tile of 32-pixel tile (0, 1)
    for f, px in ((0, one), (1, four), (5, one), (7, four), (9, one), (11, four), (12, one)):
        for r, c in px:
            d[f, r, c] = 0
    d[3, 40, 60] = BEYOND
    masks = standard_masks(RUNS[:6] + [0] + RUNS[6:], [(0, 13)])
    masks[0][key(268, 266, 431)] = 1 << 3                                  # where the pixel of 65.5 m lands
    ev = RUN_EVENTS + ("E_PROJ_4", "E_PROJ_5PLUS") + (SURE_EVENTS if trunc < 64.0 else ())
    return case(name, d.reshape(13, -1), ev, camera(trunc), masks=masks)


def bit63(last_is_band, trunc=2.5, prefix=""):
    """64 frames: the batch's last mask bit as a projected frame behind a full one, and as a full frame behind a projected one."""
    if last_is_band:
        return case(prefix + "bit63-band", constant_frames([1250, 1000, 1250, 950] * 16), ("E_FRAME63_PROJECTED", "E_PROJ_5PLUS", "E_RUN_BETWEEN"), camera(trunc))
    return case(prefix + "bit63-full", constant_frames([1000, 1250] * 32), ("E_FRAME63_FULL", "E_PROJ_5PLUS", "E_RUN_AFTER_LAST"), camera(trunc))


CUTS = {"one-call": [(0, 65)], "per-frame": [(f, f + 1) for f in range(65)], "uneven": [(0, 1), (1, 5), (5, 64), (64, 65)]}


def cuts(how):
    """65 frames, handed over three ways; the library's own cut of the single call falls behind frame 63.  State travels between launches."""
    d = constant_frames((RUNS * 6)[:65])
    return case("cuts-" + how, d, ("E_FULL_DIVIDE", "E_ROW_STORED") if how != "per-frame" else ("E_PROJ_1", "E_FULL_DIVIDE"), calls=CUTS[how])


BORDER_POSES = [pose(1.7, 1.7, 1.2, 0.0), pose(1.62, 1.7, 1.15, 0.6), pose(1.8, 1.7, 1.2, -0.8), pose(1.45, 1.7, 1.3, 1.5)]
BORDER_DEPTHS = [300, 250, 400, 350]


def border(trunc=2.5, name="border"):
    """Cameras inside and beside the unit, turned about y: boxes that straddle the image border and the camera plane -- the per-voxel range tests
    and the zero pad behind each frame that failed projections read."""
    return case(name, constant_frames(BORDER_DEPTHS), ("E_PROJ_TESTED", "E_PROJ_PAD", "E_PROJ_INSIDE", "E_ALL_CULLED"), camera(trunc), poses=BORDER_POSES,
                masks=BORDER_MASKS)


BORDER_MASKS = [{K_LEFT: 0b0100, K_MID: 0b1110, key(260, 260, 260): 0b0101}]


FAR_DEPTHS = [60000, 60100, 60320, 60050, 64500, 65535, 60200, 60000]


def far(trunc, name):
    """A long lens 60 m from its surface: scaled depths next to the 64 m bound of voxel_classify (below it with the largest float under 64) and,
    with integration_trunc = 100, beyond it -- which only k_integrate<false> may see."""
    ev = ("E_PROJ_1", "E_FULL_ONLY", "E_FULL_TRIVIAL", "E_ROW_STORED") + (("E_SURE_TAKEN",) if trunc < 64.0 else ())
    return case(name, constant_frames(FAR_DEPTHS), ev, camera(trunc, f=20000.0), masks=FAR_MASKS)


FAR_MASKS = [{key(260, 260, 416): 0b10001011, key(260, 260, 417): 0b01000100, key(260, 260, 428): 0b00010000, key(260, 260, 431): 0b00100000}]


# the planted states of `preset`, one wave box each (i0, j0, k0 of the box in K_MID; all in front of every surface for the first four frames)
PRESET_STATES = [((32, 32, 0), (1.0, 5.0)), ((32, 36, 0), (0.25, 3.0)), ((40, 32, 0), (1.0, 8388607.0)), ((40, 36, 0), (1.0, 8388608.0)),
                 ((24, 32, 0), (0.5, 8388607.0)), ((24, 36, 0), (0.5, 8388608.0)), ((32, 28, 0), (1.0, 16777215.0))]


def preset():
    """runs into a unit that arrives through er_tsdf_import_raw: apply_full's W < 2^23 term from both sides and in both branches, the last exact
    W + 1, ordinary states."""
    sdf, w = np.zeros((64, 64, 64), np.float32), np.zeros((64, 64, 64), np.float32)
    for (i0, j0, k0), (s, ww) in PRESET_STATES:
        sdf[i0:i0 + 8, j0:j0 + 4, k0:k0 + 8] = s
        w[i0:i0 + 8, j0:j0 + 4, k0:k0 + 8] = ww
    return case("preset", constant_frames(RUNS), ("E_FULL_TRIVIAL", "E_FULL_DIVIDE", "E_FULL_DIVIDE_LEN_GE2", "E_RUN_BEFORE_FIRST"),
                preset={K_MID: (sdf.reshape(-1), w.reshape(-1))})


def all_cases():
    out = [steps(n) for n in range(1, 6)]
    out += [runs(), full_only(), holes(), bit63(True), bit63(False)]
    out += [cuts(how) for how in CUTS]
    out += [border(), runs(name="partial-tiles", cols=100, rows=70)]
    for t, tag in ((64.0, "64"), (TRUNC_BELOW_64, "below64")):
        out += [runs(t, "trunc-%s-runs" % tag), holes(t, "trunc-%s-holes" % tag), border(t, "trunc-%s-border" % tag)]
    out += [bit63(True, 64.0, "trunc-64-"), bit63(False, 64.0, "trunc-64-")]     # (so that k_integrate<false> meets mask bit 63 both ways too)
    out += [far(TRUNC_BELOW_64, "far-below64"), far(64.0, "far-64"), far(100.0, "far-100")]
    out.append(preset())
    return out


def no_sure_cases(cases):
    """The fixtures k_integrate<false> runs."""
    return [c for c in cases if float(c["cam"][5]) >= 64.0]
