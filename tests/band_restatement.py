"""Numpy restatement of the band record (csrc/er_tsdf_band.hip, "band records"; include/er_hip.h) and of the owner's sum of the frame-split merge.

Written from the layout comment alone; imports nothing from the library.  A unit is (sdf[262144], weight[262144]) float32, voxel l = (i * 64 + j) * 64 + k.
A record, in 32-bit words:
  [0] flags (bit 0: float32 weights)  [1] observed voxels  [2] band voxels (observed, sdf != 1)  [3] 0
  [4, 132)       exclusive prefix of the observed-voxel counts of the 128 chunks of 2048 voxels
  [132, 260)     ... of the band-voxel counts
  [260, 8452)    observed bitmap: bit (l & 63) of 64-bit word l >> 6 <-> voxel l
  [8452, 16644)  sdf-is-one bitmap
  then           the weights of the observed voxels in voxel order: uint16 in 2 * ((obs + 3) / 4) words, or float32 in (obs + 1) & ~1 words
  then           the sdf of the band voxels in voxel order, float32, in (band + 1) & ~1 words.
The rules the kernels follow: observed <=> weight != 0 (a NaN weight is observed, -0.0 is not); "sdf is one" <=> the bits are 0x3f800000; a unit is
wide <=> some observed weight is not an integer in [1, 65535].

crafted_units() and merge_cases() are the inputs tests/test_band_restatement.py (CPU) and tests/test_band_records_gpu.py (device) share."""
import numpy as np

UNIT_VOX = 64 * 64 * 64
CHUNK = 2048
CHUNKS = UNIT_VOX // CHUNK                 # 128
BITMAP_WORDS = UNIT_VOX // 32              # 8192
OBS_PREFIX, BAND_PREFIX = 4, 4 + CHUNKS
OBS_BITS = BAND_PREFIX + CHUNKS            # 260
ONE_BITS = OBS_BITS + BITMAP_WORDS         # 8452
HEADER = ONE_BITS + BITMAP_WORDS           # 16644
ONE = 0x3f800000
MAX_SRC = 16


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    assert a.size == UNIT_VOX
    return a


def classify(sdf, w):
    """(observed mask, sdf-is-one mask, wide) of a unit."""
    sdf, w = _f32(sdf), _f32(w)
    on = w != 0
    one = on & (sdf.view(np.uint32) == ONE)
    wo = w[on]
    with np.errstate(invalid="ignore"):
        narrow = (wo >= 1) & (wo <= 65535) & (wo == np.floor(wo))
    return on, one, bool((~narrow).any())


def weight_words(obs, wide):
    return ((obs + 1) & ~1) if wide else 2 * ((obs + 3) // 4)


def record_words(sdf, w):
    on, one, wide = classify(sdf, w)
    obs, band = int(on.sum()), int((on & ~one).sum())
    return HEADER + weight_words(obs, wide) + ((band + 1) & ~1)


def pack(sdf, w):
    """The record of a unit as uint32[words]; the padding is zero here (the device leaves it unwritten: defined_bits)."""
    sdf, w = _f32(sdf), _f32(w)
    on, one, wide = classify(sdf, w)
    bandm = on & ~one
    obs, band = int(on.sum()), int(bandm.sum())
    ww = weight_words(obs, wide)
    rec = np.zeros(HEADER + ww + ((band + 1) & ~1), np.uint32)
    rec[0], rec[1], rec[2] = int(wide), obs, band
    per = on.reshape(CHUNKS, CHUNK).sum(axis=1)
    per_b = bandm.reshape(CHUNKS, CHUNK).sum(axis=1)
    rec[OBS_PREFIX:OBS_PREFIX + CHUNKS] = np.cumsum(per) - per
    rec[BAND_PREFIX:BAND_PREFIX + CHUNKS] = np.cumsum(per_b) - per_b
    rec[OBS_BITS:ONE_BITS] = np.packbits(on, bitorder="little").view("<u4")
    rec[ONE_BITS:HEADER] = np.packbits(one, bitorder="little").view("<u4")
    if wide:
        rec[HEADER:HEADER + obs] = w[on].view(np.uint32)
    else:
        half = np.zeros(2 * ww, "<u2")
        half[:obs] = w[on].astype(np.uint16)
        rec[HEADER:HEADER + ww] = half.view("<u4")
    rec[HEADER + ww:HEADER + ww + band] = sdf[bandm].view(np.uint32)
    return rec


def defined_bits(rec):
    """uint32[words]: the bits of every word that a record defines -- all of the header (word 3 is zero), the weights and the sdf values; 0 for the
    padding words, 0x0000ffff for the word that holds the last 16-bit weight of an odd count."""
    rec = np.asarray(rec, np.uint32)
    wide, obs, band = int(rec[0] & 1), int(rec[1]), int(rec[2])
    ww = weight_words(obs, wide)
    assert rec.size == HEADER + ww + ((band + 1) & ~1)
    bits = np.zeros(rec.size, np.uint32)
    bits[:HEADER] = 0xffffffff
    if wide:
        bits[HEADER:HEADER + obs] = 0xffffffff
    else:
        bits[HEADER:HEADER + obs // 2] = 0xffffffff
        if obs & 1:
            bits[HEADER + obs // 2] = 0x0000ffff
    bits[HEADER + ww:HEADER + ww + band] = 0xffffffff
    return bits


def defined_mask(rec):
    """bool[words]: false for the words that are padding altogether.  (The half-word precision is defined_bits'.)"""
    return defined_bits(rec) != 0


def same_record(got, want):
    """Number of words in which `got` differs from `want` in a defined bit (sizes must agree)."""
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    assert got.size == want.size, (got.size, want.size)
    return int(np.count_nonzero((got ^ want) & defined_bits(want)))


def unpack(rec):
    """(sdf, w) of every voxel; an unobserved one is (+0, 0)."""
    rec = np.ascontiguousarray(rec, dtype=np.uint32)
    wide, obs, band = int(rec[0] & 1), int(rec[1]), int(rec[2])
    ww = weight_words(obs, wide)
    on = np.unpackbits(rec[OBS_BITS:ONE_BITS].view(np.uint8), bitorder="little").astype(bool)
    one = np.unpackbits(rec[ONE_BITS:HEADER].view(np.uint8), bitorder="little").astype(bool)
    assert int(on.sum()) == obs and int((on & ~one).sum()) == band and not (one & ~on).any()
    sdf, w = np.zeros(UNIT_VOX, np.float32), np.zeros(UNIT_VOX, np.float32)
    if wide:
        w[on] = rec[HEADER:HEADER + obs].view(np.float32)
    else:
        w[on] = rec[HEADER:HEADER + ww].view("<u2")[:obs].astype(np.float32)
    sdf[one] = np.float32(1.0)
    sdf[on & ~one] = rec[HEADER + ww:HEADER + ww + band].view(np.float32)
    return sdf, w


def merge(own, recs_before, recs_after):
    """The owner's sum: float32, in order -- the records before its own voxels, its own voxels, the records after them --
    SW = SW + fl(sdf_r * w_r), W = W + w_r from +0; (SW / W, W) where W > 0, (+0, 0) elsewhere.  A source is a record, or a (sdf, w) pair that
    stands for its record (a unit a record restores exactly)."""
    SW, W = np.zeros(UNIT_VOX, np.float32), np.zeros(UNIT_VOX, np.float32)
    term = lambda r: (_f32(r[0]), _f32(r[1])) if isinstance(r, tuple) else unpack(r)
    terms = [term(r) for r in recs_before] + [(_f32(own[0]), _f32(own[1]))] + [term(r) for r in recs_after]
    for s, w in terms:
        SW = SW + s * w                                            # (an unobserved voxel adds +0)
        W = W + w
    pos = W > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        sdf = np.where(pos, SW / W, np.float32(0)).astype(np.float32)
    return sdf, np.where(pos, W, np.float32(0)).astype(np.float32)


# ---- the crafted units (the case table of the issue that introduced this file) -----------------------------------------------------------------
def unit_key(xi, yi, zi):
    return xi << 18 | yi << 9 | zi


def _unit(mask, w_values, sdf_values):
    """Unit with `mask` observed: weights / sdf from the given per-observed-voxel arrays, (+0, 0) elsewhere."""
    sdf, w = np.zeros(UNIT_VOX, np.float32), np.zeros(UNIT_VOX, np.float32)
    w[mask] = np.asarray(w_values, np.float32)
    sdf[mask] = np.asarray(sdf_values, np.float32)
    return sdf, w


def _mixed_sdf(rng, n, ones=0.8):
    """n sdf values, a share `ones` exactly 1.0, the rest uniform in (-1, 1) and never 1."""
    s = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    s[s == 1.0] = np.float32(0.5)
    s[rng.random(n) < ones] = np.float32(1.0)
    return s


def _mask(rng, p=0.28):
    return rng.random(UNIT_VOX) < p


def _dense(rng, obs_mod=None, band_odd=None, hi=100, ones=0.81):
    """About 28 % observed, integer weights in [1, hi], a share `ones` of sdf exactly 1; obs % 4 and the parity of band on request."""
    m = _mask(rng)
    if obs_mod is not None:
        idx = np.flatnonzero(m)
        m[idx[:(int(m.sum()) - obs_mod) % 4]] = False
    n = int(m.sum())
    s = _mixed_sdf(rng, n, ones)
    if band_odd is not None and (int((s.view(np.uint32) != ONE).sum()) & 1) != int(band_odd):
        s[np.flatnonzero(s.view(np.uint32) == ONE)[0]] = np.float32(-0.25)
    return _unit(m, rng.integers(1, hi + 1, n), s)


def crafted_units(seed=20260):
    """[(name, (sdf, w), tags)]: tags holds "moved_only" for units with NaN / infinity (never summed) and "raw" for units that break the
    precondition "unobserved voxels are (+0, 0)" (a record restores unpack(pack(u)), not u)."""
    rng = np.random.default_rng(seed)
    out = []

    def add(name, u, *tags):
        out.append((name, (_f32(u[0]), _f32(u[1])), frozenset(tags)))

    add("empty", (np.zeros(UNIT_VOX, np.float32), np.zeros(UNIT_VOX, np.float32)))
    for n in (1, 2, 3, 4, 5):
        m = np.zeros(UNIT_VOX, bool)
        m[rng.choice(UNIT_VOX, n, replace=False)] = True
        add("%d voxels" % n, _unit(m, rng.integers(1, 101, n), rng.uniform(-0.99, 0.99, n)))
    full = np.ones(UNIT_VOX, bool)
    add("full, all one", _unit(full, np.ones(UNIT_VOX), np.ones(UNIT_VOX)))
    add("full, 65535, no one", _unit(full, np.full(UNIT_VOX, 65535.0), rng.uniform(-0.99, 0.99, UNIT_VOX)))
    m = full.copy()
    m[int(rng.integers(0, UNIT_VOX))] = False
    add("all but one", _unit(m, rng.integers(1, 1000, UNIT_VOX - 1), _mixed_sdf(rng, UNIT_VOX - 1)))
    for name, chunks in (("chunk 0 only", (0,)), ("chunk 127 only", (127,)), ("chunks 63 and 64", (63, 64))):
        m = np.zeros(UNIT_VOX, bool)
        for c in chunks:
            m[c * CHUNK:(c + 1) * CHUNK] = rng.random(CHUNK) < 0.6
        n = int(m.sum())
        add(name, _unit(m, rng.integers(1, 200, n), _mixed_sdf(rng, n, 0.5)))
    m = np.zeros(UNIT_VOX, bool)
    m[64 * 1234:64 * 1235] = True
    add("one whole word", _unit(m, rng.integers(1, 200, 64), _mixed_sdf(rng, 64, 0.5)))
    m = np.zeros(UNIT_VOX, bool)
    m[64 * rng.choice(UNIT_VOX // 64, 37, replace=False) + 63] = True
    m[UNIT_VOX - 1] = True
    n = int(m.sum())
    add("bit 63 of several words", _unit(m, rng.integers(1, 200, n), _mixed_sdf(rng, n, 0.5)))
    m = np.zeros(UNIT_VOX, bool)
    m[0] = True
    add("bit 0 only", _unit(m, [7], [-0.125]))
    for obs_mod in range(4):
        for band_odd in (0, 1):
            u = _dense(rng, obs_mod, band_odd, hi=65535)
            u[1][np.flatnonzero(u[1])[5]] = np.float32(65535.0)
            add("dense, obs %% 4 = %d, band %s" % (obs_mod, "odd" if band_odd else "even"), u)
    for name, wv in (("one weight 65536", 65536.0), ("one weight 0.5", 0.5), ("one weight 65535.5", 65535.5), ("one negative weight", -2.0)):
        u = _dense(rng)
        u[1][np.flatnonzero(u[1])[int(rng.integers(0, 1000))]] = np.float32(wv)
        add(name, u)
    u = _dense(rng)
    on = u[1] != 0
    u[1][on] = rng.uniform(0.25, 7e4, int(on.sum())).astype(np.float32)
    add("uniform weights in (0.25, 7e4)", u)
    u = _dense(rng)
    idx = np.flatnonzero(u[1])
    special = np.array([np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2)), -1.0, -0.0, 0.0, 1e-40], np.float32)
    for r in range(20):                                             # each special value on 20 observed voxels, scattered
        u[0][idx[100 + 977 * r + 13 * np.arange(special.size)]] = special
    add("special sdf values", u)
    u = _dense(rng)
    idx = np.flatnonzero(u[1])
    u[1][idx[10]], u[1][idx[20000]] = np.float32(np.nan), np.float32(np.inf)
    u[0][idx[11]] = np.array([0x7fc12345], np.uint32).view(np.float32)[0]
    u[0][idx[12]], u[0][idx[30000]] = np.float32(np.inf), np.float32(-np.inf)
    add("NaN and infinity", u, "moved_only")
    u = _dense(rng)
    off = np.flatnonzero(u[1] == 0)
    u[0][off[::7]] = np.float32(0.3)                                # unobserved, but an sdf is there
    u[1][off[3::11]] = np.float32(-0.0)                             # -0.0 is not observed
    u[0][off[3::22]] = np.float32(-0.75)
    add("precondition violated", u, "raw")
    return out


def crafted_keys(n):
    """Keys for n crafted units: unit index 0 and 511 (per axis) for two of the dense ones, the middle of the lattice for the rest."""
    keys = [unit_key(256, 256, 200 + i) for i in range(n)]
    keys[17] = unit_key(0, 0, 0)
    keys[18] = unit_key(511, 511, 511)
    return keys


# ---- inputs of the owner's sum ------------------------------------------------------------------------------------------------------------------
RESERVED = slice(64 * 1000, 64 * 1001)          # one bitmap word that only the cancelling source and the owners observe


def merge_cases(seed=777):
    """(pool, cases): pool = [(sdf, w)] source units, cases = [dict(key, own=(sdf, w), src=[pool indices in rank order], self_pos, call)].
    nsrc runs over {0, 1, 2, 3, 7, 15, 16}, self_pos over {0, nsrc // 2, nsrc}; call 0 is one merge call of six units whose nsrc and self_pos all
    differ, call 1 holds the other twelve.  No NaN, no infinity."""
    rng = np.random.default_rng(seed)
    m0 = _mask(rng)
    m0[RESERVED] = False

    def unit(mask, hi=100, wide=False, ones=0.8):
        mask = mask.copy()
        mask[RESERVED] = False
        n = int(mask.sum())
        wv = rng.uniform(0.25, 300.0, n) if wide else rng.integers(max(1, hi // 2), hi + 1, n)
        return _unit(mask, wv, _mixed_sdf(rng, n, ones))

    pool = [unit(m0),                                               # 0 narrow
            unit(_mask(rng)),                                       # 1 narrow, another set
            unit(m0, ones=0.3),                                     # 2 the identical set
            unit(m0 & (rng.random(UNIT_VOX) < 0.5)),                # 3 nested in it
            unit(~m0 & _mask(rng)),                                 # 4 disjoint from it
            unit(_mask(rng), wide=True),                            # 5 wide
            unit(np.zeros(UNIT_VOX, bool)),                         # 6 obs = 0
            unit(m0, hi=65535)]                                     # 7 large counts: totals cross 65535
    c = unit(_mask(rng, 0.1))                                       # 8 wide: -3 on the reserved word
    c[1][RESERVED] = np.float32(-3.0)
    c[0][RESERVED] = rng.uniform(-0.9, 0.9, 64).astype(np.float32)
    pool.append(c)
    pool.append(unit(np.ones(UNIT_VOX, bool), hi=3, ones=0.9))      # 9 every voxel
    for i in range(8):                                              # 10..17
        pool.append(unit(_mask(rng, 0.05 + 0.04 * i), hi=50 + 5000 * (i % 3), wide=(i % 4 == 3)))
    combos = [(n, p) for n in (0, 1, 2, 3, 7, 15, 16) for p in sorted({0, n // 2, n})]
    first = [(0, 0), (1, 1), (2, 2), (7, 3), (15, 7), (16, 8)]
    cases = []
    for q, (n, p) in enumerate(combos):
        own = unit(_mask(rng), hi=65535 if q % 3 == 0 else 60, wide=(q % 5 == 1))
        own[1][RESERVED] = np.repeat(np.array([3.0, 2.0, 5.0, 0.0], np.float32), 16)    # + (-3): cancels, goes negative, stays positive, -3 alone
        own[0][RESERVED] = np.where(own[1][RESERVED] != 0, rng.uniform(-0.9, 0.9, 64), 0.0).astype(np.float32)
        if q == 4:
            own = unit(np.zeros(UNIT_VOX, bool))                    # an owner that observed nothing
        order = [int(i) for i in rng.permutation(len(pool))]
        must = [5, 0, 8, 7, 6, 2, 3, 4][:n] if n >= 2 else ([8] if (n, p) == (1, 1) else [7])[:n]
        src = (must + [i for i in order if i not in must])[:n]
        src = [src[int(i)] for i in rng.permutation(n)]
        cases.append(dict(key=unit_key(250, 256, 230 + q), own=own, src=src, self_pos=p, call=0 if (n, p) in first else 1))
    return pool, cases
