"""tests/band_restatement.py on the CPU: the record it packs follows the documented layout (sizes, header, prefixes, padding), restores a unit bit
for bit, and its owner's sum stays within the derived float32 error of a float64 computation.  The crafted units and merge cases the device
tests (tests/test_band_records_gpu.py) feed to the kernels are checked here to hold what they are meant to hold."""
import numpy as np
import pytest

import band_restatement as br
import helpers

CRAFTED = br.crafted_units()
NAMES = [c[0] for c in CRAFTED]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_unit(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


@pytest.fixture(scope="module")
def merge_inputs():
    pool, cases = br.merge_cases()
    return pool, cases, [br.pack(*u) for u in pool]


@pytest.mark.parametrize("name", NAMES)
def test_record_round_trip_size_header_and_prefixes(name):
    _, u, tags = CRAFTED[NAMES.index(name)]
    sdf, w = u
    rec = br.pack(sdf, w)
    back = br.unpack(rec)
    on = w != 0
    if "raw" in tags:                                                # the record drops what unobserved voxels held
        assert not same_unit(back, u)
        want = (np.where(on, sdf, np.float32(0)), np.where(on, w, np.float32(0)))
        assert (bits(want[1])[~on] == 0).all()
    else:
        assert (bits(sdf)[~on] == 0).all() and (bits(w)[~on] == 0).all(), "the unit breaks the precondition"
        want = u
    assert same_unit(back, want)
    assert np.array_equal(br.pack(*back), rec)
    assert rec.size == helpers.band_record_words(sdf, w) == br.record_words(sdf, w) and rec.size % 2 == 0
    # a straightforward recount, voxel by voxel
    obs = band = 0
    wide = False
    pre, pre_b = [], []
    sb, wl = bits(sdf).tolist(), w.tolist()
    for c in range(br.CHUNKS):
        pre.append(obs)
        pre_b.append(band)
        for l in range(c * br.CHUNK, (c + 1) * br.CHUNK):
            x = wl[l]
            if x != 0:
                obs += 1
                band += sb[l] != 0x3f800000
                wide = wide or not (1 <= x <= 65535 and x == int(x))
    assert [int(x) for x in rec[:4]] == [int(wide), obs, band, 0]
    assert rec[br.OBS_PREFIX:br.BAND_PREFIX].tolist() == pre and rec[br.BAND_PREFIX:br.OBS_BITS].tolist() == pre_b
    # bitmaps, bit by bit, for a sample of voxels and for the ends of the words
    rng = np.random.default_rng(1)
    for l in [0, 63, 64, br.UNIT_VOX - 1] + [int(x) for x in rng.integers(0, br.UNIT_VOX, 500)] + [int(x) for x in np.flatnonzero(on)[:200]]:
        word64 = int(rec[br.OBS_BITS + 2 * (l >> 6)]) | int(rec[br.OBS_BITS + 2 * (l >> 6) + 1]) << 32
        one64 = int(rec[br.ONE_BITS + 2 * (l >> 6)]) | int(rec[br.ONE_BITS + 2 * (l >> 6) + 1]) << 32
        assert (word64 >> (l & 63)) & 1 == int(on[l])
        assert (one64 >> (l & 63)) & 1 == int(on[l] and sb[l] == 0x3f800000)
    # the values sit where the padding rules put them
    ww = (obs + 1) & ~1 if wide else 2 * ((obs + 3) // 4)
    idx = np.flatnonzero(on)
    if obs:
        for q in {0, obs // 2, obs - 1}:
            if wide:
                assert rec[br.HEADER + q] == bits(w)[idx[q]]
            else:
                assert (int(rec[br.HEADER + q // 2]) >> (16 * (q & 1))) & 0xffff == int(w[idx[q]])
    bidx = np.flatnonzero(on & (bits(sdf) != 0x3f800000))
    for q in ({0, band // 2, band - 1} if band else ()):
        assert rec[br.HEADER + ww + q] == bits(sdf)[bidx[q]]
    # what defined_bits leaves out: at most 3 half-words and 1 word (narrow), 2 words (wide), all behind the last weight / the last sdf value
    db = br.defined_bits(rec)
    assert (db[:br.HEADER] == 0xffffffff).all() and np.array_equal(br.defined_mask(rec), db != 0)
    undefined_half_words = int(sum(2 - bin(int(x)).count("1") // 16 for x in db[br.HEADER:br.HEADER + ww]))
    undefined_sdf_words = int((db[br.HEADER + ww:] == 0).sum())
    assert undefined_sdf_words == (band & 1)
    if wide:
        assert undefined_half_words == 2 * (obs & 1)
    else:
        assert undefined_half_words == (-obs) % 4 <= 3
    assert (rec & ~db == 0).all()                                    # (pack zeroes them)


def test_the_case_table_holds_what_it_claims():
    stat = {}
    for name, (sdf, w), tags in CRAFTED:
        on, one, wide = br.classify(sdf, w)
        stat[name] = (int(on.sum()), int((on & ~one).sum()), wide, on, tags)
    obs_of = lambda n: stat[n][0]
    assert obs_of("empty") == 0 and [obs_of("%d voxels" % n) for n in (1, 2, 3, 4, 5)] == [1, 2, 3, 4, 5]
    assert stat["full, all one"][:3] == (br.UNIT_VOX, 0, False) and stat["full, 65535, no one"][:3] == (br.UNIT_VOX, br.UNIT_VOX, False)
    assert obs_of("all but one") == br.UNIT_VOX - 1 and 0.75 < 1 - stat["all but one"][1] / obs_of("all but one") < 0.85
    per_chunk = lambda n: stat[n][3].reshape(br.CHUNKS, br.CHUNK).sum(axis=1)
    assert np.flatnonzero(per_chunk("chunk 0 only")).tolist() == [0] and np.flatnonzero(per_chunk("chunk 127 only")).tolist() == [127]
    assert np.flatnonzero(per_chunk("chunks 63 and 64")).tolist() == [63, 64]
    words = lambda n: np.packbits(stat[n][3], bitorder="little").view("<u8")
    assert (words("one whole word") == 0xffffffffffffffff).sum() == 1 and obs_of("one whole word") == 64
    assert obs_of("bit 63 of several words") >= 30 and set(words("bit 63 of several words").tolist()) == {0, 1 << 63}
    assert obs_of("bit 0 only") == 1 and words("bit 0 only")[0] == 1
    dense = [n for n in NAMES if n.startswith("dense")]
    assert sorted((obs_of(n) % 4, stat[n][1] % 2) for n in dense) == [(a, b) for a in range(4) for b in range(2)]
    for n in dense:
        _, (sdf, w), _ = CRAFTED[NAMES.index(n)]
        assert not stat[n][2] and w.max() == 65535 and 0.25 < obs_of(n) / br.UNIT_VOX < 0.31 and 0.79 < 1 - stat[n][1] / obs_of(n) < 0.83
    for n, v in (("one weight 65536", 65536.0), ("one weight 0.5", 0.5), ("one weight 65535.5", 65535.5), ("one negative weight", -2.0)):
        _, (sdf, w), _ = CRAFTED[NAMES.index(n)]
        odd = w[(w != 0) & ~((w >= 1) & (w <= 65535) & (w == np.floor(w)))]
        assert stat[n][2] and odd.tolist() == [v]                    # wide because of that ONE weight
    assert stat["uniform weights in (0.25, 7e4)"][2]
    _, (sdf, w), _ = CRAFTED[NAMES.index("special sdf values")]
    seen = set(bits(sdf)[w != 0].tolist())
    assert {0x3f7fffff, 0x3f800001, 0xbf800000, 0x80000000, 0x00000000, 0x3f800000} <= seen and any(0 < b < 0x00800000 for b in seen)
    _, (sdf, w), tags = CRAFTED[NAMES.index("NaN and infinity")]
    assert "moved_only" in tags and np.isnan(w).sum() == 1 and np.isinf(w).sum() == 1 and 0x7fc12345 in bits(sdf)[w != 0].tolist()
    assert np.isposinf(sdf[w != 0]).any() and np.isneginf(sdf[w != 0]).any()
    for name, (sdf, w), tags in CRAFTED:
        assert ("moved_only" in tags) == bool(np.isnan(sdf).any() or np.isnan(w).any() or np.isinf(sdf).any() or np.isinf(w).any()), name
    _, (sdf, w), tags = CRAFTED[NAMES.index("precondition violated")]
    assert "raw" in tags and ((w == 0) & (sdf != 0)).sum() > 1000 and (bits(w) == 0x80000000).sum() > 1000
    assert ((bits(w) == 0x80000000) & (sdf != 0)).sum() > 100
    assert [n for n in NAMES if "raw" in stat[n][4]] == ["precondition violated"]
    # both formats, and the lattice corners
    assert sum(1 for n in NAMES if stat[n][2]) >= 6 and sum(1 for n in NAMES if not stat[n][2] and stat[n][0]) >= 15
    keys = br.crafted_keys(len(CRAFTED))
    assert len(set(keys)) == len(keys) and 0 in keys and (511 << 18 | 511 << 9 | 511) in keys
    assert all(0 <= k < 1 << 27 for k in keys)


def test_the_merge_cases_hold_what_they_claim(merge_inputs):
    pool, cases, recs = merge_inputs
    for u in pool + [c["own"] for c in cases]:
        assert np.isfinite(u[0]).all() and np.isfinite(u[1]).all()
        assert (bits(u[0])[u[1] == 0] == 0).all() and (bits(u[1])[u[1] == 0] == 0).all()
    wide = [bool(r[0] & 1) for r in recs]
    assert any(wide) and not all(wide) and any(int(r[1]) == 0 for r in recs)
    combos = sorted((len(c["src"]), c["self_pos"]) for c in cases)
    assert combos == sorted((n, p) for n in (0, 1, 2, 3, 7, 15, 16) for p in {0, n // 2, n})
    assert max(len(c["src"]) for c in cases) == br.MAX_SRC == 16
    assert all(len(set(c["src"])) == len(c["src"]) for c in cases) and len(set(c["key"] for c in cases)) == len(cases)
    first = [c for c in cases if c["call"] == 0]
    assert len(first) >= 5 and len(set(len(c["src"]) for c in first)) == len(first) == len(set(c["self_pos"] for c in first))
    assert any(len(set(wide[i] for i in c["src"])) == 2 for c in cases), "no sum of mixed formats"
    assert any(br.classify(*c["own"])[2] for c in cases) and any(not c["own"][1].any() for c in cases)
    on = [u[1] != 0 for u in pool]
    pairs = [(a, b) for c in cases for a in c["src"] for b in c["src"] if a < b and on[a].any() and on[b].any()]
    assert any(not (on[a] & on[b]).any() for a, b in pairs), "no disjoint sources"
    assert any(np.array_equal(on[a], on[b]) for a, b in pairs), "no identical sets"
    assert any(((on[a] & on[b]) == on[b]).all() and on[a].sum() > on[b].sum() for a, b in pairs + [(b, a) for a, b in pairs]), "no nested sets"
    crossing = cancelling = negative = 0
    for c in cases:
        p = c["self_pos"]
        sdf, w = br.merge(c["own"], [recs[i] for i in c["src"][:p]], [recs[i] for i in c["src"][p:]])
        c_on, c_one, c_wide = br.classify(sdf, w)
        crossing += int(c_wide and w.max() > 65535)
        W64 = c["own"][1].astype(np.float64) + sum(pool[i][1].astype(np.float64) for i in c["src"])
        touched = (c["own"][1] != 0) | np.logical_or.reduce([on[i] for i in c["src"]] + [np.zeros(br.UNIT_VOX, bool)])
        cancelling += int((touched & (W64 == 0)).any())
        negative += int((W64 < 0).any())
        assert (bits(sdf)[W64 <= 0] == 0).all() and (bits(w)[W64 <= 0] == 0).all()
    assert crossing >= 3 and cancelling >= 2 and negative >= 2


def test_merge_stays_within_the_float32_error_of_a_float64_sum(merge_inputs):
    """|SW32 - SW64| <= (n + 1) 2^-24 sum |sdf_r w_r| for n terms (n products and n - 1 inexact additions, each rounded once), the same for W; W is
    exact where all weights are integers and their sum is below 2^24.  No product here underflows: the only denormal sdf values of the inputs
    come with integer weights."""
    pool, cases, recs = merge_inputs
    u = 2.0 ** -24
    for c in cases:
        p = c["self_pos"]
        terms = [pool[i] for i in c["src"][:p]] + [c["own"]] + [pool[i] for i in c["src"][p:]]
        n = len(terms)
        SW64 = sum(s.astype(np.float64) * w.astype(np.float64) for s, w in terms)
        W64 = sum(w.astype(np.float64) for s, w in terms)
        A = sum(np.abs(s.astype(np.float64) * w.astype(np.float64)) for s, w in terms)
        AW = sum(np.abs(w.astype(np.float64)) for s, w in terms)
        SW32, W32 = np.zeros(br.UNIT_VOX, np.float32), np.zeros(br.UNIT_VOX, np.float32)
        for s, w in terms:
            SW32 = SW32 + s * w
            W32 = W32 + w
        assert (np.abs(SW32 - SW64) <= (n + 1) * u * A).all() and (np.abs(W32 - W64) <= (n + 1) * u * AW).all()
        integral = np.logical_and.reduce([w == np.floor(w) for s, w in terms]) & (AW < 2 ** 24)
        assert integral.sum() > 1000 and (W32[integral] == W64[integral]).all()
        sdf, w = br.merge(c["own"], [recs[i] for i in c["src"][:p]], [recs[i] for i in c["src"][p:]])
        pos = W64 > 0
        assert np.array_equal(w > 0, pos) and np.array_equal(bits(w)[pos], bits(W32)[pos])
        with np.errstate(divide="ignore", invalid="ignore"):
            assert np.array_equal(bits(sdf)[pos], bits(SW32 / W32)[pos])
        assert (bits(sdf)[~pos] == 0).all() and (bits(w)[~pos] == 0).all()


def test_merge_of_the_crafted_units_as_sources():
    """Every crafted unit that may be summed, as a record in front of and behind one owner: the result is the two-term sum, and a source that is
    all there is (the owner observed nothing) comes back as fl((+0 + fl(s w)) / w): an observed -0.0 becomes +0."""
    empty = (np.zeros(br.UNIT_VOX, np.float32), np.zeros(br.UNIT_VOX, np.float32))
    for name, (sdf, w), tags in CRAFTED:
        if "moved_only" in tags:
            continue
        rec = br.pack(sdf, w)
        a, b = br.merge(empty, [rec], []), br.merge(empty, [], [rec])
        assert same_unit(a, b)
        s, x = br.unpack(rec)
        pos = x > 0
        assert np.array_equal(bits(a[1]), bits(np.where(pos, x, np.float32(0))))
        assert np.array_equal(bits(a[0])[pos], bits((np.float32(0) + s * x) / np.where(pos, x, np.float32(1)))[pos]) and (bits(a[0])[~pos] == 0).all()
