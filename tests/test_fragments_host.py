"""fin_records_fragments and fin_effective_lengths, the host statements of the fragment geometry (include/finito_amd.h: FRAGMENT GEOMETRY), against
an independent model.  No GPU.

The model is plain Python over a read's slots, written from the header's definition: `place` (the pileup's rules 1 and 2), `fragment_of` (the classes) and
`stats_of` (histogram and counters).  tests/test_fragments.py runs the same model over the oracle's pairs.  A kind-1 record's slots come from
tests/test_records.py::brute_expand, the record's meaning in three lines.  Nothing is expected from a fin_records_* result; every comparison is exact."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import finito_amd as fa
from tests.test_records import brute_expand

NONE, ONE, SPLIT, TANDEM, OUTWARD, INWARD = range(6)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def place(slots, k, ends):
    """a read's slots [(u, off)] -> (u, s0, L, rev) where strand A lies, or None: not placed.  ends: the unitigs' cumulative ends"""
    nk = len(slots)
    found = [(i, int(u), int(o)) for i, (u, o) in enumerate(slots) if int(u) != -1]
    if len(found) < 2 or any(not 0 <= u < len(ends) for _, u, _ in found) or len({u for _, u, _ in found}) != 1:
        return None
    fwd, rev = len({o - i for i, _, o in found}) == 1, len({o + i for i, _, o in found}) == 1
    if fwd == rev:
        return None
    i, u, o = found[0]
    s0 = o - i if fwd else o + i - nk + 1
    L = nk + k - 1
    ulen = int(ends[u]) - (int(ends[u - 1]) if u else 0)
    if s0 < 0 or s0 + L > ulen:
        return None
    return u, s0, L, rev


def fragment_of(a, b):
    """two mates as `place` gives them -> (u, start, length, cls word)"""
    bits = (0x100 if a and a[3] else 0) | (0x200 if b and b[3] else 0) | (0x400 if a else 0) | (0x800 if b else 0)
    if not a and not b:
        return 0xFFFFFFFF, 0, 0, NONE | bits
    if not a or not b:
        m = a or b
        return m[0], m[1], m[2], ONE | bits
    if a[0] != b[0]:
        return 0xFFFFFFFF, 0, 0, SPLIT | bits
    start = min(a[1], b[1])
    length = max(a[1] + a[2], b[1] + b[2]) - start
    if a[3] == b[3]:
        return a[0], start, length, TANDEM | bits
    F, R = (b, a) if a[3] else (a, b)
    inward = F[1] <= R[1] and F[1] + F[2] <= R[1] + R[2]
    if inward:
        assert length == R[1] + R[2] - F[1]
    return a[0], start, length, (INWARD if inward else OUTWARD) | bits


def fragments_model(pairs, nks, k, ends):
    """FRAGMENT_DTYPE[len(nks) // 2] from every read's slots, back to back in `pairs`"""
    at = np.concatenate([[0], np.cumsum(nks)]).astype(np.int64)
    pl = np.asarray(pairs).reshape(-1, 2).tolist()
    mates = [place(pl[at[r]:at[r + 1]], k, ends) for r in range(len(nks))]
    out = np.zeros(len(nks) // 2, dtype=fa.FRAGMENT_DTYPE)
    for f in range(len(out)):
        out[f] = fragment_of(mates[2 * f], mates[2 * f + 1])
    return out


def stats_of(frags, n_bins, bin_width):
    """(hist uint64[n_bins], counters uint64[7]) of the fragments"""
    cls = frags["cls"] & 0xFF
    counters = [int((cls == c).sum()) for c in range(6)]
    lens = frags["length"][cls == INWARD].astype(np.int64)
    hist = np.bincount(np.minimum(lens // bin_width, n_bins - 1), minlength=n_bins)
    return hist.astype(np.uint64), np.array(counters + [int(lens.sum())], dtype=np.uint64)


def assert_frags(got, want, what=""):
    assert got.dtype == fa.FRAGMENT_DTYPE and got.shape == want.shape, what
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%s: %d fragments differ, first %d: got %s, model %s" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])


def assert_stats(got, want, what=""):
    assert got[0].dtype == np.uint64 and np.array_equal(got[0], want[0]), "%s: histogram: got %s at %s, model %s" % (
        what, got[0][got[0] != want[0]][:4], np.nonzero(got[0] != want[0])[0][:4], want[0][got[0] != want[0]][:4])
    assert got[1].tolist() == want[1].tolist(), "%s: counters %s, model %s" % (what, got[1], want[1])


# ---- hand-made mates ------------------------------------------------------------------------------------------------------------------------
def mate(u, s0, nk, rev, how="scan", Es=()):
    """a straight mate with strand A at offset s0 of u: ('scan', slots) a kind-0 read, ('rec', record fields) a kind-1 record with positions Es"""
    if how == "rec":
        return ("rec", u, s0, nk, rev, tuple(Es))
    return ("scan", [(u, s0 + (nk - 1 - i if rev else i)) for i in range(nk)])


def build(mates):
    """(recs, stream) of a flat list of mates: 'scan', 'rec', ('none', nk) a kind-2 read"""
    recs = np.zeros(len(mates), dtype=fa.RECORD_DTYPE)
    stream = []
    for r, m in zip(recs, mates):
        if m[0] == "scan":
            r["nk"] = len(m[1]); stream += m[1]
        elif m[0] == "none":
            r["nk"], r["meta"] = m[1], 2 << 16
        else:
            _, u, s0, nk, rev, Es = m
            r["u"], r["off0"], r["nk"], r["meta"] = u, s0, nk, len(Es) | (int(rev) << 8) | (1 << 16)
            r["Es"] = sum(E << (16 * e) for e, E in enumerate(Es[:4])); r["Es2"] = sum(E << (16 * e) for e, E in enumerate(Es[4:]))
    return recs, np.array(stream, dtype=np.int32).reshape(-1, 2)


def twin(mates, k, ends, n_bins=64, bin_width=1, n_threads=1):
    recs, stream = build(mates)
    return fa.records_fragments(recs, stream, k, ends, n_bins, bin_width, n_threads), (recs, stream)


def model(recs, stream, k, ends, n_bins=64, bin_width=1):
    fr = fragments_model(brute_expand(recs, stream, k), recs["nk"].astype(np.int64), k, ends)
    return fr, stats_of(fr, n_bins, bin_width)


K = 5
ENDS = np.cumsum([300, 40, 500, K, K + 1, 5_000_000]).astype(np.int64)


def one(a, b, k=K, ends=ENDS):
    """the twin's fragment of two mates, held to the model"""
    (fr, hist, counters), (recs, stream) = twin([a, b], k, ends)
    want, wstats = model(recs, stream, k, ends)
    assert_frags(fr, want, "%s + %s" % (a, b))
    assert_stats((hist, counters), wstats, "%s + %s" % (a, b))
    return tuple(int(x) for x in fr[0])


# ---- classes and the inward rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["scan", "rec"])
def test_every_class_and_every_boundary_of_the_inward_rule(how):
    """expectations stated by hand from the header's table; F forward, R reverse, L = nk + K - 1"""
    F = lambda s0, nk=20, u=0: mate(u, s0, nk, False, how)
    R = lambda s0, nk=20, u=0: mate(u, s0, nk, True, how)
    L = 20 + K - 1
    for first_is_forward in (True, False):
        ab = (lambda f, r: (f, r)) if first_is_forward else (lambda f, r: (r, f))
        bits = 0xC00 | (0x200 if first_is_forward else 0x100)
        cases = [("apart", F(10), R(100), INWARD, 10, 100 + L - 10), ("equal starts", F(50), R(50, 30), INWARD, 50, 30 + K - 1), ("equal ends", F(50, 30), R(60), INWARD, 50, 30 + K - 1),
                 ("equal ends, F longer", F(40, 40), R(60, 20), INWARD, 40, 40 + K - 1), ("identical extents", F(70), R(70), INWARD, 70, L),
                 ("R inside F", F(10, 60), R(20, 20), OUTWARD, 10, 60 + K - 1), ("F inside R", F(20, 20), R(10, 60), OUTWARD, 10, 60 + K - 1),
                 ("dovetail by one base", F(51), R(50), OUTWARD, 50, L + 1), ("dovetail, far", F(200), R(20), OUTWARD, 20, 200 + L - 20),
                 ("F ends one past R", F(50, 21), R(50, 20), OUTWARD, 50, L + 1)]
        for name, f, r, cls, start, length in cases:
            a, b = ab(f, r)
            assert one(a, b) == (0, start, length, cls | bits), "%s, first mate forward %s" % (name, first_is_forward)
    assert one(F(10), F(100)) == (0, 10, 100 + L - 10, TANDEM | 0xC00)
    assert one(R(100), R(10)) == (0, 10, 100 + L - 10, TANDEM | 0xF00)
    assert one(F(10), R(100, u=2)) == (0xFFFFFFFF, 0, 0, SPLIT | 0xE00)
    assert one(F(10), ("none", 7)) == (0, 10, L, ONE | 0x400)
    assert one(("scan", [(-1, -1)] * 9), R(33, 12, u=2)) == (2, 33, 12 + K - 1, ONE | 0xA00)
    assert one(("none", 3), ("scan", [])) == (0xFFFFFFFF, 0, 0, NONE)
    # the unitig's ends: flush with either end is placed, one base over is not; a unitig of exactly one k-mer never places anything
    assert one(F(0, 296), R(300 - L)) == (0, 0, 300, INWARD | 0xE00)
    assert one(mate(4, 0, 2, False, how), ("none", 3)) == (4, 0, K + 1, ONE | 0x400)
    # a straight read that hangs over an end of its unitig, its found slots all inside: not placed
    hang_left = ("scan", [(-1, -1)] * 3 + [(0, i) for i in range(10)])
    hang_right = ("scan", [(0, 290 + i) for i in range(6)] + [(-1, -1)] * 3)
    hang_rev = ("scan", [(-1, -1)] * 3 + [(0, 9 - i) for i in range(10)] + [(-1, -1)] * 3)   # dR = 12, nk = 16: s0 = -3
    assert one(hang_left, hang_right) == (0xFFFFFFFF, 0, 0, NONE) and one(hang_rev, F(10)) == (0, 10, L, ONE | 0x800)


def test_mates_that_are_not_placed():
    ok = mate(2, 100, 12, True)
    placed_one = lambda m: one(m, ok)[3] == (ONE | 0xA00)
    assert placed_one(mate(0, 7, 1, False)) and placed_one(mate(0, 7, 1, False, "rec")), "nk = 1"
    assert placed_one(("scan", [])), "a read shorter than k, an empty read"
    assert placed_one(("scan", [(0, 5), (-1, -1), (-1, -1)])), "one found slot"
    assert placed_one(("scan", [(0, 5), (0, 6), (1, 7)])), "a mosaic"
    assert placed_one(("scan", [(0, 5), (0, 6), (0, 8), (0, 9)])), "an indel"
    assert placed_one(("scan", [(0, 5), (0, 5)])), "a repeated pair"
    assert placed_one(("scan", [(0, 5), (0, 6), (0, 5)])), "both directions"
    assert placed_one(("rec", 0, 3, 12, False, (0, 5, 10, 15))), "a record whose positions leave no found slot"
    assert placed_one(("rec", 0, 3, 12, True, (4, 10, 15))), "a record whose positions leave one found slot"
    assert placed_one(mate(3, 0, 1, False)), "a unitig of exactly one k-mer never places anything"
    assert one(("rec", 0, 3, 12, True, (5, 10)), ok)[3] == SPLIT | 0xF00, "... and two"
    assert one(("scan", [(-1, -1), (0, 9), (-1, -1), (0, 7)]), ok) == (0xFFFFFFFF, 0, 0, SPLIT | 0xF00), "two found slots on the reverse diagonal"
    # the reverse mate's place: strand A begins nk - 1 slots before the first output slot's offset
    assert one(("scan", [(-1, -1), (0, 9), (-1, -1), (0, 7)]), mate(0, 0, 2, False)) == (0, 0, 15, INWARD | 0xD00)


def test_invariance_under_swapping_the_mates_and_reversing_the_unitig():
    rng = np.random.default_rng(4027)
    ulen, seen = 500, set()
    for _ in range(400):
        m = [(int(rng.integers(0, 60)), int(rng.integers(2, 40)), bool(rng.integers(0, 2))) for _ in range(2)]
        a, b = (mate(2, s0, nk, rev, "scan" if rng.random() < 0.5 else "rec") for s0, nk, rev in m)
        u, start, length, cls = one(a, b)
        seen.add(cls & 0xFF)
        swapped = one(b, a)
        assert swapped[:3] == (u, start, length) and swapped[3] & 0xFF == cls & 0xFF
        assert swapped[3] >> 8 == ((cls >> 9) & 1) | (((cls >> 8) & 1) << 1) | (((cls >> 11) & 1) << 2) | (((cls >> 10) & 1) << 3)
        # the unitig stored the other way round: offsets x -> ulen - x, every direction flips
        ra, rb = (mate(2, ulen - s0 - (nk + K - 1), nk, not rev) for s0, nk, rev in m)
        mu, mstart, mlength, mcls = one(ra, rb)
        assert (mu, mlength, mcls & 0xFF) == (u, length, cls & 0xFF) and mstart == ulen - start - length
    assert seen == {TANDEM, OUTWARD, INWARD}


# ---- the twin against the model over random fragments ----------------------------------------------------------------------------------------------------
def random_mates(rng, n):
    kmers = np.diff(np.concatenate([[0], ENDS[:5]])) - K + 1
    out = []
    for _ in range(n):
        t = rng.random()
        u = int(rng.integers(0, 3)); nk = int(rng.integers(2, 26)); s0 = int(rng.integers(0, kmers[u] - nk + 1)); rev = bool(rng.integers(0, 2))
        if t < 0.35:
            out.append(mate(u, s0, nk, rev))
        elif t < 0.7:
            out.append(mate(u, s0, nk, rev, "rec", sorted(int(x) for x in rng.integers(0, nk + K - 1, int(rng.integers(0, 9))))))
        elif t < 0.8:
            slots = mate(u, s0, nk, rev)[1]
            for i in rng.integers(0, nk, int(rng.integers(1, nk))):
                slots[int(i)] = (-1, -1)
            out.append(("scan", slots))
        elif t < 0.9:
            out.append(("scan", mate(u, s0, nk, rev)[1] + mate(int(rng.integers(0, 5)), 0, 1, False)[1] * int(rng.integers(1, 3))))
        elif t < 0.95:
            out.append(("none", nk))
        else:
            out.append(("scan", []))
    return out


def test_twin_equals_model_over_random_fragments():
    rng = np.random.default_rng(4127)
    mates = random_mates(rng, 2 * 15400)   # (more than 15 * 1024 fragments: sixteen threads take a chunk each)
    recs, stream = build(mates)
    want, _ = model(recs, stream, K, ENDS)
    cls = want["cls"] & 0xFF
    assert all((cls == c).sum() >= 50 for c in range(6)), np.bincount(cls)
    for n_bins, bw in ((64, 1), (7, 3), (1, 1), (4096, 1)):
        wstats = stats_of(want, n_bins, bw)
        for T in (1, 3, 16):
            fr, hist, counters = fa.records_fragments(recs, stream, K, ENDS, n_bins, bw, T)
            assert_frags(fr, want, "%d threads" % T)
            assert_stats((hist, counters), wstats, "%d bins of %d, %d threads" % (n_bins, bw, T))
    assert wstats[1][:6].sum() == len(want) and wstats[1][6] == want["length"][cls == INWARD].sum() > 0


@pytest.mark.parametrize("n_bins, bin_width", [(1, 1), (4096, 1), (1, 3), (4096, 3), (5, 1000), (4096, 1000), (16, 1)])
def test_lengths_on_every_bin_edge(n_bins, bin_width):
    edges = sorted({q * bin_width + d for q in (1, 2, 3, n_bins - 2, n_bins - 1, n_bins, n_bins + 1, 2 * n_bins) for d in (-1, 0, 1)})
    lens = [x for x in sorted(set(edges) | {K + 1, K + 2, 100, 4_500_000}) if K + 1 <= x <= 4_900_000]   # (K + 1: the shortest inward fragment there is)
    mates = []
    for x in lens:   # F at 0 with two slots, R ending at x: an inward fragment of length x
        mates += [mate(5, 0, 2, False), mate(5, x - (K + 1), 2, True)]
    (fr, hist, counters), _ = twin(mates, K, ENDS, n_bins, bin_width)
    assert fr["length"].tolist() == lens and (fr["cls"] & 0xFF == INWARD).all()
    want = np.zeros(n_bins, dtype=np.uint64)
    for x in lens:
        want[min(x // bin_width, n_bins - 1)] += 1
    assert np.array_equal(hist, want) and counters[INWARD] == len(lens) and counters[6] == sum(lens)
    assert any(x // bin_width > n_bins - 1 for x in lens), "no length saturates"


def test_refusals():
    ok = [mate(0, 0, 4, False), mate(0, 9, 4, True)]
    recs, stream = build(ok)
    L = fa.lib()
    e = np.ascontiguousarray(ENDS)

    def rc_of(recs, stream, n_reads=None, k=K, n_bins=8, bw=1, want_hist=True, ends=e):
        hist, frags, cnt = np.zeros(4096, dtype=np.uint64), np.zeros(len(recs), dtype=fa.FRAGMENT_DTYPE), np.zeros(7, dtype=np.uint64)
        return L.fin_records_fragments(recs.ctypes.data_as(C.c_void_p), len(recs) if n_reads is None else n_reads, stream.ctypes.data_as(C.c_void_p), len(stream), k,
                                       ends.ctypes.data_as(C.POINTER(C.c_int64)), len(ends), n_bins, bw, frags.ctypes.data_as(C.c_void_p),
                                       hist.ctypes.data_as(C.c_void_p) if want_hist else None, cnt.ctypes.data_as(C.c_void_p), 1)
    assert rc_of(recs, stream) == 0
    assert rc_of(recs, stream, n_bins=0, want_hist=False) == 0, "n_bins is looked at only with a histogram"
    assert rc_of(recs[:1], stream[:4]) == fa.FIN_EINVAL, "an odd n_reads"
    for nb, bw in ((0, 1), (4097, 1), (8, 0)):
        assert rc_of(recs, stream, n_bins=nb, bw=bw) == fa.FIN_EINVAL
    assert rc_of(recs, stream, k=0) == fa.FIN_EINVAL
    assert rc_of(recs, stream[:-1]) == fa.FIN_EINVAL, "a stream that is not this record set's"
    assert rc_of(*build([mate(6, 0, 4, False), ok[1]])) == fa.FIN_EINVAL, "a unitig number outside the index"
    assert rc_of(*build([mate(6, 0, 4, False, "rec"), ok[1]])) == fa.FIN_EINVAL, "a record outside the index"
    assert rc_of(*build([mate(1, 40 - K - 2, 4, False), ok[1]])) == fa.FIN_EINVAL, "a k-mer that does not lie inside its unitig"
    assert rc_of(*build([("scan", [(-2, 0), (0, 1)]), ok[1]])) == fa.FIN_EINVAL
    bad = recs.copy(); bad["meta"][0] = 3 << 16
    assert rc_of(bad, stream[4:]) == fa.FIN_EINVAL, "a kind above 2"
    assert rc_of(recs, stream, ends=np.array([10, 5], dtype=np.int64)) == fa.FIN_EINVAL, "ends that descend"
    fr, hist, cnt = fa.records_fragments(recs[:0], stream[:0], K, ENDS)
    assert len(fr) == 0 and not hist.any() and not cnt.any()
    with pytest.raises(fa.FinitoError) as err:
        fa.records_fragments(recs[:1], stream[:4], K, ENDS)
    assert err.value.code == fa.FIN_EINVAL and "odd" in str(err.value)


# ---- effective lengths --------------------------------------------------------------------------------------------------------------------------------
def eff_numpy(hist, ref_len):
    """the header's expression in numpy: uint64 prefix sums, one float64 division"""
    h = np.asarray(hist, dtype=np.uint64)
    nb = len(h) - 1
    out = np.asarray(ref_len, dtype=np.uint64).astype(np.float64)
    if nb == 0:
        return out
    with np.errstate(over="ignore"):
        S0, S1 = np.cumsum(h[:nb], dtype=np.uint64), np.cumsum(h[:nb] * np.arange(nb, dtype=np.uint64), dtype=np.uint64)
    m = np.minimum(np.asarray(ref_len, dtype=np.uint64), np.uint64(nb - 1)).astype(np.int64)
    s0, s1 = S0[m], S1[m]
    with np.errstate(divide="ignore", invalid="ignore"):
        v = out + 1.0 - s1.astype(np.float64) / s0.astype(np.float64)
    return np.where((s0 > 0) & (v >= 1.0), v, out)


def test_effective_lengths():
    rng = np.random.default_rng(4227)
    for n_bins in (1, 2, 3, 300, 4096):
        hist = rng.integers(0, 1000, n_bins).astype(np.uint64)
        hist[: min(n_bins // 3, 120)] = 0   # no fragment shorter than that
        ref = np.concatenate([np.arange(0, min(n_bins + 5, 400)), rng.integers(0, 3 * n_bins + 10, 200), [10**6, 2**40, 2**63]]).astype(np.uint64)
        got = fa.effective_lengths(hist, ref)
        want = eff_numpy(hist, ref)
        assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), "n_bins %d: not the header's expression bit for bit" % n_bins
        # ... and within one ulp of the exact rational.  The ulp is that of the larger of the result and ref_len: the quotient (the mean, at most ref_len) is off
        # by half an ulp of its own, the difference by half an ulp of the result, (double)ref_len + 1 by half an ulp of ref_len where it is not exact
        for r, g in zip(ref.tolist(), got.tolist()):
            m = min(r, n_bins - 2)
            s0 = sum(int(x) for x in hist[: m + 1]) if m >= 0 else 0
            if s0 == 0:
                assert g == float(r), "the fall-back: no fragment fits"
                continue
            exact = Fraction(r + 1) - Fraction(sum(j * int(x) for j, x in enumerate(hist[: m + 1])), s0)
            assert exact >= 1 and g >= 1.0   # (the mean of lengths <= ref_len: "below 1" can only be a rounding's doing)
            assert abs(Fraction(g) - exact) <= Fraction(float(np.spacing(max(g, float(r))))), (n_bins, r, g, float(exact))
        if n_bins >= 300:
            shortest = int(np.nonzero(hist)[0][0])
            assert shortest >= 100 and (got[:shortest] == ref[:shortest].astype(np.float64)).all(), "ref_len below the shortest fragment: no fragment fits"
            assert (got[shortest + 1:300] < ref[shortest + 1:300].astype(np.float64)).all()
    # the last bin is "this much or more" and takes no part; a histogram with nothing below it falls back
    h = np.array([0, 0, 4, 0, 4, 10**9], dtype=np.uint64)
    assert fa.effective_lengths(h, [1, 2, 3, 4, 5, 100]).tolist() == [1.0, 1.0, 2.0, 2.0, 3.0, 98.0]
    assert fa.effective_lengths(np.array([0, 0, 0, 7], dtype=np.uint64), [0, 5, 50]).tolist() == [0.0, 5.0, 50.0]
    assert fa.effective_lengths(np.array([7], dtype=np.uint64), [5]).tolist() == [5.0]
    assert fa.effective_lengths(np.array([0, 0, 0, 1, 0], dtype=np.uint64), [3]).tolist() == [1.0], "the value 1 stands"
    assert fa.effective_lengths(np.array([0, 0, 0, 0, 1, 0], dtype=np.uint64), [3, 4]).tolist() == [3.0, 1.0]
    # counts past 2^53: the sums are uint64, each rounded to a double once
    big = np.array([0, 2**53 + 1, 2**54 + 3, 2**55 + 5, 0], dtype=np.uint64)
    got = fa.effective_lengths(big, [1, 2, 3, 1000])
    assert got.tobytes() == eff_numpy(big, [1, 2, 3, 1000]).tobytes()
    s0, s1 = 2**53 + 1 + 2**54 + 3 + 2**55 + 5, 2**53 + 1 + 2 * (2**54 + 3) + 3 * (2**55 + 5)
    assert got[3] == 1001.0 - float(s1) / float(s0)
    for bw in (0, 2, 1000):
        with pytest.raises(fa.FinitoError) as e:
            fa.effective_lengths(h, [5], bin_width=bw)
        assert e.value.code == fa.FIN_EINVAL and "bin_width" in str(e.value)
    for bad in (np.zeros(0, dtype=np.uint64), np.zeros(4097, dtype=np.uint64)):
        with pytest.raises(fa.FinitoError):
            fa.effective_lengths(bad, [5])
