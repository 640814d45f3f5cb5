"""Paired-end pseudoalignment, the parts that need no GPU (include/finito_amd.h: fin_pair_pseudo, fin_records_pseudoalign_paired).  The
expectation is always the numpy definition, tests/test_colors_host.py::rows_of, applied to the pairs with nks_frag[f] = nks[2f] + nks[2f + 1] -- a fragment's
slots are its mates' slots back to back --; n_colored_first comes from the per-read heads of the even reads.  The closed form of DESIGN.md 4.17 is written
out in Python and its algebra checked against the definition exhaustively (the device's code for it is tested on the GPU); the two identities (AND or the other at 1000, OR at 0) are cross-checks."""
import ctypes as C

import numpy as np
import pytest

import finito_amd as fa
from tests.test_colors_host import pack, random_matrix, rows_of, words_of
from tests.util import hand_made_case

PERMILLES = (0, 300, 1000)


def frags_of(pairs, nks, bits, n_colors, permille, both=False):
    """the definition for interleaved mates: (rows uint64[F, W], heads PAIR_PSEUDO_DTYPE[F]).  rows_of over the pooled slots; the first mate's share of n_colored
    from rows_of's per-read heads; FIN_PAIR_BOTH zeroes the row and n_colors of a fragment one of whose mates has no coloured slot"""
    nks = np.asarray(nks, dtype=np.int64)
    assert len(nks) % 2 == 0
    rows, h = rows_of(pairs, nks[0::2] + nks[1::2], bits, n_colors, permille)
    per_read = rows_of(pairs, nks, bits, n_colors, permille)[1]
    first, second = per_read["n_colored"][0::2], per_read["n_colored"][1::2]
    heads = np.zeros(len(h), dtype=fa.PAIR_PSEUDO_DTYPE)
    heads["n_found"], heads["n_colored"], heads["n_colors"], heads["n_colored_first"] = h["n_found"], h["n_colored"], h["n_colors"], first
    assert (heads["n_colored"] == first + second).all() and (heads["n_found"] == per_read["n_found"][0::2] + per_read["n_found"][1::2]).all()
    return only_both((rows, heads)) if both else (rows, heads)


def only_both(want):
    """FIN_PAIR_BOTH from FIN_PAIR_ANY's expectation"""
    rows, heads = np.array(want[0]), np.array(want[1])
    lone = (heads["n_colored_first"] == 0) | (heads["n_colored_first"] == heads["n_colored"])
    rows[lone] = 0
    heads["n_colors"][lone] = 0
    return rows, heads


def assert_frags(got, want, what=""):
    rows, heads = got
    wrows, wheads = want
    assert heads.dtype == fa.PAIR_PSEUDO_DTYPE and heads.shape == wheads.shape and rows.dtype == np.uint64 and rows.shape == wrows.shape, what
    for f in ("n_found", "n_colored", "n_colors", "n_colored_first"):
        bad = np.nonzero(heads[f] != wheads[f])[0]
        assert len(bad) == 0, "%s: field %s differs in %d fragments, first %d: got %s, want %s" % (what, f, len(bad), bad[0], heads[bad[0]], wheads[bad[0]])
    bad = np.nonzero((rows != wrows).any(axis=1))[0]
    assert len(bad) == 0, "%s: the row differs in %d fragments, first %d: got %s, want %s" % (what, len(bad), bad[0], rows[bad[0]], wrows[bad[0]])


def closed_form(wa, wb, na, nb, permille):
    """the closed form of DESIGN.md 4.17 for two mates of one unitig each, written out in Python: word arrays in, the fragment's word out (permille may be an
    array).  This is the algebra, not the device code: that is run on these inputs by tests/test_paired.py (hand-made records, thresholds on both sides of
    1000 ca / (ca + cb))"""
    ca = na if (na > 0 and wa != 0) else 0
    cb = nb if (nb > 0 and wb != 0) else 0
    need = permille * (ca + cb)
    xa, xb = (wa if ca else 0), (wb if cb else 0)
    pa = (ca >= 1) & (1000 * ca >= need)
    pb = (cb >= 1) & (1000 * cb >= need)
    pab = (ca + cb >= 1) & (need == need)
    M = lambda p: np.where(p, 7, 0)
    return (xa & xb & M(pab)) | (xa & ~xb & 7 & M(pa)) | (xb & ~xa & 7 & M(pb))


def test_the_closed_form_is_the_definition_exhaustively():
    """The ALGEBRA of the closed form (its Python statement above, not the kernel) against the definition: na, nb in 0 .. 6, every permille 0 .. 1000, every pattern of wa and wb over 3 colours (empty rows included), ua == ub and ua != ub.  The definition for all
    1001 thresholds is written over arrays (cnt, n_colored, the two comparisons); at the thresholds of `probe` -- the ends, and both sides of every ratio a / b
    with b <= 12 that is near them -- the same fragments go through rows_of itself, so the array form is tied to it"""
    pm = np.arange(0, 1001, dtype=np.int64)
    probe = sorted({0, 1, 142, 143, 166, 167, 250, 251, 300, 333, 334, 499, 500, 501, 545, 546, 600, 666, 667, 750, 857, 858, 999, 1000})
    # unitigs 0 .. 7 have the row pattern of their number; 8 .. 15 the same patterns again, so that equal rows occur in one unitig and in two
    bits = np.array([[u & 7] for u in range(16)], dtype=np.uint64)
    frag_pairs, frag_nks, keys = [], [], []
    for na in range(7):
        for nb in range(7):
            for wa in range(8):
                for wb in range(8):
                    for same in ((False, True) if wa == wb else (False,)):
                        ua, ub = wa, (wb if same else wb + 8)
                        # the definition over arrays of thresholds
                        ca, cb = (na if wa else 0), (nb if wb else 0)
                        want = np.zeros(len(pm), dtype=np.int64)
                        for c in range(3):
                            cnt = ca * ((wa >> c) & 1) + cb * ((wb >> c) & 1)
                            want |= np.where((cnt >= 1) & (1000 * cnt >= pm * (ca + cb)), 1 << c, 0)
                        got = closed_form(wa, wb, na, nb, pm)
                        assert np.array_equal(got, want), "na %d nb %d wa %d wb %d: first at permille %d" % (na, nb, wa, wb, int(np.nonzero(got != want)[0][0]))
                        frag_pairs += [(ua, i) for i in range(na)] + [(ub, i) for i in range(nb)]
                        frag_nks += [na, nb]
                        keys.append((na, nb, wa, wb))
    assert len(keys) == 49 * (64 + 8)
    for p in probe:
        rows, heads = frags_of(frag_pairs, frag_nks, bits, 3, p)
        mine = np.array([int(closed_form(wa, wb, na, nb, np.int64(p))) for na, nb, wa, wb in keys], dtype=np.uint64)
        bad = np.nonzero(rows[:, 0] != mine)[0]
        assert len(bad) == 0, "permille %d: %s gives %d, rows_of %d" % (p, keys[bad[0]], mine[bad[0]], rows[bad[0], 0])
        assert np.array_equal(heads["n_colored_first"], [na if wa else 0 for na, nb, wa, wb in keys])


def test_the_definition_on_small_fragments():
    # unitig: 0 {0,1}, 1 {1,2}, 2 {3}, 3 {} (uncoloured), 4 {0,1,2,3}
    n_colors = 4
    bits = pack([[0, 1], [1, 2], [3], [], [0, 1, 2, 3]], n_colors)
    A = (-1, -1)

    def ask(a, b, permille, both=False):
        rows, heads = frags_of(list(a) + list(b), [len(a), len(b)], bits, n_colors, permille, both)
        return [c for c in range(n_colors) if (int(rows[0, 0]) >> c) & 1], tuple(int(x) for x in heads[0].tolist())

    # an ambiguous mate {0,1} resolved by its partner {1,2}: the AND; the union at 0; counts 0: 2, 1: 3, 2: 1 of 3 at 500
    assert ask([(0, 5), (0, 6)], [(1, 0)], 1000) == ([1], (3, 3, 1, 2)) and ask([(0, 5), (0, 6)], [(1, 0)], 0) == ([0, 1, 2], (3, 3, 3, 2))
    assert ask([(0, 5), (0, 6)], [(1, 0)], 500) == ([0, 1], (3, 3, 2, 2)) and ask([(1, 0)], [(0, 5), (0, 6)], 500) == ([0, 1], (3, 3, 2, 1))
    # disjoint mates: an empty AND
    assert ask([(0, 1)], [A, (2, 7), (2, 8)], 1000) == ([], (3, 3, 0, 1))
    # a mate without coloured slots (absent, uncoloured, no k-mers at all): the other mate's row -- and nothing under FIN_PAIR_BOTH, counts kept
    for lone in ([A, A], [(3, 0), (3, 1)], []):
        nf = sum(1 for u, _ in lone if u >= 0)
        assert ask([(0, 1), (1, 1)], lone, 1000) == ([1], (2 + nf, 2, 1, 2)) and ask(lone, [(0, 1), (1, 1)], 1000) == ([1], (2 + nf, 2, 1, 0))
        assert ask([(0, 1), (1, 1)], lone, 1000, both=True) == ([], (2 + nf, 2, 0, 2)) and ask(lone, [(0, 1), (1, 1)], 0, both=True) == ([], (2 + nf, 2, 0, 0))
    assert ask([(0, 1)], [(1, 1)], 1000, both=True) == ([1], (2, 2, 1, 1))
    assert ask([], [], 0) == ([], (0, 0, 0, 0)) and ask([A], [(3, 0)], 0) == ([], (1, 0, 0, 0))
    # swapping the mates and reversing either mate's slots changes the row and every count but n_colored_first
    a, b = [(3, 0), (0, 1), A, (0, 2)], [(4, 0), (1, 3), (1, 4)]
    for pm in PERMILLES:
        r0, h0 = ask(a, b, pm)
        for x, y in ((b, a), (a[::-1], b), (a, b[::-1])):
            r1, h1 = ask(x, y, pm)
            assert r1 == r0 and h1[:3] == h0[:3]
        assert ask(b, a, pm)[1][3] == h0[1] - h0[3]


def even_case(k):
    """hand_made_case's records as interleaved mates: the last of its 3 019 reads is dropped"""
    c = hand_made_case(k)
    n = len(c.recs) - 1
    assert n % 2 == 0
    last_pairs = int(c.recs["nk"][-1])
    stream = c.stream[: len(c.stream) - last_pairs] if (c.recs["meta"][-1] >> 16) == 0 else c.stream
    return c, c.recs[:n], stream, c.pairs[: len(c.pairs) - last_pairs], c.nks[:n]


def kind_pairs(recs):
    kinds = (recs["meta"] >> 16).astype(np.int64)
    return kinds[0::2], kinds[1::2]


@pytest.mark.parametrize("n_colors", [1, 64, 65, 130])
@pytest.mark.parametrize("k", [16, 31, 63])
def test_host_twin_on_hand_made_records(k, n_colors):
    c, recs, stream, pairs, nks = even_case(k)
    rng = np.random.default_rng(2500 + 7 * k + n_colors)
    bits = random_matrix(rng, len(c.unitigs), n_colors)
    ka, kb = kind_pairs(recs)
    for x in (0, 1, 2):
        for y in (0, 1, 2):
            assert ((ka == x) & (kb == y)).sum() >= 3, "no fragment of kinds (%d, %d)" % (x, y)
    both11 = (ka == 1) & (kb == 1)
    assert (both11 & (recs["u"][0::2] == recs["u"][1::2])).any() and (both11 & (recs["u"][0::2] != recs["u"][1::2])).any()
    per_read = {pm: fa.records_pseudoalign(recs, stream, k, bits, n_colors, pm) for pm in (0, 1000)}
    for pm in PERMILLES:
        anyway = frags_of(pairs, nks, bits, n_colors, pm)
        for both in (False, True):
            want = only_both(anyway) if both else anyway
            got = fa.records_pseudoalign_pairs(recs, stream, k, bits, n_colors, pm, both)
            assert_frags(got, want, "k=%d, %d colours, permille %d, both %s" % (k, n_colors, pm, both))
            one, eight = (fa.records_pseudoalign_pairs(recs, stream, k, bits, n_colors, pm, both, n_threads=t) for t in (1, 8))
            assert one[0].tobytes() == eight[0].tobytes() == got[0].tobytes() and one[1].tobytes() == eight[1].tobytes() == got[1].tobytes()
            if both:
                h = want[1]
                lone = (h["n_colored_first"] == 0) | (h["n_colored_first"] == h["n_colored"])
                assert (lone & anyway[0].any(axis=1)).any(), "FIN_PAIR_BOTH zeroes no row that FIN_PAIR_ANY gives"
                assert ((h["n_colored_first"] > 0) & (h["n_colored_first"] < h["n_colored"])).any()
    # the identities, against the per-read rows of the host function: 1000 -- the AND where both mates have coloured k-mers, else the row of the one that has; 0 -- the OR
    rows, heads = fa.records_pseudoalign_pairs(recs, stream, k, bits, n_colors, 1000)
    ra, rb = per_read[1000][0][0::2], per_read[1000][0][1::2]
    ca, cb = per_read[1000][1]["n_colored"][0::2], per_read[1000][1]["n_colored"][1::2]
    two = ((ca > 0) & (cb > 0))[:, None]
    assert np.array_equal(rows, np.where(two, ra & rb, np.where((ca > 0)[:, None], ra, rb)))
    if n_colors > 1:
        assert (two[:, 0] & ~(ra & rb).any(axis=1) & ra.any(axis=1) & rb.any(axis=1)).any(), "no fragment whose AND is empty while both mates' rows are not"
    assert np.array_equal(fa.records_pseudoalign_pairs(recs, stream, k, bits, n_colors, 0)[0], per_read[0][0][0::2] | per_read[0][0][1::2])
    assert np.array_equal(heads["n_colored_first"], ca)


def test_refusals():
    c, recs, stream, pairs, nks = even_case(31)
    nu = len(c.unitigs)
    bits = pack([[0]] * nu, 3)
    with pytest.raises(fa.FinitoError) as e:   # an odd number of reads
        fa.records_pseudoalign_pairs(c.recs, c.stream, 31, bits, 3)
    assert e.value.code == fa.FIN_EINVAL
    for mode in (2, 7, 0xFFFFFFFF):
        with pytest.raises(fa.FinitoError) as e:
            fa.records_pseudoalign_pairs(recs, stream, 31, bits, 3, mode=mode)
        assert e.value.code == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:
        fa.records_pseudoalign_pairs(recs, stream, 31, bits, 3, permille=1001)
    assert e.value.code == fa.FIN_EINVAL
    # every refusal of the unpaired twin
    for n_colors in (0, 4097):
        with pytest.raises(fa.FinitoError) as e:
            fa.records_pseudoalign_pairs(recs, stream, 31, np.zeros((nu, max(1, words_of(n_colors))), np.uint64), n_colors)
        assert e.value.code == fa.FIN_ELIMIT
    fa.records_pseudoalign_pairs(recs, stream, 31, np.zeros((nu, 64), np.uint64), 4096)
    for n_colors, stray in ((3, 3), (3, 63), (65, 65 - 64)):   # a set bit at or above n_colors, in the last word
        bad = pack([[0]] * nu, n_colors)
        bad[nu // 2, -1] |= np.uint64(1) << np.uint64(stray)
        with pytest.raises(fa.FinitoError) as e:
            fa.records_pseudoalign_pairs(recs, stream, 31, bad, n_colors)
        assert e.value.code == fa.FIN_EINVAL
    for threads in (1, 8):
        for st in (stream[:-1], np.concatenate([stream, stream[:3]])):   # a truncated stream, a stream with pairs to spare
            with pytest.raises(fa.FinitoError) as e:
                fa.records_pseudoalign_pairs(recs, st, 31, bits, 3, n_threads=threads)
            assert e.value.code == fa.FIN_EINVAL
        bad = np.array(stream); bad[len(bad) // 2] = (-2, 5)   # neither found nor (-1,-1)
        with pytest.raises(fa.FinitoError) as e:
            fa.records_pseudoalign_pairs(recs, bad, 31, bits, 3, n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
        top = int(max(stream[:, 0].max(), recs["u"].max()))
        with pytest.raises(fa.FinitoError) as e:   # a unitig number at or above n_unitigs
            fa.records_pseudoalign_pairs(recs, stream, 31, bits[:top], 3, n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
        bad = np.array(stream); bad[np.nonzero(bad[:, 0] >= 0)[0][0], 0] = nu   # ... in the stream
        with pytest.raises(fa.FinitoError) as e:
            fa.records_pseudoalign_pairs(recs, bad, 31, bits, 3, n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
        fa.records_pseudoalign_pairs(recs, stream, 31, bits[:top + 1], 3, n_threads=threads)
    rows, heads = fa.records_pseudoalign_pairs(np.zeros(0, fa.RECORD_DTYPE), np.zeros((0, 2), np.int32), 31, bits, 3)   # nothing is legal
    assert rows.shape == (0, 1) and len(heads) == 0 and heads.dtype.names == ("n_found", "n_colored", "n_colors", "n_colored_first") and heads.dtype.itemsize == 16


def test_null_and_bad_arguments_are_refused_before_any_device_call():
    L = fa.lib()
    err = C.create_string_buffer(512)
    assert L.fin_batch_pseudoalign_paired(None, None, 1000, 0, err, 512) == fa.FIN_EINVAL and b"null" in err.value
    assert L.fin_batch_device_pair_rows(None) is None and L.fin_batch_device_pair_heads(None) is None
    assert L.fin_batch_download_pair_pseudo(None, None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_batch_add_eqclasses_paired(None, None, 1000, 0, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_search_batch_pseudoalign_paired(None, None, None, 0, fa.FIN_MERGED, None, 1000, 0, None, None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_search_batch_add_eqclasses_paired(None, None, None, 0, fa.FIN_MERGED, None, 1000, 0, err, 512) == fa.FIN_EINVAL
    out = (C.c_uint64 * 4)()
    assert L.fin_records_pseudoalign_paired(None, 4, None, 0, 31, out, 1, 3, 1000, 0, out, out, 1) == fa.FIN_EINVAL
    assert L.fin_records_pseudoalign_paired(None, 0, None, 0, 31, None, 0, 3, 1000, 0, None, None, 1) == fa.FIN_OK
    assert L.fin_records_pseudoalign_paired(None, 0, None, 0, 31, None, 0, 3, 1000, 2, None, None, 1) == fa.FIN_EINVAL
    assert fa.FIN_PAIR_ANY == 0 and fa.FIN_PAIR_BOTH == 1
