"""The host twin of the colour matrix times itself (include/finito_amd.h: fin_unitig_color_shared; fin_colsim_host.cpp) against an independent
numpy model -- `shared_model`: the matrix unpacked to 0/1, M.T @ diag(v) @ M.  Up to 130 colours the product is taken in `object` dtype, Python integers, and
reduced mod 2^64; at 4096 colours it is one float64 BLAS product, exact because every sum is asserted to be below 2^53.  Weights of 2^40 push the sums past 2^32,
so 32-bit arithmetic anywhere in the twin fails.  Every comparison is exact.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import finito_amd as fa
from tests.test_color_coverage_host import matrix, special_colors
from tests.test_colors_host import pack, unpack, words_of

BIG = 2 ** 40


def shared_model(bits, n_colors, v):
    """uint64[n_colors, n_colors] by the definition"""
    member = unpack(bits, n_colors) if len(bits) else np.zeros((0, n_colors), dtype=np.int64)
    vals = [int(x) for x in v]
    if n_colors <= 130:
        m = member.astype(object)
        prod = (m * np.array(vals, dtype=object).reshape(-1, 1)).T @ m if len(vals) else np.zeros((n_colors, n_colors), dtype=object)
        return np.array([[int(x) % 2 ** 64 for x in row] for row in prod], dtype=np.uint64).reshape(n_colors, n_colors)
    assert sum(vals) < 2 ** 53, "the float64 product would round"
    m = member.astype(np.float64)
    prod = (m * np.array(vals, dtype=np.float64).reshape(-1, 1)).T @ m
    assert float(prod.max(initial=0.0)) < 2.0 ** 53
    return prod.astype(np.uint64)


def assert_shared(got, want, what):
    assert got.table.dtype == np.uint64 and got.table.shape == want.shape and got.table.tobytes() == want.tobytes(), "%s: %d entries differ" % (what, int((got.table != want).sum()))
    assert np.array_equal(got.table, got.table.T), what + ": not symmetric"
    assert np.array_equal(got.sizes, np.diagonal(want))


def weights_of(rng, n, kind):
    if kind == "nk":
        return rng.integers(0, 130, n).astype(np.uint64)   # (zeros among them: a unitig shorter than k)
    if kind == "big":
        return np.full(n, BIG, dtype=np.uint64)
    return rng.integers(0, BIG + 1, n).astype(np.uint64)


# (at 4096 colours the table is 128 MB: one shape, the one with every kind of row)
@pytest.mark.parametrize("n_colors,n_unitigs", [(c, n) for c in (1, 5, 64, 65, 130) for n in (0, 1, 65, 200)] + [(4096, 200)])
def test_twin_equals_the_model(n_colors, n_unitigs):
    rng = np.random.default_rng(3700 + 7 * n_colors + n_unitigs)
    bits = matrix(rng, n_unitigs, n_colors)
    if n_unitigs == 200:
        member = unpack(bits, n_colors)
        per_row = member.sum(axis=1)
        assert (per_row == 0).any() and (per_row == n_colors).any() and all(((per_row == 1) & (member[:, c] == 1)).any() for c in special_colors(n_colors))
    for kind in ("nk", "big", "mixed") if n_colors <= 130 else ("big",):   # (at 4096 colours a dense row is millions of pairs: one set of weights)
        v = weights_of(rng, n_unitigs, kind)
        want = shared_model(bits, n_colors, v)
        what = "%d colours, %d unitigs, %s weights" % (n_colors, n_unitigs, kind)
        if kind == "big" and n_unitigs >= 65:
            assert int(want.max()) > 2 ** 32
        first = None
        for threads in (1, 3, 0):
            got = fa.unitig_color_shared(bits, n_colors, v, n_threads=threads)
            assert_shared(got, want, "%s, %d threads" % (what, threads))
            first = first if first is not None else got.table.tobytes()
            assert got.table.tobytes() == first


def test_sums_are_mod_two_to_the_64():
    rng = np.random.default_rng(3800)
    n_colors, n = 5, 70
    bits = matrix(rng, n, n_colors)
    v = rng.integers(2 ** 62, 2 ** 63, n).astype(np.uint64)
    member = unpack(bits, n_colors)
    assert sum(int(x) for x, m in zip(v, member[:, 0]) if m) >= 2 ** 64, "nothing wraps"
    for threads in (1, 3):
        assert_shared(fa.unitig_color_shared(bits, n_colors, v, n_threads=threads), shared_model(bits, n_colors, v), "wrapping sums, %d threads" % threads)


def test_refusals():
    rng = np.random.default_rng(3900)
    n_colors, n = 70, 20
    bits = matrix(rng, n, n_colors)
    v = weights_of(rng, n, "mixed")
    for bad_nc in (0, 4097):
        with pytest.raises(fa.FinitoError) as e:
            fa.unitig_color_shared(np.zeros((n, max(1, words_of(bad_nc))), dtype=np.uint64), bad_nc, v)
        assert e.value.code == fa.FIN_ELIMIT
    L = fa.lib()
    u64p = C.POINTER(C.c_uint64)
    out = np.full(16, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    sentinel = out.tobytes()
    wide = np.zeros((n, 65), dtype=np.uint64)
    for bad_nc in (0, 4097):   # the C entry itself: refused before anything is written
        assert L.fin_unitig_color_shared(wide.ctypes.data_as(u64p), n, bad_nc, v.ctypes.data_as(u64p), out.ctypes.data_as(u64p), 1) == fa.FIN_ELIMIT
    assert L.fin_unitig_color_shared(bits.ctypes.data_as(u64p), n, n_colors, v.ctypes.data_as(u64p), None, 1) == fa.FIN_EINVAL
    assert L.fin_unitig_color_shared(None, n, n_colors, v.ctypes.data_as(u64p), out.ctypes.data_as(u64p), 1) == fa.FIN_EINVAL
    assert L.fin_unitig_color_shared(bits.ctypes.data_as(u64p), n, n_colors, None, out.ctypes.data_as(u64p), 1) == fa.FIN_EINVAL
    assert out.tobytes() == sentinel
    for u, bit in ((0, 70), (n - 1, 127), (7, 71)):   # a bit at or above n_colors, in the first, the last and a middle row
        stray = bits.copy()
        stray[u, 1] |= np.uint64(1) << np.uint64(bit - 64)
        with pytest.raises(fa.FinitoError) as e:
            fa.unitig_color_shared(stray, n_colors, v)
        assert e.value.code == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:   # weights of another length
        fa.unitig_color_shared(bits, n_colors, v[:-1])
    assert e.value.code == fa.FIN_EINVAL
    assert_shared(fa.unitig_color_shared(bits, 128, v), shared_model(bits, 128, v), "the same words under 128 colours")


def test_groups_and_containment_on_a_hand_made_matrix():
    """colours 0 and 3: equal columns; 1: a subset of 0 (and so of 3); 2: empty; 4: overlaps 0 without containing or being contained; 5 and 6: equal, apart from
    the others"""
    n_colors = 7
    sets = [[0, 3, 1], [0, 3, 1, 4], [0, 3], [0, 3, 4], [4], [5, 6], [5, 6], []]
    bits = pack(sets, n_colors)
    v = np.array([3, 5, 7, 11, 13, 17, 19, 23], dtype=np.uint64)
    s = fa.unitig_color_shared(bits, n_colors, v)
    assert_shared(s, shared_model(bits, n_colors, v), "hand-made")
    assert [int(x) for x in s.sizes] == [26, 8, 0, 26, 29, 36, 36]
    assert int(s.table[0, 4]) == 16 and int(s.table[1, 4]) == 5 and int(s.table[0, 5]) == 0
    assert s.identical_groups() == [[0, 3], [5, 6]]
    assert s.contained() == [(1, 0), (1, 3)]
    assert all(2 not in g for g in s.identical_groups()) and all(2 not in pair for pair in s.contained())
    j, c = s.jaccard, s.containment
    assert j.dtype == np.float64 and c.dtype == np.float64 and j.shape == c.shape == (7, 7)
    assert j[0, 3] == 1.0 and j[0, 1] == 8 / 26 and j[0, 4] == 16 / (26 + 29 - 16) and j[0, 5] == 0.0 and np.array_equal(j, j.T, equal_nan=True)
    assert np.isnan(j[2, 2]) and j[2, 0] == 0.0 and np.isnan(c[2]).all() and c[0, 2] == 0.0
    assert c[1, 0] == 1.0 and c[0, 1] == 8 / 26 and c[4, 0] == 16 / 29 and (np.diagonal(c)[[0, 1, 3, 4, 5, 6]] == 1.0).all()
    # three equal columns are one group; a weight of zero hides a difference, as the definition says
    s3 = fa.unitig_color_shared(pack([[0, 1, 2, 3], [0, 1, 2, 3], [3], [0]], 4), 4, np.array([2, 3, 5, 0], dtype=np.uint64))
    assert s3.identical_groups() == [[0, 1, 2]] and s3.contained() == [(0, 3), (1, 3), (2, 3)]
