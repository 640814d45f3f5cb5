"""The host twin of the colour coverage projection (include/finito_amd.h: fin_unitig_color_coverage; fin_colcov_host.cpp) against an independent
numpy model -- `coverage_model`: the matrix unpacked to booleans, B.T @ v, and the _only sums over the rows with exactly one bit.  The model's sums are made in
Python integers: every value is cut into limbs of 21 bits, the limbs' column sums are one int64 matrix product that cannot overflow (asserted: rows * 2^21 < 2^63),
and the limbs are put together again as Python integers; on the small shapes the same product is also taken in `object` dtype outright and must agree.  Values go
up to 2^40 + 3, so 32-bit arithmetic anywhere in the twin fails.  Every comparison is exact.  No GPU."""
import numpy as np
import pytest

import finito_amd as fa
from tests.test_colors_host import pack, pack_members, unpack, words_of

FIELDS = ("kmers", "covered", "depth_sum", "solid")
BIG = 2 ** 40 + 3


def column_sums(member, vs):
    """member.T @ v in Python integers for every v of vs: member 0/1 int64 [n, n_colors], v a list of n Python integers below 2^63; object arrays [n_colors]"""
    n = member.shape[0]
    assert n * 2 ** 21 < 2 ** 63 and all(0 <= x < 2 ** 63 for v in vs for x in v)
    limbs = np.array([[(x >> (21 * limb)) & (2 ** 21 - 1) for x in row for limb in range(3)] for row in zip(*vs)], dtype=np.int64).reshape(n, 3 * len(vs))
    prod = (member.T @ limbs).astype(object)   # (one product for all limbs of all values; no entry can pass n * 2^21)
    return [prod[:, 3 * i] + prod[:, 3 * i + 1] * (1 << 21) + prod[:, 3 * i + 2] * (1 << 42) for i in range(len(vs))]


def coverage_model(bits, n_colors, nk, covered=None, stats=None, cross_check=False):
    """(COLOR_COVERAGE_DTYPE table[n_colors], the dict of the uncoloured unitigs' four sums) by the definition; what is absent is zero"""
    member = unpack(bits, n_colors) if len(bits) else np.zeros((0, n_colors), dtype=np.int64)
    n = len(member)
    per_row = member.sum(axis=1)
    single = member * (per_row == 1)[:, None]
    vals = {"kmers": [int(x) for x in nk]}
    if covered is not None:
        vals["covered"] = [int(x) for x in covered]
    if stats is not None:
        vals["depth_sum"], vals["solid"] = [int(x) for x in stats["sum"]], [int(x) for x in stats["n_at_least"]]
    table = np.zeros(n_colors, dtype=fa.COLOR_COVERAGE_DTYPE)
    unc = {f: 0 for f in FIELDS}
    names = list(vals)
    for f, both, only in zip(names, column_sums(member, [vals[f] for f in names]), column_sums(single, [vals[f] for f in names])):
        if cross_check:
            v = np.array(vals[f], dtype=object).reshape(n)
            assert list(member.T.astype(object) @ v) == list(both) and list(single.T.astype(object) @ v) == list(only)
        assert all(int(x) < 2 ** 64 for x in both)
        table[f] = [int(x) for x in both]
        table[f + "_only"] = [int(x) for x in only]
        unc[f] = sum(x for x, pc in zip(vals[f], per_row) if pc == 0)
    return table, unc


def without(want, fields):
    """the model's result with the sums of `fields` zeroed: what the definition gives when their accumulator is absent"""
    table, unc = want[0].copy(), dict(want[1])
    for f in fields:
        table[f] = 0; table[f + "_only"] = 0; unc[f] = 0
    return table, unc


def assert_coverage(got, want, what):
    table, unc = want
    assert got.table.dtype == fa.COLOR_COVERAGE_DTYPE and got.table.tobytes() == table.tobytes(), "%s: the table differs in %s" % (
        what, [f for f in table.dtype.names if not np.array_equal(got.table[f], table[f])])
    assert got.uncolored == unc, "%s: the uncoloured entry %s, the model %s" % (what, got.uncolored, unc)
    for f in table.dtype.names:
        assert np.array_equal(getattr(got, f), table[f])


def special_colors(n_colors):
    return sorted({c for c in (0, 63, 64, n_colors - 1) if c < n_colors})


def matrix(rng, n_unitigs, n_colors):
    """random rows (empty, single, several, dense, full), and behind them by hand: an empty row, a full row, every special colour alone and all of them
    together -- as far as there are rows"""
    member = np.zeros((n_unitigs, n_colors), dtype=np.int64)
    how = rng.integers(0, 5, n_unitigs)
    for u in range(n_unitigs):
        if how[u] == 1:
            member[u, int(rng.integers(0, n_colors))] = 1
        elif how[u] == 2:
            member[u, rng.choice(n_colors, size=min(n_colors, int(rng.integers(2, 9))), replace=False)] = 1
        elif how[u] == 3:
            member[u] = rng.random(n_colors) < 0.6
        elif how[u] == 4:
            member[u] = 1
    bits = pack_members(member) if n_unitigs else np.zeros((0, words_of(n_colors)), dtype=np.uint64)
    sp = special_colors(n_colors)
    hand = [[], list(range(n_colors))] + [[c] for c in sp] + [sp]
    for u, cs in zip(range(n_unitigs - 1, -1, -1), hand):
        bits[u] = pack([cs], n_colors)[0]
    return bits


def values(rng, n):
    """nk up to 2^40 + 3 with the bound itself among them, covered <= nk, stats with sum up to 2^40 + 3"""
    nk = rng.integers(0, BIG + 1, n).astype(np.uint64)
    if n:
        nk[rng.integers(0, n)] = BIG
    covered = (nk * rng.random(n)).astype(np.uint64)
    covered[rng.random(n) < 0.2] = 0
    assert (covered <= nk).all()
    stats = np.zeros(n, dtype=fa.DEPTH_STAT_DTYPE)
    stats["sum"] = rng.integers(0, BIG + 1, n)
    stats["max"] = rng.integers(0, 2 ** 32, n)
    stats["n_at_least"] = rng.integers(0, 2 ** 32, n)
    if n:
        stats["sum"][rng.integers(0, n)] = BIG
        stats["n_at_least"][rng.integers(0, n)] = 2 ** 32 - 1
    return nk, covered, stats


@pytest.mark.parametrize("n_unitigs", [0, 1, 63, 64, 65, 257, 3000])
@pytest.mark.parametrize("n_colors", [1, 63, 64, 65, 130, 4079])
def test_twin_equals_the_model(n_colors, n_unitigs):
    rng = np.random.default_rng(3400 + 7 * n_colors + n_unitigs)
    bits = matrix(rng, n_unitigs, n_colors)
    nk, covered, stats = values(rng, n_unitigs)
    small = n_unitigs <= 257 and n_colors <= 130
    what = "%d colours, %d unitigs" % (n_colors, n_unitigs)
    full = coverage_model(bits, n_colors, nk, covered, stats, cross_check=small)
    for cov, st in ((covered, stats), (covered, None), (None, stats), (None, None)):
        want = without(full, ([] if cov is not None else ["covered"]) + ([] if st is not None else ["depth_sum", "solid"]))   # (what is absent is zero)
        if small:
            lone = coverage_model(bits, n_colors, nk, cov, st)
            assert lone[0].tobytes() == want[0].tobytes() and lone[1] == want[1]
        if n_unitigs >= 257:
            assert int(want[0]["kmers"].max()) > 2 ** 32 and (st is None or int(want[0]["depth_sum"].max()) > 2 ** 32)
        for threads in (1, 3) if cov is not None else (5,):
            got = fa.unitig_color_coverage(bits, n_colors, nk, cov, st, n_threads=threads)
            assert_coverage(got, want, "%s, covered %s, stats %s, %d threads" % (what, cov is not None, st is not None, threads))
        if cov is None:
            assert not want[0]["covered"].any() and not want[0]["covered_only"].any() and want[1]["covered"] == 0
        if st is None:
            assert not want[0]["depth_sum"].any() and not want[0]["solid_only"].any() and want[1]["solid"] == 0


@pytest.mark.parametrize("n_colors", [1, 65, 4079])
def test_the_identities_of_the_definition(n_colors):
    """covered[c] <= kmers[c]; solid == covered where every unitig's n_at_least is its covered count (bitmap and depth of the same runs at min_depth 1); the
    k-mers of the single rows, of the empty rows and of the rows with two or more colours are all the k-mers; the derived ratios"""
    rng = np.random.default_rng(3500 + n_colors)
    n = 300
    bits = matrix(rng, n, n_colors)
    nk = rng.integers(1, 2 ** 31, n).astype(np.uint64)
    covered = (nk * rng.random(n)).astype(np.uint64)
    stats = np.zeros(n, dtype=fa.DEPTH_STAT_DTYPE)
    stats["n_at_least"] = covered
    stats["sum"] = covered * np.uint64(3)
    got = fa.unitig_color_coverage(bits, n_colors, nk, covered, stats)
    assert_coverage(got, coverage_model(bits, n_colors, nk, covered, stats), "%d colours" % n_colors)
    assert (got.covered <= got.kmers).all() and (got.covered_only <= got.kmers_only).all() and (got.kmers_only <= got.kmers).all()
    assert np.array_equal(got.solid, got.covered) and np.array_equal(got.solid_only, got.covered_only) and got.uncolored["solid"] == got.uncolored["covered"]
    per_row = unpack(bits, n_colors).sum(axis=1)
    multi = sum(int(x) for x in nk[per_row >= 2])
    assert sum(int(x) for x in got.kmers_only) + got.uncolored["kmers"] + multi == sum(int(x) for x in nk)
    assert (per_row == 0).any() and (per_row == 1).any() and (n_colors == 1 or (per_row >= 2).any())
    for ratio, num, den in ((got.breadth, got.covered, got.kmers), (got.breadth_only, got.covered_only, got.kmers_only), (got.mean_depth, got.depth_sum, got.covered)):
        assert ratio.dtype == np.float64 and len(ratio) == n_colors
        for c in range(n_colors):
            assert np.isnan(ratio[c]) if den[c] == 0 else ratio[c] == float(num[c]) / float(den[c])
    assert n_colors < 4079 or np.isnan(got.breadth_only).any()   # (300 rows cannot hold 4079 single colours: a reference without a unitig of its own)


def test_refusals():
    rng = np.random.default_rng(3600)
    n_colors, n = 70, 20
    bits = matrix(rng, n, n_colors)
    nk, covered, stats = values(rng, n)
    for bad_nc in (0, 4097):
        with pytest.raises(fa.FinitoError) as e:
            fa.unitig_color_coverage(np.zeros((n, max(1, words_of(bad_nc))), dtype=np.uint64), bad_nc, nk)
        assert e.value.code == fa.FIN_ELIMIT
    L = fa.lib()
    out = np.zeros(4097, dtype=fa.COLOR_COVERAGE_DTYPE)
    import ctypes as C
    u64p = C.POINTER(C.c_uint64)
    wide = np.zeros((n, 65), dtype=np.uint64)
    for bad_nc in (0, 4097):   # the C entry itself
        assert L.fin_unitig_color_coverage(wide.ctypes.data_as(u64p), n, bad_nc, nk.ctypes.data_as(u64p), None, None, out.ctypes.data_as(C.c_void_p), None, 1) == fa.FIN_ELIMIT
    for u, bit in ((0, 70), (n - 1, 127), (7, 71)):   # a bit at or above n_colors, in the first, the last and a middle row
        stray = bits.copy()
        stray[u, 1] |= np.uint64(1) << np.uint64(bit - 64)
        with pytest.raises(fa.FinitoError) as e:
            fa.unitig_color_coverage(stray, n_colors, nk, covered, stats)
        assert e.value.code == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:   # a per-unitig array of another length
        fa.unitig_color_coverage(bits, n_colors, nk[:-1])
    assert e.value.code == fa.FIN_EINVAL
    assert fa.unitig_color_coverage(bits, 128, nk).table.tobytes() == coverage_model(bits, 128, nk)[0].tobytes()   # (the same words are legal under 128 colours)
