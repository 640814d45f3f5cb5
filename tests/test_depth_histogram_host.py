"""Depth histograms and quantiles, the host side (include/finito_amd.h: DEPTH HISTOGRAMS AND QUANTILES; fin_depthhist_host.cpp): the twins
fa.depth_positions_histogram and fa.unitig_color_depth_histogram against a plain numpy / Python-integer model written from the definitions (np.bincount over the
counted positions of each unitig), and fa.histogram_quantile by hand.  No GPU."""
import numpy as np
import pytest

import finito_amd as fa
from tests.test_color_coverage_host import matrix
from tests.test_colors_host import unpack

TOP = 2 ** 32 - 1


def unitig_bins(depth, ends, k, n_bins, bin_width):
    """per unitig: the bincount (int64[n_bins]) of min(d // bin_width, n_bins - 1) over the positions at which a k-mer begins"""
    out = np.zeros((len(ends), n_bins), dtype=np.int64)
    start = 0
    for u, e in enumerate(ends):
        nk = max(0, int(e) - start - k + 1)
        d = np.asarray(depth[start:start + nk], dtype=np.int64)
        out[u] = np.bincount(np.minimum(d // bin_width, n_bins - 1), minlength=n_bins)
        start = int(e)
    return out


def spectrum_model(depth, ends, k, n_bins, bin_width):
    return unitig_bins(depth, ends, k, n_bins, bin_width).sum(axis=0).astype(np.uint64)


def color_model(depth, ends, k, bits, n_colors, n_bins, bin_width):
    """(table uint64[n_colors, 2, n_bins], uncolored uint64[n_bins]) by the definition"""
    V = unitig_bins(depth, ends, k, n_bins, bin_width)
    member = unpack(bits, n_colors) if len(bits) else np.zeros((0, n_colors), dtype=np.int64)
    per_row = member.sum(axis=1)
    table = np.zeros((n_colors, 2, n_bins), dtype=np.uint64)
    assert int(V.sum()) < 2 ** 53   # every sum below is then exact in float64, whose matrix product is the quick one
    Vf = V.astype(np.float64)
    table[:, 0] = (member.T.astype(np.float64) @ Vf).astype(np.uint64)
    table[:, 1] = ((member * (per_row == 1)[:, None]).T.astype(np.float64) @ Vf).astype(np.uint64)
    return table, V[per_row == 0].sum(axis=0).astype(np.uint64)


def assert_hist(got, want, what):
    table, unc = want
    assert got.table.dtype == np.uint64 and got.table.shape == table.shape and got.table.tobytes() == table.tobytes(), what + ": the table differs"
    assert got.uncolored.tobytes() == unc.tobytes(), what + ": the uncoloured histogram differs"
    assert np.array_equal(got.kmers, table[:, 0].sum(axis=1)) and np.array_equal(got.kmers_only, table[:, 1].sum(axis=1))


def edge_depths(n_bins, bin_width):
    """every depth at which the bin rule can go wrong, kept below 2^32"""
    vals = [0, bin_width - 1, bin_width, (n_bins - 1) * bin_width - 1, (n_bins - 1) * bin_width, (n_bins - 1) * bin_width + 1, TOP]
    return [v for v in vals if 0 <= v <= TOP]


def layout(rng, k, n_unitigs):
    """unitig lengths with k - 1, k and k + 1 among them (no k-mer, one, two); ends as X_ENDS"""
    lens = rng.integers(k, 3 * k, n_unitigs)
    lens[: min(3, n_unitigs)] = [k - 1, k, k + 1][: min(3, n_unitigs)]
    if n_unitigs > 5:
        lens[-1] = k - 1
    return np.cumsum(lens).astype(np.int64)


def depths(rng, total, n_bins, bin_width):
    edges = np.array(edge_depths(n_bins, bin_width), dtype=np.uint32)
    d = rng.integers(0, max(2, 2 * n_bins * bin_width), total).astype(np.uint32)
    where = rng.random(total) < 0.3
    d[where] = edges[rng.integers(0, len(edges), int(where.sum()))]
    d[: len(edges)] = edges[: total]
    return d


@pytest.mark.parametrize("bin_width", [1, 3, 1000])
@pytest.mark.parametrize("n_bins", [1, 2, 64, 1024])
def test_the_spectrum_twin_equals_the_model(n_bins, bin_width):
    rng = np.random.default_rng(5000 + n_bins + bin_width)
    k = 5
    ends = layout(rng, k, 40)
    d = depths(rng, int(ends[-1]), n_bins, bin_width)
    want = spectrum_model(d, ends, k, n_bins, bin_width)
    nk = np.maximum(0, np.diff(np.concatenate([[0], ends])) - k + 1)
    assert int(want.sum()) == int(nk.sum()) and (nk == 0).any() and (nk == 1).any() and (nk == 2).any()
    got = [fa.depth_positions_histogram(d, ends, k, n_bins, bin_width, n_threads=t) for t in (1, 3, 16)]
    assert got[0].dtype == np.uint64 and got[0].tobytes() == want.tobytes()
    assert got[1].tobytes() == got[0].tobytes() and got[2].tobytes() == got[0].tobytes()


def test_every_edge_depth_lands_in_its_bin():
    """one unitig of k-mers whose depths are exactly the edges; the last k - 1 positions carry depths that must not be counted"""
    k = 4
    for n_bins, bw in ((1, 1), (2, 1), (2, 7), (1024, 1), (1024, 3), (5, 2 ** 30)):
        e = edge_depths(n_bins, bw)
        d = np.array(e + [TOP, 1, bw][: k - 1], dtype=np.uint32)
        ends = np.array([len(d)], dtype=np.int64)
        want = np.zeros(n_bins, dtype=np.uint64)
        for v in e:
            want[min(v // bw, n_bins - 1)] += 1
        got = fa.depth_positions_histogram(d, ends, k, n_bins, bw, n_threads=1)
        assert got.tobytes() == want.tobytes() and int(got.sum()) == len(e), (n_bins, bw)


@pytest.mark.parametrize("n_colors", [1, 5, 64, 65, 130])
@pytest.mark.parametrize("n_bins,bin_width", [(1, 1), (2, 3), (65, 1), (1024, 2)])
def test_the_colour_twin_equals_the_model(n_colors, n_bins, bin_width):
    rng = np.random.default_rng(5100 + 11 * n_colors + n_bins)
    k = 5
    n = 50
    ends = layout(rng, k, n)
    d = depths(rng, int(ends[-1]), n_bins, bin_width)
    bits = matrix(rng, n, n_colors)
    want = color_model(d, ends, k, bits, n_colors, n_bins, bin_width)
    got = [fa.unitig_color_depth_histogram(d, ends, k, bits, n_colors, n_bins, bin_width, n_threads=t) for t in (1, 3, 16)]
    for g in got:
        assert_hist(g, want, "%d colours, %d bins of %d" % (n_colors, n_bins, bin_width))
        assert g.n_bins == n_bins and g.bin_width == bin_width and g.n_colors == n_colors
    # the spectrum is the single rows', the empty rows' and the several-coloured rows' histograms together
    per_row = unpack(bits, n_colors).sum(axis=1)
    V = unitig_bins(d, ends, k, n_bins, bin_width)
    total = want[1].astype(np.int64) + want[0][:, 1].sum(axis=0).astype(np.int64) + V[per_row >= 2].sum(axis=0)
    assert np.array_equal(total.astype(np.uint64), fa.depth_positions_histogram(d, ends, k, n_bins, bin_width))


def test_no_unitigs_and_no_kmers():
    z = fa.depth_positions_histogram(np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int64), 31, 7)
    assert z.shape == (7,) and not z.any()
    h = fa.unitig_color_depth_histogram(np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int64), 31, np.zeros((0, 1), dtype=np.uint64), 3, 7)
    assert h.table.shape == (3, 2, 7) and not h.table.any() and not h.uncolored.any()
    assert np.array_equal(h.median()[0], [-1, -1, -1]) and np.isnan(h.breadth()).all() and np.array_equal(h.iqr()[0], [-1, -1, -1])
    short = fa.depth_positions_histogram(np.full(9, 5, dtype=np.uint32), np.array([4, 9]), 6, 8)   # both unitigs shorter than k
    assert not short.any()


def test_refusals():
    rng = np.random.default_rng(5200)
    k, n, n_colors = 5, 12, 70
    ends = layout(rng, k, n)
    d = depths(rng, int(ends[-1]), 16, 1)
    bits = matrix(rng, n, n_colors)
    stray = bits.copy()
    stray[n - 1, 1] |= np.uint64(1) << np.uint64(n_colors & 63)
    with pytest.raises(fa.FinitoError) as e:
        fa.unitig_color_depth_histogram(d, ends, k, stray, n_colors, 16)
    assert e.value.code == fa.FIN_EINVAL
    for bad in (0, 4097):
        with pytest.raises(fa.FinitoError) as e:
            fa.unitig_color_depth_histogram(d, ends, k, bits, bad, 16)
        assert e.value.code == fa.FIN_ELIMIT
    L = fa.lib()
    vp = lambda a: a.ctypes.data
    out = np.full((n_colors * 2 + 1) * 16, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    sentinel = out.tobytes()
    e64 = ends.astype(np.int64)
    assert L.fin_unitig_color_depth_histogram(vp(d), vp(e64), n, k, vp(bits), 0, 16, 1, vp(out), None, 1) == fa.FIN_ELIMIT
    assert L.fin_unitig_color_depth_histogram(vp(d), vp(e64), n, k, vp(bits), 4097, 16, 1, vp(out), None, 1) == fa.FIN_ELIMIT
    assert L.fin_unitig_color_depth_histogram(vp(d), vp(e64), n, k, vp(stray), n_colors, 16, 1, vp(out), None, 1) == fa.FIN_EINVAL
    for n_bins, bw in ((0, 1), (1025, 1), (16, 0)):
        assert L.fin_unitig_color_depth_histogram(vp(d), vp(e64), n, k, vp(bits), n_colors, n_bins, bw, vp(out), None, 1) == fa.FIN_EINVAL
        assert L.fin_depth_positions_histogram(vp(d), vp(e64), n, k, n_bins, bw, vp(out), 1) == fa.FIN_EINVAL
    assert L.fin_depth_positions_histogram(vp(d), vp(e64), n, k, 16, 1, None, 1) == fa.FIN_EINVAL
    assert L.fin_depth_positions_histogram(vp(d), vp(e64[::-1].copy()), n, k, 16, 1, vp(out), 1) == fa.FIN_EINVAL   # ends that decrease
    assert out.tobytes() == sentinel   # (a refusal writes nothing)
    assert L.fin_unitig_color_depth_histogram(vp(d), vp(e64), n, k, vp(bits), n_colors, 16, 1, vp(out), None, 2) == fa.FIN_OK   # (uncolored may be NULL)
    assert out[: n_colors * 32].tobytes() == color_model(d, ends, k, bits, n_colors, 16, 1)[0].tobytes() and out[n_colors * 32:].tobytes() == sentinel[-128:]
    for n_bins, bw in ((0, 1), (1025, 1), (16, 0)):
        with pytest.raises(fa.FinitoError) as e:
            fa.depth_positions_histogram(d, ends, k, n_bins, bw)
        assert e.value.code == fa.FIN_EINVAL


def test_histogram_quantile_by_hand():
    h = [3, 0, 1]   # N = 4: t = 1, 1, 2, 4, 4
    assert [fa.histogram_quantile(h, p) for p in (0, 1, 500, 999, 1000)] == [(0, False), (0, False), (0, False), (2, True), (2, True)]
    assert fa.histogram_quantile(h, 750) == (0, False) and fa.histogram_quantile(h, 751) == (2, True)   # t = 3, then ceil(3.004) = 4
    assert fa.histogram_quantile(h, 1000, bin_width=5) == (10, True) and fa.histogram_quantile(h, 0, bin_width=5) == (0, False)
    # a single non-empty bin answers every p; it is saturated only as the last of several
    for p in (0, 1, 500, 1000):
        assert fa.histogram_quantile([0, 0, 9, 0], p, 3) == (6, False)
        assert fa.histogram_quantile([0, 0, 0, 9], p, 3) == (9, True)
        assert fa.histogram_quantile([9], p, 3) == (0, False)   # one bin: nothing to saturate against
    assert fa.histogram_quantile([0, 0, 0], 500) is None and fa.histogram_quantile([], 500) is None
    # p * N passes 2^53: floats would round the threshold
    big = 2 ** 62
    h = [big, 1, big - 1]   # N = 2^63: the median's t is 2^62 exactly, one more falls into bin 1, two more into bin 2
    assert fa.histogram_quantile(h, 500) == (0, False)
    assert fa.histogram_quantile([big - 1, 1, big], 500) == (1, False)
    assert fa.histogram_quantile([big - 2, 1, big + 1], 500) == (2, True)
    assert fa.histogram_quantile(np.array([2 ** 63, 2 ** 63], dtype=np.uint64), 501) == (1, True)   # (uint64 entries whose sum passes 2^64 in numpy)
    for bad in (-1, 1001):
        with pytest.raises(fa.FinitoError):
            fa.histogram_quantile([1], bad)


def test_quantiles_of_a_table():
    table = np.zeros((3, 2, 4), dtype=np.uint64)
    table[0, 0] = [1, 1, 1, 1]; table[0, 1] = [0, 4, 0, 0]
    table[2, 0] = [0, 0, 0, 8]
    h = fa.ColorDepthHistogram(table, np.zeros(4, dtype=np.uint64), 10)
    assert np.array_equal(h.kmers, [4, 0, 8]) and np.array_equal(h.kmers_only, [4, 0, 0])
    v, s = h.median()
    assert np.array_equal(v, [10, -1, 30]) and np.array_equal(s, [False, False, True])
    v, s = h.quantile(1000)
    assert np.array_equal(v, [30, -1, 30]) and np.array_equal(s, [True, False, True])
    v, s = h.median(only=True)
    assert np.array_equal(v, [10, -1, -1]) and not s.any()
    v, s = h.iqr()
    assert np.array_equal(v, [20, -1, 0]) and np.array_equal(s, [False, False, True])
    b = h.breadth()
    assert b[0] == 0.75 and np.isnan(b[1]) and b[2] == 1.0 and np.isnan(h.breadth(only=True)[2])
