"""Depth histograms per index and per reference, on the device (include/finito_amd.h: fin_depth_histogram, fin_colors_depth_histogram; fin_depthhist.hip; DESIGN.md
4.26).  The device is held against the host twins (fa.depth_positions_histogram, fa.unitig_color_depth_histogram) and against the numpy model of
tests/test_depth_histogram_host.py, byte for byte; what goes into twin and model are the accumulators' own downloads -- Depth.download()'s positions,
Colors.download(), the exported ends --, never a result of the call under test."""
import ctypes as C

import numpy as np
import pytest

import finito_amd as fa
from tests.test_color_coverage import hand_made, hip_runtime, nk_of
from tests.test_color_coverage_host import matrix
from tests.test_colors_host import pack, unpack
from tests.test_depth_histogram_host import TOP, assert_hist, color_model, edge_depths, spectrum_model
from tests.test_eqclasses import N_COLORS_OF_W, small   # noqa: F401 (the fixture: the suite's small index)
from tests.util import cut_unitigs, random_genome, sample_reads

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A5A5A5A5A
TILE_CHUNK = 64 * 64   # positions per chunk of the prefix sum under debug_depth_tile = 64
BINNINGS = [(n_bins, bw) for n_bins in (1, 2, 64, 65, 1024) for bw in (1, 3)]


@pytest.fixture(scope="module")
def filled(small):   # noqa: F811
    """the small index with a depth filled by overlapping reads, its download, and a cache of the expectations every case of the grid shares"""
    p, g, rng = small
    dep = p.depth().add_reads(sample_reads(rng, g, 300, 100, err=0.01))
    positions, stats, _ = dep.download(1)
    assert int(stats["max"].max()) >= 3 and (positions == 0).any(), "no position found three times, or none left out"
    yield p, g, dep, positions.copy(), p.export(fa.X_ENDS), {}
    dep.close()


class Options:
    def __init__(self, p, **kw):
        self.p, self.kw = p, kw

    def __enter__(self):
        for name, v in self.kw.items():
            self.p.set_option(name, v)

    def __exit__(self, *a):
        for name in self.kw:
            self.p.set_option(name, None)


def unitigs_per_chunk(ends, chunk):
    """how many unitigs have a position in each chunk of `chunk` positions"""
    starts = np.concatenate([[0], ends[:-1]])
    return [int(((starts < b + chunk) & (ends > b)).sum()) for b in range(0, int(ends[-1]), chunk)]


@pytest.mark.parametrize("tile", [None, 64])
@pytest.mark.parametrize("sub", [0, 16])
@pytest.mark.parametrize("W", [1, 2, 3, 64])
def test_device_equals_twin_equals_model(filled, W, sub, tile):
    p, _, dep, positions, ends, cache = filled
    n_colors = N_COLORS_OF_W[W]
    # the seams the case is about are really there: several chunks with a partial last one, several sub-ranges per chunk with a partial last one, unitigs astride both
    assert p.n_unitigs >= 200 and p.n_unitigs % 64 and p.n_unitigs % 16
    if tile:
        per_chunk = unitigs_per_chunk(ends, TILE_CHUNK)
        assert p.total_len > 2 * TILE_CHUNK and p.total_len % TILE_CHUNK and sum(per_chunk) > p.n_unitigs, "one chunk, or no unitig astride a chunk seam"
        assert not sub or (min(per_chunk[:-1]) > 3 * sub and any(n % sub for n in per_chunk))
    col = p.colors(n_colors, hand_made(np.random.default_rng(4100 + W), p.n_unitigs, n_colors))
    bits = col.download()[0]
    before = dep.download(2), bits.tobytes()
    try:
        with Options(p, depthhist_unitigs=sub, debug_depth_tile=tile):
            for n_bins, bw in BINNINGS:
                what = "W=%d, sub-ranges of %d, tile %s, %d bins of %d" % (W, sub, tile, n_bins, bw)
                if (W, n_bins, bw) not in cache:
                    twin = fa.unitig_color_depth_histogram(positions, ends, p.k, bits, n_colors, n_bins, bw, n_threads=3)
                    want = color_model(positions, ends, p.k, bits, n_colors, n_bins, bw)
                    assert_hist(twin, want, what + " (the twin)")
                    s_twin, s_want = fa.depth_positions_histogram(positions, ends, p.k, n_bins, bw, n_threads=3), spectrum_model(positions, ends, p.k, n_bins, bw)
                    assert s_twin.tobytes() == s_want.tobytes()
                    cache[(W, n_bins, bw)] = want, s_want
                want, s_want = cache[(W, n_bins, bw)]
                got = col.depth_histogram(dep, n_bins, bw)
                assert_hist(got, want, what)
                assert got.n_bins == n_bins and got.bin_width == bw
                hist = dep.histogram(n_bins, bw)
                assert hist.dtype == np.uint64 and hist.tobytes() == s_want.tobytes(), what + ": the spectrum differs"
                assert int(hist.sum()) == int(nk_of(p).sum())
            again = col.depth_histogram(dep, 65, 3)
            assert_hist(again, cache[(W, 65, 3)][0], "the second call")
    finally:
        after = dep.download(2), col.download()[0].tobytes()
        col.close()
    assert before[0][0].tobytes() == after[0][0].tobytes() and before[0][1].tobytes() == after[0][1].tobytes() and before[0][2] == after[0][2], "the call changed the depth"
    assert before[1] == after[1], "the call changed the colours"


@pytest.mark.parametrize("T", [1, 2])
def test_the_identities_against_coverage(filled, T):
    """bin_width 1 and n_bins above the greatest depth: the histograms' moments are Colors.coverage's sums of the same objects"""
    p, _, dep, positions, ends, _ = filled
    n_colors = 100
    col = p.colors(n_colors, hand_made(np.random.default_rng(4500), p.n_unitigs, n_colors))
    n_bins = int(positions.max()) + 2
    assert n_bins <= 1024
    b = np.arange(n_bins, dtype=np.uint64)
    try:
        with Options(p, depthhist_unitigs=16, debug_depth_tile=64):
            cc = col.coverage(None, dep, T)
            h = col.depth_histogram(dep, n_bins, 1)
            hist = dep.histogram(n_bins, 1)
        for j, suffix in ((0, ""), (1, "_only")):
            t = h.table[:, j]
            assert np.array_equal(t.sum(axis=1), getattr(cc, "kmers" + suffix)) and np.array_equal((t * b).sum(axis=1), getattr(cc, "depth_sum" + suffix))
            assert np.array_equal(t[:, T:].sum(axis=1), getattr(cc, "solid" + suffix))
        assert np.array_equal(h.kmers, cc.kmers) and np.array_equal(h.kmers_only, cc.kmers_only) and cc.depth_sum.any() and cc.solid_only.any()
        unc = h.uncolored
        assert int(unc.sum()) == cc.uncolored["kmers"] > 0 and int((unc * b).sum()) == cc.uncolored["depth_sum"] and int(unc[T:].sum()) == cc.uncolored["solid"]
        # the whole-index sum: the single rows, the empty rows and the rows of two or more colours
        per_row = unpack(col.download()[0], n_colors).sum(axis=1)
        several = np.where(per_row >= 2)[0]
        starts = np.concatenate([[0], ends[:-1]])
        rest = np.zeros(n_bins, dtype=np.uint64)
        for u in several:
            rest += np.bincount(positions[starts[u]: starts[u] + max(0, int(ends[u] - starts[u]) - p.k + 1)], minlength=n_bins).astype(np.uint64)
        assert np.array_equal(hist, unc + h.table[:, 1].sum(axis=0) + rest) and hist[0] > 0 and hist[2:].any()
        # quantiles: the median of a reference against the sorted depths of its k-mer positions
        member = unpack(col.download()[0], n_colors)
        med, sat = h.median()
        for c in (0, 63, 64, n_colors - 1):
            ds = np.sort(np.concatenate([positions[starts[u]: starts[u] + max(0, int(ends[u] - starts[u]) - p.k + 1)] for u in np.where(member[:, c])[0]]))
            assert len(ds) == int(h.kmers[c]) and med[c] == int(ds[max(1, -(-500 * len(ds) // 1000)) - 1]) and not sat[c]
        with np.errstate(invalid="ignore", divide="ignore"):
            assert np.array_equal(h.breadth(), 1 - h.table[:, 0, 0] / h.kmers, equal_nan=True)
    finally:
        col.close()


def plant(dep, depth):
    """writes the difference array of `depth` (uint32[total_len]) to the accumulator's HBM through the HIP runtime: the counterpart of
    tests/test_unitig_depth.py::device_int32"""
    d = np.asarray(depth, dtype=np.uint32)
    diff = np.zeros(len(d) + 1, dtype=np.uint32)
    diff[0] = d[0]
    diff[1:-1] = d[1:] - d[:-1]   # (modulo 2^32)
    diff[-1] = (0 - int(d[-1])) & 0xFFFFFFFF
    hip = hip_runtime()
    assert hip.hipDeviceSynchronize() == 0 and hip.hipMemcpy(C.c_void_p(dep.device_ptr()), diff.view(np.int32).ctypes.data_as(C.c_void_p), diff.nbytes, 1) == 0   # 1 = hipMemcpyHostToDevice


PLANT_BINNINGS = [(256, 1), (64, 3), (1024, 1), (2, 5), (1, 1), (1024, 2 ** 22)]


def test_planted_depths(small):   # noqa: F811
    p, g, rng = small
    k = p.k
    ends = p.export(fa.X_ENDS)
    starts = np.concatenate([[0], ends[:-1]])
    nk = nk_of(p).astype(np.int64)
    depth = np.zeros(p.total_len, dtype=np.uint32)
    with np.errstate(over="ignore"):
        depth[0:512] = 5                                              # 64 consecutive lanes' worth of positions (8 each) in one bin ...
        depth[512:1024] = np.repeat(np.arange(64, dtype=np.uint32) + 10, 8)   # ... and in 64 different bins, a bin per lane
    first = int(np.searchsorted(starts, 1024))   # the first unitig that begins behind them
    roomy = [u for u in range(first, p.n_unitigs) if nk[u] >= 12]
    one_run, no_runs, tail, edges_u = roomy[0], roomy[1], roomy[2], roomy[3:]
    depth[starts[one_run]: ends[one_run]] = 7                         # one run -- and the value stands over the last k - 1 positions too
    depth[starts[no_runs]: ends[no_runs]] = np.arange(ends[no_runs] - starts[no_runs], dtype=np.uint32) * 3 + 1   # a new value at every position
    depth[starts[tail] + nk[tail]: ends[tail]] = TOP                  # the last k - 1 positions alone: nothing of it may be counted
    edge_vals = sorted({v for n_bins, bw in PLANT_BINNINGS for v in edge_depths(n_bins, bw)})
    assert TOP in edge_vals and 0 in edge_vals
    at = 0
    for u in edges_u:                                                 # every bin edge, one position each, on counted positions
        take = edge_vals[at: at + int(nk[u])]
        depth[starts[u]: starts[u] + len(take)] = take
        at += len(take)
        if at >= len(edge_vals):
            break
    assert at >= len(edge_vals)
    n_colors = 70
    sets = [[int(c) for c in np.where(r)[0] if c not in (3, 69)] for r in unpack(matrix(rng, p.n_unitigs, n_colors), n_colors)]   # (3 and 69 are the planted unitigs' alone)
    sets[one_run], sets[no_runs], sets[tail] = [3], [3, 69], [69]
    bits = pack(sets, n_colors)
    col, dep = p.colors(n_colors, bits), p.depth()
    try:
        plant(dep, depth)
        assert np.array_equal(dep.download()[0], depth), "the planted depths are not what the download sees"
        for sub, tile in ((0, None), (16, 64)):
            with Options(p, depthhist_unitigs=sub, debug_depth_tile=tile):
                for n_bins, bw in PLANT_BINNINGS:
                    what = "planted, %d bins of %d, sub-ranges of %d, tile %s" % (n_bins, bw, sub, tile)
                    hist = dep.histogram(n_bins, bw)
                    assert hist.tobytes() == spectrum_model(depth, ends, k, n_bins, bw).tobytes(), what
                    assert int(hist.sum()) == int(nk.sum()), what + ": positions where no k-mer begins were counted, or counted ones dropped"
                    assert_hist(col.depth_histogram(dep, n_bins, bw), color_model(depth, ends, k, bits, n_colors, n_bins, bw), what)
                h = col.depth_histogram(dep, 1024, 1)
                only69 = h.table[69, 1]
                assert int(only69.sum()) == nk[tail] == int(only69[0]), "the depth over a unitig's last k - 1 positions was counted"
                assert int(h.table[3, 1, 7]) == nk[one_run] == int(h.kmers_only[3])
                assert int((h.table[3, 0] > 0).sum()) >= nk[no_runs]
                assert int(dep.histogram(1024, 1)[1023]) >= 1 and int(dep.histogram(2, 5)[1]) > 64   # 2^32 - 1 saturates into the last bin; so do the 64 bins of the lanes
        # nothing but the last k - 1 positions of every unitig holds depth: every counted position is in bin 0
        depth[:] = 0
        for u in range(p.n_unitigs):
            depth[starts[u] + max(0, nk[u]): ends[u]] = 9
        plant(dep, depth)
        hist = dep.histogram(16, 1)
        assert int(hist[0]) == int(nk.sum()) and not hist[1:].any()
        h = col.depth_histogram(dep, 16, 1)
        assert not h.table[:, :, 1:].any() and not h.uncolored[1:].any() and np.array_equal(h.table[:, 0, 0], h.kmers) and h.kmers.any()
    finally:
        dep.reset()
        dep.close(); col.close()


def raw_hist(dep, n_bins, bw, out):
    err = C.create_string_buffer(512)
    rc_ = fa.lib().fin_depth_histogram(dep.h if dep is not None else None, n_bins, bw, out.ctypes.data_as(C.c_void_p) if out is not None else None, err, 512)
    return rc_, err.value.decode()


def raw_color_hist(col, dep, n_bins, bw, out, unc):
    err = C.create_string_buffer(512)
    rc_ = fa.lib().fin_colors_depth_histogram(col.h if col is not None else None, dep.h if dep is not None else None, n_bins, bw,
                                              out.ctypes.data_as(C.c_void_p) if out is not None else None, unc.ctypes.data_as(C.c_void_p) if unc is not None else None, err, 512)
    return rc_, err.value.decode()


@pytest.mark.parametrize("n_bins", [1, 1024])
@pytest.mark.parametrize("n_colors", [1, 65])
def test_buffers_of_exactly_the_stated_size(filled, n_colors, n_bins):
    """the C ABI through ctypes: sentinels behind hist_out, out and uncolored stay; more adds and an upload between two calls show in the second"""
    p, g, _, _, ends, _ = filled
    rng = np.random.default_rng(4600 + n_colors + n_bins)
    col, dep = p.colors(n_colors, matrix(rng, p.n_unitigs, n_colors)), p.depth()
    cells = n_colors * 2 * n_bins
    hist, out, unc = (np.full(n + 4, SENT, dtype=np.uint64) for n in (n_bins, cells, n_bins))
    try:
        for step in range(2):
            if step:
                dep.add_reads(sample_reads(rng, g, 80, 90, err=0.0))
                col.upload(matrix(rng, p.n_unitigs, n_colors))
            positions, bits = dep.download()[0], col.download()[0]
            assert raw_hist(dep, n_bins, 2, hist)[0] == fa.FIN_OK and raw_color_hist(col, dep, n_bins, 2, out, unc)[0] == fa.FIN_OK
            want = color_model(positions, ends, p.k, bits, n_colors, n_bins, 2)
            assert hist[:n_bins].tobytes() == spectrum_model(positions, ends, p.k, n_bins, 2).tobytes() and (hist[n_bins:] == SENT).all()
            assert out[:cells].tobytes() == want[0].tobytes() and (out[cells:] == SENT).all()
            assert unc[:n_bins].tobytes() == want[1].tobytes() and (unc[n_bins:] == SENT).all()
            assert step == 0 or (positions.any() and (n_bins == 1 or hist[1:n_bins].any()))
            keep = out.copy()
            assert raw_color_hist(col, dep, n_bins, 2, out, None)[0] == fa.FIN_OK and out.tobytes() == keep.tobytes()   # (uncolored may be NULL; a second call gives the same bytes)
    finally:
        dep.close(); col.close()


def test_refusals(small):   # noqa: F811
    p, g, rng = small
    k = 31
    rng = np.random.default_rng(4700)
    other = fa.FinimizerIndex.build(cut_unitigs(rng, random_genome(rng, 3000), k, max_len=80), k).to_device(0)
    col, dep, dep_o = p.colors(5, matrix(rng, p.n_unitigs, 5)), p.depth(), other.depth()
    out, unc, hist = (np.full(n, SENT, dtype=np.uint64) for n in (5 * 2 * 8, 8, 8))
    try:
        for n_bins, bw, word in ((0, 1, "n_bins"), (1025, 1, "n_bins"), (8, 0, "bin_width")):
            rc_, msg = raw_hist(dep, n_bins, bw, hist)
            assert rc_ == fa.FIN_EINVAL and word in msg
            rc_, msg = raw_color_hist(col, dep, n_bins, bw, out, unc)
            assert rc_ == fa.FIN_EINVAL and word in msg
            for call in (lambda: dep.histogram(n_bins, bw), lambda: col.depth_histogram(dep, n_bins, bw)):
                with pytest.raises(fa.FinitoError) as e:
                    call()
                assert e.value.code == fa.FIN_EINVAL
        for args in ((None, 8, 1, hist), (dep, 8, 1, None)):
            rc_, msg = raw_hist(*args)
            assert rc_ == fa.FIN_EINVAL and "null" in msg
        for args in ((None, dep, 8, 1, out, unc), (col, None, 8, 1, out, unc), (col, dep, 8, 1, None, unc)):
            rc_, msg = raw_color_hist(*args)
            assert rc_ == fa.FIN_EINVAL and "null" in msg
        rc_, msg = raw_color_hist(col, dep_o, 8, 1, out, unc)
        assert rc_ == fa.FIN_EINVAL and "depth accumulator" in msg and "different indexes or devices" in msg
        with pytest.raises(fa.FinitoError) as e:
            col.depth_histogram(dep_o, 8)
        assert e.value.code == fa.FIN_EINVAL
        col.compact()
        rc_, msg = raw_color_hist(col, dep, 8, 1, out, unc)
        assert rc_ == fa.FIN_EINVAL and "fin_colors_expand" in msg
        with pytest.raises(fa.FinitoError, match="fin_colors_expand"):
            col.depth_histogram(dep, 8)
        assert (out == SENT).all() and (unc == SENT).all() and (hist == SENT).all()   # (a refusal writes nothing)
        col.expand()
        assert raw_color_hist(col, dep, 8, 1, out, unc)[0] == fa.FIN_OK and int(out.reshape(5, 2, 8)[:, 0, 1:].sum()) == 0 and int(unc[0]) > 0
    finally:
        for a in (col, dep, dep_o):
            a.close()
        other.close()


def test_a_withheld_step_is_reported_until_the_reset():
    """tests/test_color_coverage.py::test_a_withheld_step_is_reported_until_the_reset's recipe: a step whose overflow list overran is added to the depth, which
    flags itself; both calls then answer FIN_ELIMIT with fin_depth_download's message and write nothing, until the reset; the same for the colours"""
    k = 31
    rng = np.random.default_rng(11)
    g = random_genome(rng, 40000)
    p = fa.FinimizerIndex.build(cut_unitigs(rng, g, k, max_len=500), k).to_device(0)
    reads = sample_reads(rng, g, 500, 150)
    L = fa.lib()
    col, dep = p.colors(3), p.depth()
    windows = [g[i:min(20000, i + 5000 + k - 1)] for i in range(0, 20000, 5000)]   # (overlapping by k - 1 bases: no k-mer is lost)
    col.add_reads(windows, 0)
    out, unc, hist = (np.full(n, SENT, dtype=np.uint64) for n in (3 * 2 * 8, 8, 8))

    def refused(word):
        for _ in range(2):
            rc_, msg = raw_color_hist(col, dep, 8, 1, out, unc)
            assert rc_ == fa.FIN_ELIMIT and "overflow list" in msg and word in msg, (rc_, msg)
        assert (out == SENT).all() and (unc == SENT).all()
        with pytest.raises(fa.FinitoError) as e:
            col.depth_histogram(dep, 8)
        assert e.value.code == fa.FIN_ELIMIT

    try:
        assert L.fin_set_option(b"lds_deque_limit", 1) == 0 and L.fin_set_option(b"seed_anchors", 0) == 0 and L.fin_set_option(b"debug_ovf_cap", 3) == 0
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        dep.add(b)   # nobody has looked at the step's overflow counter yet: the kernel does
        refused("nothing of it was counted")
        rc_, msg = raw_hist(dep, 8, 1, hist)
        assert rc_ == fa.FIN_ELIMIT and "nothing of it was counted" in msg and (hist == SENT).all()
        with pytest.raises(fa.FinitoError) as e:
            dep.histogram(8)
        assert e.value.code == fa.FIN_ELIMIT
        dep.reset()
        h = col.depth_histogram(dep, 8)
        assert not h.table[:, :, 1:].any() and h.kmers[0] > 0 and int(dep.histogram(8)[0]) == int(nk_of(p).sum())
        col.add(b, 1)
        refused("nothing of it was coloured")
        assert raw_hist(dep, 8, 1, hist)[0] == fa.FIN_OK   # (the spectrum does not look at the colours)
        b.close()
        col.reset()
        assert L.fin_set_option(b"debug_ovf_cap", 0) == 0
        col.add_reads(windows, 0)
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        dep.add(b)
        h = col.depth_histogram(dep, 8)
        want = color_model(dep.download()[0], p.export(fa.X_ENDS), k, col.download()[0], 3, 8, 1)
        assert_hist(h, want, "a good step after the resets")
        assert h.table[0, 0, 1:].any()
        b.close()
    finally:
        L.fin_set_option(b"lds_deque_limit", 16); L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"debug_ovf_cap", 0)
        for a in (dep, col):
            a.close()
        p.close()


def test_a_read_set_through_the_index():
    """FinimizerIndex.color_depth_histogram on references coloured by search: reads drawn from reference 0 alone leave reference 1's own k-mers at depth 0"""
    k = 31
    rng = np.random.default_rng(4800)
    shared, priv = random_genome(rng, 4000), [random_genome(rng, 3000) for _ in range(2)]
    unitigs = []
    for piece in [shared] + priv:
        unitigs += cut_unitigs(rng, piece, k, max_len=300)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    col = p.colors(2)
    for c in range(2):
        col.add_reads([shared, priv[c]], c)
    try:
        reads = sample_reads(rng, shared + priv[0], 1500, 100, err=0.0, random_frac=0.0)
        h = p.color_depth_histogram(reads, col, n_bins=64)
        dep = p.depth().add_reads(reads)
        assert_hist(h, color_model(dep.download()[0], p.export(fa.X_ENDS), k, col.download()[0], 2, 64, 1), "FinimizerIndex.color_depth_histogram")
        dep.close()
        med, sat = h.median(only=True)
        assert med[0] >= 5 and med[1] == 0 and not sat.any() and h.breadth(only=True)[1] == 0.0 and h.breadth(only=True)[0] > 0.9
        assert h.iqr()[0][0] >= 0 and h.median()[0][1] > 0   # (reference 1 shares the covered piece)
    finally:
        col.close(); p.close()
