"""Shared k-mers between references: the colour matrix times itself on the device (include/finito_amd.h: fin_colors_shared; fin_colsim.hip).  The
device is held against the host twin (fa.unitig_color_shared) and against the numpy model of tests/test_color_shared_host.py (`shared_model`), byte for byte; what
goes into twin and model are the accumulators' own downloads -- Colors.download()'s matrix, Cover.download()'s covered[] -- and nk from the index's exported unitig
ends, never a result of the call under test."""
import ctypes as C

import numpy as np
import pytest

import finito_amd as fa
from tests.test_color_coverage import canonical_kmers, hand_made, nk_of
from tests.test_color_coverage_host import matrix
from tests.test_color_shared_host import shared_model
from tests.test_eqclasses import N_COLORS_OF_W, small   # noqa: F401 (the fixture: the suite's small index)
from tests.util import cut_unitigs, random_genome, sample_reads

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
BIG = 2 ** 40


def check(col, v, cover, weights, what):
    """device == twin == model under the weights v; the matrix is the colours' own download"""
    bits = col.download()[0]
    want = shared_model(bits, col.n_colors, v)
    twin = fa.unitig_color_shared(bits, col.n_colors, v, n_threads=3)
    got = col.shared(cover=cover, weights=weights)
    assert twin.table.tobytes() == want.tobytes(), what + ": twin and model differ"
    assert got.table.dtype == np.uint64 and got.table.shape == (col.n_colors, col.n_colors)
    assert got.table.tobytes() == want.tobytes(), "%s: %d entries differ from the model" % (what, int((got.table != want).sum()))
    assert np.array_equal(got.table, got.table.T) and np.array_equal(got.sizes, np.diagonal(want))
    return got


@pytest.fixture(scope="module")
def filled(small):   # noqa: F811
    p, g, rng = small
    cov = p.cover().add_reads(sample_reads(rng, g, 200, 100, err=0.01))
    assert 0 < int((cov.download()[1] > 0).sum()) < p.n_unitigs
    yield p, nk_of(p), cov
    cov.close()


@pytest.mark.parametrize("chunk", [64, 0])
@pytest.mark.parametrize("W", [1, 2, 3, 64])
def test_hand_made_matrices(filled, W, chunk):
    p, nk, cov = filled
    n_colors = N_COLORS_OF_W[W]
    rng = np.random.default_rng(4600 + W)
    assert p.n_unitigs >= 200 and p.n_unitigs % 64 and (chunk == 0 or p.n_unitigs > 3 * chunk)   # several chunks, the last one partial
    bits = hand_made(rng, p.n_unitigs, n_colors)
    col = p.colors(n_colors, bits)
    before = cov.download()
    covered = before[1]
    p.set_option("colsim_chunk", chunk)
    try:
        what = "W=%d, chunk %d, " % (W, chunk)
        got = check(col, nk, None, None, what + "the unitigs' k-mers")
        assert np.array_equal(got.sizes, col.coverage(cov).kmers) and got.sizes.any()
        assert col.shared().table.tobytes() == got.table.tobytes(), what + "the second call differs"
        got = check(col, covered, cov, None, what + "the found k-mers")
        assert np.array_equal(got.sizes, col.coverage(cov).covered) and got.sizes.any()
        assert col.shared(cover=cov).table.tobytes() == got.table.tobytes(), what + "the second call differs"
        big = np.full(p.n_unitigs, BIG, dtype=np.uint64)
        got = check(col, big, None, big, what + "weights of 2^40")
        assert int(got.table.max()) > 2 ** 32 and int(got.table.max()) % BIG == 0
        assert col.shared(weights=big).table.tobytes() == got.table.tobytes(), what + "the second call differs"
    finally:
        p.set_option("colsim_chunk", None)
    after = cov.download()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes() and before[2] == after[2], "the call changed the bitmap"
    assert col.download()[0].tobytes() == bits.tobytes(), "the call changed the matrix"
    col.close()


def raw_shared(col, cov, weights, out):
    err = C.create_string_buffer(512)
    rc_ = col.L.fin_colors_shared(col.h, cov.h if cov is not None else None, weights.ctypes.data_as(C.c_void_p) if weights is not None else None,
                                  out.ctypes.data_as(C.c_void_p) if out is not None else None, err, 512)
    return rc_, err.value.decode()


@pytest.mark.parametrize("n_colors", [1, 65])
def test_the_last_row_and_column_stay_inside_out(small, n_colors):   # noqa: F811
    """out's stride is n_colors, not 64 W: a word behind the table keeps its sentinel, under both chunkings"""
    p, g, rng = small
    nk = nk_of(p)
    rng = np.random.default_rng(4700 + n_colors)
    col = p.colors(n_colors, hand_made(rng, p.n_unitigs, n_colors))
    want = shared_model(col.download()[0], n_colors, nk)
    assert want[n_colors - 1, n_colors - 1] > 0 and want[0, n_colors - 1] > 0
    try:
        for chunk in (64, 0):
            p.set_option("colsim_chunk", chunk)
            out = np.full(n_colors * n_colors + 4, SENTINEL, dtype=np.uint64)
            rc_, msg = raw_shared(col, None, None, out)
            assert rc_ == fa.FIN_OK, msg
            assert out[: n_colors * n_colors].tobytes() == want.tobytes() and (out[n_colors * n_colors:] == SENTINEL).all()
    finally:
        p.set_option("colsim_chunk", None)
        col.close()


def test_three_references_coloured_by_search():
    """tests/test_color_coverage.py's index: a shared piece and three private ones, coloured by searching every reference, and a fourth colour that is reference 0
    again.  Every k-mer of a unitig shares its colour set, so shared[i][j] is the number of distinct canonical k-mers references i and j have in common"""
    k = 31
    rng = np.random.default_rng(4800)
    shared, priv = random_genome(rng, 6000), [random_genome(rng, 3000) for _ in range(3)]
    unitigs = []
    for piece in [shared] + priv:
        unitigs += cut_unitigs(rng, piece, k, max_len=300)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    refs = [[shared, priv[0]], [shared, priv[1]], [shared, priv[2]], [shared, priv[0]]]
    col = p.colors(4)
    for c, r in enumerate(refs):
        col.add_reads(r, c)
    try:
        assert len(canonical_kmers(unitigs, k)) == sum(len(u) - k + 1 for u in unitigs), "a k-mer in two unitigs: the sums of nk would not be set sizes"
        kmers = [canonical_kmers(r, k) for r in refs]
        got = col.shared()
        assert [[int(x) for x in row] for row in got.table] == [[len(kmers[i] & kmers[j]) for j in range(4)] for i in range(4)]
        assert got.identical_groups() == [[0, 3]] and got.contained() == []
        assert got.jaccard[0, 3] == 1.0 and 0 < got.jaccard[0, 1] < 1 and got.containment[1, 0] == got.table[1, 0] / got.sizes[1]
        # reads from reference 0 alone: what references 1 and 2 share of the found k-mers is the found k-mers of the shared piece
        reads = sample_reads(rng, shared + priv[0], 400, 100, err=0.0, random_frac=0.0)
        cov = p.cover().add_reads(reads)
        found = canonical_kmers(reads, k)
        sc = col.shared(cover=cov)
        assert [[int(x) for x in row] for row in sc.table] == [[len(kmers[i] & kmers[j] & found) for j in range(4)] for i in range(4)]
        assert int(sc.table[1, 2]) == len(found & canonical_kmers([shared], k)) > 0 and int(sc.sizes[0]) > int(sc.sizes[1])
        assert sc.identical_groups() == [[0, 3], [1, 2]] and sc.contained() == [(1, 0), (1, 3), (2, 0), (2, 3)]
        assert np.array_equal(sc.sizes, col.coverage(cov).covered)
        cov.close()
    finally:
        col.close(); p.close()


def test_after_more_adds_and_an_upload(small):   # noqa: F811
    """the result follows every add to the bitmap and a new matrix: the scratch of an earlier call is not the answer of a later one"""
    p, g, rng = small
    nk = nk_of(p)
    n_colors = 100
    rng = np.random.default_rng(4900)
    col = p.colors(n_colors, hand_made(rng, p.n_unitigs, n_colors))
    cov = p.cover()
    p.set_option("colsim_chunk", 64)
    try:
        first = check(col, cov.download()[1], cov, None, "nothing added")
        assert not first.table.any()
        base = check(col, nk, None, None, "the graph")
        seen = first
        for step in range(3):
            cov.add_reads(sample_reads(rng, g, 60, 90, err=0.0))
            got = check(col, cov.download()[1], cov, None, "after add %d" % step)
            assert (got.table >= seen.table).all() and int(got.table.sum()) > int(seen.table.sum()) and (got.table <= base.table).all()
            seen = got
        col.upload(hand_made(rng, p.n_unitigs, n_colors))
        got = check(col, cov.download()[1], cov, None, "a new matrix")
        assert got.table.tobytes() != seen.table.tobytes()
        check(col, nk, None, None, "a new matrix, the graph")
        cov.reset()
        assert not check(col, cov.download()[1], cov, None, "the bitmap reset").table.any()
    finally:
        p.set_option("colsim_chunk", None)
        cov.close(); col.close()


def test_refusals(small):   # noqa: F811
    p, g, rng = small
    k = 31
    rng = np.random.default_rng(5000)
    other = fa.FinimizerIndex.build(cut_unitigs(rng, random_genome(rng, 3000), k, max_len=80), k).to_device(0)
    col = p.colors(5, matrix(rng, p.n_unitigs, 5))
    cov, cov_o = p.cover(), other.cover()
    w = np.ones(p.n_unitigs, dtype=np.uint64)
    out = np.full(5 * 5 + 1, SENTINEL, dtype=np.uint64)
    sentinel = out.tobytes()
    try:
        rc_, msg = raw_shared(col, cov_o, None, out)
        assert rc_ == fa.FIN_EINVAL and "coverage bitmap" in msg and "different indexes or devices" in msg and out.tobytes() == sentinel
        with pytest.raises(fa.FinitoError) as e:
            col.shared(cover=cov_o)
        assert e.value.code == fa.FIN_EINVAL
        rc_, msg = raw_shared(col, cov, w, out)
        assert rc_ == fa.FIN_EINVAL and "both" in msg and out.tobytes() == sentinel
        with pytest.raises(fa.FinitoError) as e:
            col.shared(cover=cov, weights=w)
        assert e.value.code == fa.FIN_EINVAL
        with pytest.raises(fa.FinitoError) as e:   # weights of another length never reach the library
            col.shared(weights=w[:-1])
        assert e.value.code == fa.FIN_EINVAL
        rc_, msg = raw_shared(col, cov, None, None)
        assert rc_ == fa.FIN_EINVAL and "null" in msg
        err = C.create_string_buffer(512)
        assert col.L.fin_colors_shared(None, cov.h, None, out.ctypes.data_as(C.c_void_p), err, 512) == fa.FIN_EINVAL and out.tobytes() == sentinel
        rc_, msg = raw_shared(col, None, w, out)
        assert rc_ == fa.FIN_OK and out[:25].tobytes() == col.shared(weights=w).table.tobytes() and out[25] == SENTINEL
        assert out[:25].tobytes() == shared_model(col.download()[0], 5, w).tobytes()   # (weights of 1: shared unitigs)
    finally:
        for a in (cov, cov_o, col):
            a.close()
        other.close()


def test_a_withheld_step_is_reported_until_the_reset():
    """tests/test_color_coverage.py::test_a_withheld_step_is_reported_until_the_reset's recipe: a step whose overflow list overran is added to the bitmap, which
    flags itself; the product then answers FIN_ELIMIT with fin_cover_download's message and writes nothing, until the reset; the same for the colours"""
    k = 31
    rng = np.random.default_rng(11)
    g = random_genome(rng, 40000)
    p = fa.FinimizerIndex.build(cut_unitigs(rng, g, k, max_len=500), k).to_device(0)
    reads = sample_reads(rng, g, 500, 150)
    nk = nk_of(p)
    L = fa.lib()
    col = p.colors(3)
    windows = lambda a, b: [g[i:min(b, i + 5000 + k - 1)] for i in range(a, b, 5000)]   # (overlapping by k - 1 bases: no k-mer is lost)
    col.add_reads(windows(0, 20000), 0).add_reads(windows(10000, 40000), 2)
    cov = p.cover()
    out = np.full(3 * 3 + 1, SENTINEL, dtype=np.uint64)
    sentinel = out.tobytes()

    def refused(c_, word):
        for _ in range(2):
            rc_, msg = raw_shared(col, c_, None, out)
            assert rc_ == fa.FIN_ELIMIT and "overflow list" in msg and word in msg and out.tobytes() == sentinel, (rc_, msg)
        with pytest.raises(fa.FinitoError) as e:
            col.shared(cover=c_)
        assert e.value.code == fa.FIN_ELIMIT

    try:
        assert L.fin_set_option(b"lds_deque_limit", 1) == 0 and L.fin_set_option(b"seed_anchors", 0) == 0 and L.fin_set_option(b"debug_ovf_cap", 3) == 0
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        cov.add(b)   # nobody has looked at the step's overflow counter yet: the kernel does
        refused(cov, "nothing of it was set")
        got = check(col, nk, None, None, "the graph alone, the bitmap flagged")
        assert got.sizes[0] > 0 and got.sizes[2] > 0 and got.sizes[1] == 0 and 0 < got.table[0, 2] < got.sizes[0]
        cov.reset()
        assert not check(col, cov.download()[1], cov, None, "after the reset").table.any()
        col.add(b, 1)
        refused(cov, "nothing of it was coloured")
        refused(None, "nothing of it was coloured")
        b.close()
        col.reset()
        assert L.fin_set_option(b"debug_ovf_cap", 0) == 0
        col.add_reads(windows(0, 20000), 0)
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        cov.add(b)
        got = check(col, cov.download()[1], cov, None, "a good step after the resets")
        assert got.sizes[0] > 0 and got.sizes[1] == 0 and got.sizes[2] == 0
        b.close()
    finally:
        L.fin_set_option(b"lds_deque_limit", 16); L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"debug_ovf_cap", 0)
        for a in (cov, col):
            a.close()
        p.close()
