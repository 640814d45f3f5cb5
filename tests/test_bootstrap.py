"""Bootstrap replicates of the abundance estimate, resampled on the device (include/finito_amd.h: fin_eqclasses_bootstrap; fin_bootstrap.hip).
The resampled counts are exact integers and are compared with tests/test_bootstrap_host.py's Python restatement, never with the library; a replicate's estimate
is compared with tests/test_abundance_host.py's numpy model over the replicate's non-zero classes under that module's two rules: one iteration within
RTOL1 = 4 (C + n_colors + 4) 2^-53 (C: the classes of the dense list, which keeps the zero-count ones), fifty within 16 D with D measured on the case itself."""
import ctypes as C

import numpy as np
import pytest
import torch

import finito_amd as fa
from tests.test_abundance import fill
from tests.test_abundance_host import Model, assert_many_iterations, measured_tolerance, random_classes, rtol1
from tests.test_bootstrap_host import M64, N_LIST, class_count, counts_ref, row_hash
from tests.test_colors_host import pack, words_of
from tests.test_eqclasses import on_device, small   # noqa: F401 (the fixture: the suite's small index)
from tests.test_streams import Delay

pytestmark = pytest.mark.gpu


# ---- 1. the launchers on hand-made dense lists -----------------------------------------------------------------------------------------
def run_resample(rows, reads, W, seed, b, twice=True):
    """fin_bootstrap.hip's launchers over a hand-made dense {rows, reads} list: (h, counts, N_b, S)"""
    L = fa.lib()
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.fin_launch_ab_rowhash.argtypes = [vp, u64, u32, vp, vp]
    L.fin_launch_ab_slabs.argtypes = [vp, u64, vp, vp, vp, vp]
    L.fin_launch_ab_resample.argtypes = [vp, vp, vp, u64, u64, u64, u32, vp, vp, vp]
    n = len(rows)
    d_rows, d_reads = on_device(rows), on_device(reads)
    i64 = lambda k: torch.zeros(k, dtype=torch.int64, device="cuda")
    d_h, d_pref, d_counts, d_nb, d_S, d_slabs = i64(n), i64(n), i64(n), i64(1), i64(1), torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert L.fin_launch_ab_rowhash(d_rows.data_ptr(), n, W, d_h.data_ptr(), None) == 0
    assert L.fin_launch_ab_slabs(d_reads.data_ptr(), n, d_slabs.data_ptr(), d_pref.data_ptr(), d_S.data_ptr(), None) == 0
    torch.cuda.synchronize()
    S = int(d_S.cpu()[0])
    slabs = (np.asarray(reads, dtype=np.uint64).astype(np.int64) + 4095) // 4096
    assert S == int(slabs.sum()) and np.array_equal(d_slabs.cpu().numpy(), slabs) and np.array_equal(d_pref.cpu().numpy(), np.cumsum(slabs) - slabs)
    out = []
    for _ in range(2 if twice else 1):
        d_counts.zero_(); d_nb.zero_()
        torch.cuda.synchronize()
        assert L.fin_launch_ab_resample(d_h.data_ptr(), d_reads.data_ptr(), d_pref.data_ptr(), n, S, seed, b, d_counts.data_ptr(), d_nb.data_ptr(), None) == 0
        torch.cuda.synchronize()
        out.append((d_counts.cpu().numpy().view(np.uint64), int(d_nb.cpu()[0])))
    assert all(np.array_equal(o[0], out[0][0]) and o[1] == out[0][1] for o in out), "two runs into re-zeroed buffers differ"
    return d_h.cpu().numpy().view(np.uint64), out[0][0], out[0][1], S


@pytest.mark.parametrize("W", [1, 2, 3, 64])
def test_launchers_on_hand_made_lists(W):
    """C = 1, 63, 64, 65 and 300 classes whose reads walk through 1, 2, 3, 4, 5, 4095, 4096, 4097, 8193 and -- once per list of three classes or more -- 2^20:
    256 slabs on one counter.  The list is in random order, as a dense list is"""
    rng = np.random.default_rng(2700 + W)
    for n_classes, seed, b in ((1, 0, 0), (63, 1, 255), (64, 1 << 32, 256), (65, M64, 4095), (300, 0x0123456789ABCDEF, 1)):
        rows, _ = random_classes(rng, n_classes, 64 * W)
        reads = np.array([N_LIST[(j + 7) % 10] for j in range(n_classes)], dtype=np.uint64)
        reads[(reads == 1 << 20) & (np.arange(n_classes) != 2)] = 4096
        perm = rng.permutation(n_classes)
        rows, reads = rows[perm], reads[perm]
        h, counts, n_b, S = run_resample(rows, reads, W, seed, b)
        what = "W = %d, %d classes" % (W, n_classes)
        assert np.array_equal(h, np.array([row_hash(r) for r in rows], dtype=np.uint64)), what + ": the row hashes"
        want = counts_ref(rows, reads, seed, b)
        assert np.array_equal(counts, want), what + ": the counts"
        assert n_b == int(want.sum()), what
        if n_classes >= 3:
            assert (reads == 1 << 20).sum() == 1 and S >= 256
    if W == 1:   # replicates and seeds are not copies of each other, on the device as in the restatement
        one = lambda seed, b: int(run_resample(pack([[3, 40]], 64), [1000], 1, seed, b, twice=False)[1][0])
        assert one(5, 0) != one(5, 1) and one(5, 0) != one(6, 0) and one(5, 0) == int(class_count(row_hash(pack([[3, 40]], 64)[0]), 1000, 5, 0)[0])


# ---- 2. through the accumulator --------------------------------------------------------------------------------------------------------
def classes_for(rng, n_colors, n_classes):
    """distinct classes with 1 .. 3 reads each, three of them with 4095, 4096 and 4097: up to 4097 rows of one class go through add_rows"""
    C_ = min(n_classes, (1 << n_colors) - 1 if n_colors < 20 else n_classes)
    rows, reads = random_classes(rng, C_, n_colors, max_reads=3, skip=(1,) if n_colors > 5 else ())
    reads[rng.permutation(C_)[:3]] = [4095, 4096, 4097]
    return rows, reads


def assert_replicate_after_one_iteration(alpha, iters, crows, counts, n_colors, lens, what):
    """rule 2 of tests/test_abundance_host.py on a replicate: alpha relative to the value, an exactly-zero colour exactly zero"""
    nz = counts > 0
    want = Model(crows[nz], counts[nz], n_colors, lens).run(1, 0.0)["alpha"]
    r = rtol1(len(crows), n_colors)
    assert iters == 1, what
    assert np.array_equal(alpha == 0.0, want == 0.0), what + ": the colours that are exactly zero"
    assert (np.abs(alpha - want) <= r * np.abs(want)).all(), "%s: alpha off by %.3g relative, bound %.3g" % (what, (np.abs(alpha - want) / np.maximum(np.abs(want), 1e-300)).max(), r)


@pytest.mark.parametrize("n_colors,n_classes", [(5, 31), (130, 300), (4096, 300)])
def test_through_the_accumulator(small, n_colors, n_classes):
    p, g, _ = small
    rng = np.random.default_rng(2710 + n_colors)
    rows, reads = classes_for(rng, n_colors, n_classes)
    lens = rng.uniform(0.5, 2000, n_colors)
    col = p.colors(n_colors)
    eq = col.eqclasses(1024)
    t = fill(eq, rows, reads, rng)
    crows, creads, un = eq.download()                                       # np.unique's order: the expectation is built from the download
    assert len(crows) == len(rows) and creads.max() == 4097 and un == 0
    seed, n_boot = 2710, 3
    want = [counts_ref(crows, creads, seed, b) for b in range(n_boot)]
    what = "%d colours, %d classes" % (n_colors, len(crows))
    p.set_option("ab_chunk", 64)
    try:
        one = eq.bootstrap(n_boot, seed=seed, lengths=lens, max_iters=1, tol=0.0)
        assert [int(x) for x in one.n_reads] == [int(w.sum()) for w in want], what + ": N_b"
        assert any((w == 0).any() for w in want), what + ": no replicate has an empty class"
        for b in range(n_boot):
            assert_replicate_after_one_iteration(one.alpha[b], one.iters[b], crows, want[b], n_colors, lens, "%s, replicate %d" % (what, b))
            assert abs(one.alpha[b].sum() - int(one.n_reads[b])) <= rtol1(len(crows), n_colors) * int(one.n_reads[b])
        point = eq.abundance(lens, max_iters=1, tol=0.0)
        assert np.array_equal(one.point.alpha, point.alpha) and one.point.loglik == point.loglik and one.point.n_reads == int(creads.sum())
        fifty = eq.bootstrap(n_boot, seed=seed, lengths=lens, max_iters=50, tol=0.0)
        assert np.array_equal(fifty.n_reads, one.n_reads)
        for b in range(n_boot):
            nz = want[b] > 0
            allowed, ref = measured_tolerance(crows[nz], want[b][nz], n_colors, lens, 50, rng, "%s, replicate %d" % (what, b))
            got = type("R", (), dict(alpha=fifty.alpha[b], iters=int(fifty.iters[b]), converged=bool(fifty.converged[b]), trace=None, loglik=float(ref["loglik"])))
            assert_many_iterations(got, ref, allowed, "%s, replicate %d" % (what, b))   # (a replicate reports no log-likelihood: alpha, iters and converged are what is checked)
            assert n_colors == 5 or fifty.alpha[b][1] == 0.0
    finally:
        p.set_option("ab_chunk", None)
    del t
    eq.close(); col.close()


def test_order_free_across_fills(small):
    """the same rows added in two shuffled orders into two accumulators: the slot orders differ, the resampled counts do not"""
    p, g, _ = small
    n_colors = 130
    rng = np.random.default_rng(2720)
    rows, reads = classes_for(rng, n_colors, 400)
    col = p.colors(n_colors)
    got = []
    for _ in range(2):
        eq = col.eqclasses(1024)
        t = fill(eq, rows, reads, rng)
        got.append(eq.bootstrap(4, seed=77, max_iters=1, tol=0.0))
        del t
        eq.close()
    a, b = got
    assert np.array_equal(a.n_reads, b.n_reads) and [int(x) for x in a.n_reads] == [int(counts_ref(rows, reads, 77, r).sum()) for r in range(4)]
    assert (np.abs(a.alpha - b.alpha) <= rtol1(len(rows), n_colors) * np.abs(b.alpha)).all() and np.array_equal(a.alpha == 0, b.alpha == 0)
    col.close()


def test_determinism_point_estimate_and_the_accumulator_left_as_found(small):
    p, g, _ = small
    n_colors = 130
    rng = np.random.default_rng(2730)
    rows, reads = classes_for(rng, n_colors, 500)
    lens = rng.uniform(0.5, 2000, n_colors)
    col = p.colors(n_colors)
    eq = col.eqclasses(1024)
    t = fill(eq, rows, reads, rng)
    before, stats, est = eq.download(), eq.stats(), eq.abundance(lens, max_iters=40, tol=1e-9)
    a = eq.bootstrap(3, seed=5, lengths=lens, max_iters=40, tol=1e-9)
    b = eq.bootstrap(3, seed=5, lengths=lens, max_iters=40, tol=1e-9)
    seven = eq.bootstrap(7, seed=5, lengths=lens, max_iters=40, tol=1e-9)
    for x in (b, seven):
        assert np.array_equal(x.alpha[:3], a.alpha) and np.array_equal(x.n_reads[:3], a.n_reads) and np.array_equal(x.iters[:3], a.iters)
        assert np.array_equal(x.converged[:3], a.converged) and np.array_equal(x.point.alpha, a.point.alpha) and x.point.loglik == a.point.loglik
    assert np.array_equal(b.mean, a.mean) and np.array_equal(b.sd, a.sd) and a.seed == 5 and seven.alpha.shape == (7, n_colors)
    assert not np.array_equal(seven.alpha[3], seven.alpha[4]) and not np.array_equal(eq.bootstrap(1, seed=6, lengths=lens, max_iters=40, tol=1e-9).n_reads, a.n_reads[:1])
    # the point estimate is abundance()'s, bit for bit
    pt = a.point
    assert np.array_equal(pt.alpha, est.alpha) and (pt.iters, pt.converged, pt.loglik, pt.max_change, pt.n_reads, pt.n_classes, pt.n_unaligned) == \
        (est.iters, est.converged, est.loglik, est.max_change, est.n_reads, est.n_classes, est.n_unaligned)
    assert np.array_equal(a.theta, a.alpha / a.n_reads.astype(np.float64)[:, None]) and np.array_equal(a.sd, a.alpha.std(axis=0, ddof=1))
    # the accumulator is left as it was found
    after = eq.download()
    assert all(np.array_equal(x, y) for x, y in zip(before[:2], after[:2])) and before[2] == after[2] and eq.stats() == stats
    later = eq.abundance(lens, max_iters=40, tol=1e-9)
    assert np.array_equal(later.alpha, est.alpha) and later.loglik == est.loglik and later.iters == est.iters
    del t
    eq.close(); col.close()


# ---- 3. empty replicates, an empty accumulator, refusals -------------------------------------------------------------------------------
def test_empty_replicates_and_an_empty_accumulator(small):
    p, g, _ = small
    col = p.colors(3)
    eq = col.eqclasses(64)
    empty = eq.bootstrap(4, seed=1)
    assert not empty.alpha.any() and not empty.n_reads.any() and not empty.iters.any() and empty.converged.all() and not empty.theta.any()
    assert empty.point.iters == 0 and empty.point.converged and not empty.point.alpha.any() and empty.point.n_classes == 0
    row = pack([[1]], 3)
    t = fill(eq, row, [1])                                                  # N = 1: a replicate is empty with probability 1 / e
    counts = [int(class_count(row_hash(row[0]), 1, 2650, b)[0]) for b in range(16)]
    assert 0 in counts and any(counts), counts
    got = eq.bootstrap(16, seed=2650, max_iters=10)
    assert [int(x) for x in got.n_reads] == counts and np.array_equal(got.point.alpha, [0.0, 1.0, 0.0])
    for b, c in enumerate(counts):
        if c == 0:
            assert not got.alpha[b].any() and got.iters[b] == 0 and got.converged[b] and not got.theta[b].any()
        else:
            assert np.array_equal(got.alpha[b], [0.0, float(c), 0.0]) and got.iters[b] >= 1 and got.converged[b] and np.array_equal(got.theta[b], [0.0, 1.0, 0.0])
    zeros = on_device(np.zeros((5, 1), dtype=np.uint64))
    only_unaligned = eq.reset().add_rows(zeros.data_ptr(), 5).bootstrap(2)
    assert not only_unaligned.alpha.any() and only_unaligned.point.n_unaligned == 5 and not only_unaligned.n_reads.any()
    del t
    eq.close(); col.close()


def test_refusals(small):
    p, g, _ = small
    n_colors = 70
    rng = np.random.default_rng(2740)
    rows, reads = random_classes(rng, 40, n_colors, max_reads=2)
    col = p.colors(n_colors)
    eq = col.eqclasses(32)
    t = fill(eq, rows[:20], reads[:20])
    L, err = fa.lib(), C.create_string_buffer(512)
    out = fa._BootOut(4, n_colors)
    call = lambda nb, mi=10, tol=1e-6: L.fin_eqclasses_bootstrap(eq.h, None, mi, tol, nb, 0, *out.args(), err, 512)
    for nb, code in ((0, fa.FIN_EINVAL), (4097, fa.FIN_ELIMIT)):
        with pytest.raises(fa.FinitoError) as e:
            eq.bootstrap(nb)
        assert e.value.code == code and "n_boot is 1 .. 4096" in str(e.value)
        assert call(nb) == code and b"n_boot is 1 .. 4096" in err.value
    assert call(4, 0) == fa.FIN_EINVAL and call(4, 100001) == fa.FIN_ELIMIT and call(4, 10, -1.0) == fa.FIN_EINVAL
    for kw, code in ((dict(max_iters=0), fa.FIN_EINVAL), (dict(tol=float("nan")), fa.FIN_EINVAL), (dict(lengths=np.ones(69)), fa.FIN_EINVAL), (dict(seed=-1), fa.FIN_EINVAL),
                     (dict(seed=1 << 64), fa.FIN_EINVAL)):
        with pytest.raises(fa.FinitoError) as e:
            eq.bootstrap(4, **kw)
        assert e.value.code == code, kw
    assert call(4) == fa.FIN_OK and out.n_reads.all() and eq.bootstrap(2, seed=M64).n_reads.all()
    # N n_boot above 2^38: the argument check the call makes, on a hand-stated N -- never by running it
    assert L.fin_bootstrap_check((1 << 26) + 1, 4096, err, 512) == fa.FIN_ELIMIT and b"67108865" in err.value and b"4096" in err.value and b"2^38" in err.value
    assert L.fin_bootstrap_check(1 << 26, 4096, err, 512) == fa.FIN_OK
    # a flagged accumulator answers as it answers the download
    t = fill(eq, rows, reads)                                               # 40 classes, room for 32
    with pytest.raises(fa.FinitoError) as e:
        eq.bootstrap(2)
    assert e.value.code == fa.FIN_ELIMIT and "max_classes" in str(e.value)
    bad = rows[:20].copy(); bad[3, 1] |= np.uint64(1) << np.uint64(n_colors & 63)
    t = fill(eq, bad, np.ones(20, dtype=np.int64))
    with pytest.raises(fa.FinitoError) as e:
        eq.bootstrap(2)
    assert e.value.code == fa.FIN_EINVAL and "n_colors" in str(e.value)
    t = fill(eq, rows[:20], reads[:20])                                     # (the reset clears it)
    assert eq.bootstrap(2, max_iters=2).iters.tolist() == [2, 2]
    del t
    eq.close(); col.close()


# ---- 4. order --------------------------------------------------------------------------------------------------------------------------
def test_the_bootstrap_waits_for_an_add_behind_a_delay(small):
    """tests/test_abundance.py's case: the add sits behind a delay on a non-blocking stream when the call is issued, and every replicate includes it"""
    p, g, _ = small
    n_colors = 70
    rng = np.random.default_rng(2750)
    rows, reads = random_classes(rng, 200, n_colors, max_reads=3)
    col = p.colors(n_colors)
    eq = col.eqclasses(1024)
    t = fill(eq, rows[:100], reads[:100], rng)
    eq.stats()
    late = on_device(np.repeat(rows[100:], reads[100:].astype(np.int64), axis=0))
    delay, S = Delay(), torch.cuda.Stream()
    delay(S, 60.0)
    eq.add_rows(late.data_ptr(), late.shape[0], stream=S.cuda_stream)
    assert S.query() is False, "the stream is idle where its delay should still run"
    got = eq.bootstrap(2, seed=3, max_iters=1, tol=0.0)
    assert got.point.n_reads == int(reads.sum()) and got.point.n_classes == 200
    crows, creads, _ = eq.download()
    for b in range(2):
        want = counts_ref(crows, creads, 3, b)
        assert int(got.n_reads[b]) == int(want.sum())
        assert_replicate_after_one_iteration(got.alpha[b], got.iters[b], crows, want, n_colors, None, "behind a delay, replicate %d" % b)
    del t, late
    eq.close(); col.close()
