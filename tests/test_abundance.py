"""Abundances from the equivalence classes, EM on the device (include/finito_amd.h: fin_eqclasses_abundance; fin_abundance.hip).  Rows come through
EqClasses.add_rows on a small index; the expectation is always tests/test_abundance_host.py's numpy model over download()'s classes, never the library, under
that module's two rules: one iteration within RTOL1 = 4 (C + n_colors + 4) 2^-53, many iterations within 16 D with D measured on the case itself.

Read counts: a class gets its reads by adding its row that many times, so through the accumulator the counts go from 1 to 2^17; classes of 1 and of 2^40 reads
are given to the kernels' launchers as a hand-made dense list (test_reads_one_and_two_to_the_forty)."""
import numpy as np
import pytest
import torch

import finito_amd as fa
from tests.test_abundance_host import (TWO, Model, assert_many_iterations, assert_one_iteration, assert_sum_and_trace, measured_tolerance, random_classes, rtol1)
from tests.test_colors_host import pack, words_of
from tests.test_eqclasses import on_device, small   # noqa: F401 (the fixture: the suite's small index)
from tests.test_streams import Delay
from tests.util import cut_unitigs, random_genome, sample_reads

pytestmark = pytest.mark.gpu


def fill(eq, rows, reads, rng=None, reset=True):
    """the classes into the accumulator: row j added reads[j] times, the rows shuffled; returns the device tensor, to be kept until a waiting call"""
    rep = np.repeat(np.asarray(rows, dtype=np.uint64), np.asarray(reads).astype(np.int64), axis=0)
    if rng is not None:
        rep = rep[rng.permutation(len(rep))]
    t = on_device(rep)
    if reset:
        eq.reset()
    eq.add_rows(t.data_ptr(), len(rep))
    return t


def classes_on(eq):
    rows, reads, un = eq.download()
    return rows, reads, un


def max_classes_of(n_colors):
    return (1 << n_colors) - 1 if n_colors < 20 else 1 << 30


# ---- 1. shapes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_colors", [1, 5, 64, 65, 130, 4096])
def test_shapes_with_chunks_of_64(small, n_colors):
    """C = 1, 63, 64, 65, 127, 129 and 4097 under ab_chunk = 64: seams inside, at and behind a wave's step (fewer classes where n_colors has fewer sets)"""
    p, g, _ = small
    rng = np.random.default_rng(2430 + n_colors)
    col = p.colors(n_colors)
    eq = col.eqclasses(8192)
    lens = rng.uniform(0.5, 2000, n_colors)
    p.set_option("ab_chunk", 64)
    try:
        for n_classes in (1, 63, 64, 65, 127, 129, 4097):
            C = min(n_classes, max_classes_of(n_colors))
            rows, reads = random_classes(rng, C, n_colors, max_reads=3, skip=(1,) if n_colors > 5 else ())
            t = fill(eq, rows, reads, rng)
            crows, creads, un = classes_on(eq)
            assert len(crows) == C and un == 0 and int(creads.sum()) == int(reads.sum())
            what = "%d colours, %d classes" % (n_colors, C)
            for ln in (None, lens):
                got = eq.abundance(ln, max_iters=1, tol=0.0, trace=True)
                assert_one_iteration(got, Model(crows, creads, n_colors, ln).run(1, 0.0), C, n_colors, what)
                assert got.n_reads == int(reads.sum()) and got.n_classes == C and got.n_unaligned == 0
            if n_colors >= 64 and C >= 63:
                allowed, ref = measured_tolerance(crows, creads, n_colors, lens, 50, rng, what)
                got = eq.abundance(lens, max_iters=50, tol=0.0, trace=True)
                assert_many_iterations(got, ref, allowed, what)
                assert_sum_and_trace(got.alpha, got.trace, int(reads.sum()), ref["absll"], C, n_colors, what)
                assert got.alpha[1] == 0.0
            del t
    finally:
        p.set_option("ab_chunk", None)
    eq.close(); col.close()


@pytest.mark.parametrize("n_classes,n_colors", [(3000, 5), (3000, 130), (5000, 64), (20000, 4096)])
def test_default_chunks_and_determinism(small, n_classes, n_colors):
    """a few thousand classes at the default ab_chunk, and 20 000 x 4096 once (the largest case: a 10 MB row list); the same filled accumulator estimated twice
    is bit-identical; chunks of 64 against the default differ by rounding only (one iteration, RTOL1)"""
    p, g, _ = small
    rng = np.random.default_rng(2440 + n_colors)
    col = p.colors(n_colors)
    eq = col.eqclasses(32768)
    lens = rng.uniform(0.5, 2000, n_colors)
    C = min(n_classes, max_classes_of(n_colors))
    rows, reads = random_classes(rng, C, n_colors, max_reads=3, skip=(1,) if n_colors > 5 else ())
    t = fill(eq, rows, reads, rng)
    crows, creads, un = classes_on(eq)
    what = "%d colours, %d classes, default chunks" % (n_colors, C)
    one = eq.abundance(lens, max_iters=1, tol=0.0, trace=True)
    assert_one_iteration(one, Model(crows, creads, n_colors, lens).run(1, 0.0), C, n_colors, what)
    if n_colors > 5:
        allowed, ref = measured_tolerance(crows, creads, n_colors, lens, 50, rng, what)
        a = eq.abundance(lens, max_iters=50, tol=0.0, trace=True)
        assert_many_iterations(a, ref, allowed, what)
        assert_sum_and_trace(a.alpha, a.trace, int(reads.sum()), ref["absll"], C, n_colors, what)
    else:
        a = eq.abundance(lens, max_iters=200, tol=1e-9, trace=True)
    b = eq.abundance(lens, max_iters=a.iters, tol=0.0 if n_colors > 5 else 1e-9, trace=True)
    assert np.array_equal(a.alpha, b.alpha) and a.loglik == b.loglik and np.array_equal(a.trace, b.trace) and a.iters == b.iters and a.max_change == b.max_change, what
    p.set_option("ab_chunk", 64)
    try:
        c64 = eq.abundance(lens, max_iters=1, tol=0.0)
    finally:
        p.set_option("ab_chunk", None)
    assert (np.abs(c64.alpha - one.alpha) <= rtol1(C, n_colors) * np.abs(one.alpha)).all() and np.array_equal(c64.alpha == 0, one.alpha == 0), what
    if C > 256:
        assert not np.array_equal(c64.alpha, one.alpha) or n_colors <= 5, what + ": chunks of 64 and the default gave the same bits -- is the option read?"
    del t
    eq.close(); col.close()


# ---- 2. rows of interest ---------------------------------------------------------------------------------------------------------------
def test_rows_of_interest(small):
    p, g, _ = small
    n_colors = 4096
    rng = np.random.default_rng(2450)
    rows, reads = random_classes(rng, 600, n_colors, max_reads=3, skip=(1, 10, 11, 4095))
    extra = pack([list(range(4096)), [4095], [10, 11], [10, 11, 77], [10, 11, 4000, 3]], n_colors)   # every colour; bit 63 of the last word alone; 10 and 11 always together
    rows = np.concatenate([rows, extra])
    reads = np.concatenate([reads, np.array([2, 1, 1 << 17, 5, 1], dtype=np.uint64)])              # reads 1 and 2^17
    lens = np.exp(rng.uniform(np.log(0.5), np.log(2000), n_colors))                                   # spread over 0.5 to 2000
    lens[11] = lens[10]
    col = p.colors(n_colors)
    eq = col.eqclasses(2048)
    t = fill(eq, rows, reads)
    crows, creads, un = classes_on(eq)
    C = len(crows)
    assert C == 605 and creads.max() == 1 << 17 and creads.min() == 1
    p.set_option("ab_chunk", 64)
    try:
        one = eq.abundance(lens, max_iters=1, tol=0.0, trace=True)
        assert_one_iteration(one, Model(crows, creads, n_colors, lens).run(1, 0.0), C, n_colors, "rows of interest")
        allowed, ref = measured_tolerance(crows, creads, n_colors, lens, 50, rng, "rows of interest")
        got = eq.abundance(lens, max_iters=50, tol=0.0, trace=True)
    finally:
        p.set_option("ab_chunk", None)
    assert_many_iterations(got, ref, allowed, "rows of interest")
    assert_sum_and_trace(got.alpha, got.trace, int(creads.sum()), ref["absll"], C, n_colors, "rows of interest")
    for r in (one, got):
        assert r.alpha[4095] > 0 and r.alpha[10] > 1 << 16   # (the class of every colour is here, so no colour is in no class: that row of interest is colour 1 of test_shapes_with_chunks_of_64)
        assert abs(r.alpha[10] - r.alpha[11]) <= rtol1(C, n_colors) * r.alpha[10]   # the columns that always occur together, equal lengths
    del t
    eq.close(); col.close()


def run_kernels(rows, reads, n_colors, lens, iters, ab_chunk=0):
    """fin_abundance.hip's launchers over a hand-made dense {rows, reads} list -- what fin_eqclasses_abundance runs behind the table's compaction --, so that a
    class can have any number of reads; tol = 0.  Returns what the assert helpers read: alpha, iters, converged, loglik, max_change, trace"""
    import ctypes as C
    import types
    L = fa.lib()
    vp, u32, u64, dbl = C.c_void_p, C.c_uint32, C.c_uint64, C.c_double
    L.fin_ab_geometry.argtypes = [u64, u32, u32] + [C.POINTER(u32)] * 4
    L.fin_ab_geometry.restype = None
    L.fin_launch_ab_transpose.argtypes = [vp, u64, u32, vp, vp]
    L.fin_launch_ab_iteration.argtypes = [vp, vp, vp, vp, u64, u32, u32, u32, vp, dbl, dbl, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp]
    n_classes, W = len(rows), words_of(n_colors)
    N = int(np.asarray(reads, dtype=np.uint64).astype(object).sum())
    geo = [u32() for _ in range(4)]
    L.fin_ab_geometry(n_classes, W, ab_chunk, *[C.byref(x) for x in geo])
    cpb, n_ll, chunk, n_chunks = [int(x.value) for x in geo]
    assert n_ll * cpb >= n_classes and n_chunks * chunk >= n_classes and chunk % 64 == 0
    pad = 64 * W
    len_p = np.ones(pad); len_p[:n_colors] = lens
    alpha0 = np.zeros(pad); alpha0[:n_colors] = float(N) / n_colors
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_rows, d_reads = on_device(rows), on_device(reads)
    d_rowsT = torch.empty_like(d_rows) if W > 1 else d_rows
    d_len, d_alpha, d_x = dev(len_p), dev(alpha0), dev(alpha0 / len_p)
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device="cuda")
    d_q, d_part, d_ll, d_chg, d_trace = f64(n_classes), f64(n_chunks * pad), f64(n_ll), f64(64), f64(iters)
    d_ok, d_state = torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    if W > 1:
        assert L.fin_launch_ab_transpose(d_rows.data_ptr(), n_classes, W, d_rowsT.data_ptr(), None) == 0
    for t in range(iters):
        assert L.fin_launch_ab_iteration(d_state.data_ptr(), d_rows.data_ptr(), d_rowsT.data_ptr(), d_reads.data_ptr(), n_classes, W, n_colors, ab_chunk, d_len.data_ptr(), float(N),
                                         0.0, d_alpha.data_ptr(), d_x.data_ptr(), d_q.data_ptr(), d_part.data_ptr(), d_ll.data_ptr(), d_ok.data_ptr(), d_chg.data_ptr(), t,
                                         d_trace.data_ptr(), None) == 0
    torch.cuda.synchronize()
    state = d_state.cpu().numpy()
    done, n_it = int(state[0]) & 0xFFFFFFFF, int(state[0]) >> 32
    return types.SimpleNamespace(alpha=d_alpha.cpu().numpy()[:n_colors], iters=n_it, converged=bool(done), max_change=float(state[1:2].view(np.float64)[0]),
                                 loglik=float(state[2:3].view(np.float64)[0]), trace=d_trace.cpu().numpy()[:n_it])


@pytest.mark.parametrize("n_classes,n_colors", [(40, 5), (300, 64), (3000, 130), (700, 4096)])
def test_reads_one_and_two_to_the_forty(n_classes, n_colors):
    """classes of 1 read beside classes of 2^40 reads (N about 10^12 and more), on the kernels themselves: the accumulator counts a row per read, so such counts go
    in through a hand-made dense list.  One iteration under rule 2, fifty under rule 3, chunks of 64 and the default"""
    rng = np.random.default_rng(2455 + n_colors)
    C = min(n_classes, max_classes_of(n_colors))
    rows, reads = random_classes(rng, C, n_colors, max_reads=50, skip=(1,) if n_colors > 5 else ())
    reads[rng.permutation(C)[: max(2, C // 10)]] = np.uint64(1) << np.uint64(40)
    reads[0] = 1; reads[-1] = np.uint64(1) << np.uint64(40); reads[C // 2] = 1
    perm = rng.permutation(C)                                               # (a dense list is in slot order, not in np.unique's)
    rows, reads = rows[perm], reads[perm]
    lens = rng.uniform(0.5, 2000, n_colors)
    N = int(reads.astype(object).sum())
    what = "%d colours, %d classes, reads 1 and 2^40" % (n_colors, C)
    for chunk in (64, 0):
        got = run_kernels(rows, reads, n_colors, lens, 1, chunk)
        assert_one_iteration(got, Model(rows, reads, n_colors, lens).run(1, 0.0), C, n_colors, what)
        assert abs(float(got.alpha.sum()) - N) <= rtol1(C, n_colors) * N
    if n_colors > 5:
        allowed, ref = measured_tolerance(rows, reads, n_colors, lens, 50, rng, what)
        got = run_kernels(rows, reads, n_colors, lens, 50, 64)
        assert_many_iterations(got, ref, allowed, what)
        assert_sum_and_trace(got.alpha, got.trace, N, ref["absll"], C, n_colors, what)
        assert got.alpha[1] == 0.0


# ---- 3. closed forms and stopping ------------------------------------------------------------------------------------------------------
def test_closed_forms_and_stopping(small):
    p, g, _ = small
    rng = np.random.default_rng(2460)
    col = p.colors(6)
    eq = col.eqclasses(64)
    t = fill(eq, pack([[0], [2], [3], [5]], 6), [7, 1, 300, 12], rng)       # singleton classes only: alpha_c = n_c after one iteration
    got = eq.abundance(max_iters=5, tol=1e-9, trace=True)
    assert np.array_equal(got.alpha, [7, 0, 1, 300, 0, 12]) and got.iters == 2 and got.converged and got.max_change <= rtol1(4, 6) and len(got.trace) == 2   # (iteration 1 lands within an ulp of n_c, iteration 2 on it)
    assert np.array_equal(got.theta, got.alpha / 320) and np.array_equal(got.rho, got.alpha / got.alpha.sum())
    eq.close(); col.close()
    col = p.colors(2)
    eq = col.eqclasses(64)
    t = fill(eq, *TWO, rng)
    crows, creads, _ = classes_on(eq)
    m = Model(crows, creads, 2).run(1000, 1e-9)
    assert m["converged"] and m["iters"] == 30
    sentinel = np.full(1000, -7.5)
    got = eq.abundance(max_iters=1000, tol=1e-9, trace=sentinel)
    assert got.converged and abs(got.iters - m["iters"]) <= 1 and abs(got.alpha[0] - 60) <= 2 * 1e-9 * 60 and abs(got.alpha[1] - 20) <= 2 * 1e-9 * 60
    assert (sentinel[got.iters:] == -7.5).all() and (sentinel[: got.iters] != -7.5).all() and got.loglik == sentinel[got.iters - 1]
    assert got.max_change <= 1e-9 and got.n_reads == 80 and got.n_classes == 3
    assert_sum_and_trace(got.alpha, got.trace, 80, m["absll"][: got.iters] if got.iters <= 30 else m["absll"] + m["absll"][-1:], 3, 2, "two colours")
    lazy = eq.abundance(max_iters=3, tol=1e-9)                            # a slow case for three iterations: 40, 50, 55, 57.5
    assert not lazy.converged and lazy.iters == 3 and lazy.trace is None and abs(lazy.alpha[0] - 57.5) <= 57.5 * rtol1(3, 2) * 3
    at32 = eq.abundance(max_iters=32, tol=1e-9)                           # the criterion met inside the first host group, and at its last iteration
    assert at32.converged and at32.iters == got.iters
    exact = eq.abundance(max_iters=got.iters, tol=1e-9)
    assert exact.converged and exact.iters == got.iters and np.array_equal(exact.alpha, got.alpha)
    del t
    eq.close(); col.close()


def test_seventy_iterations_cross_two_host_groups(small):
    p, g, _ = small
    n_colors = 130
    rng = np.random.default_rng(2470)
    rows, reads = random_classes(rng, 3000, n_colors, max_reads=3, skip=(1,))
    lens = rng.uniform(0.5, 2000, n_colors)
    col = p.colors(n_colors)
    eq = col.eqclasses(4096)
    t = fill(eq, rows, reads, rng)
    crows, creads, _ = classes_on(eq)
    allowed, ref = measured_tolerance(crows, creads, n_colors, lens, 70, rng, "70 iterations")
    got = eq.abundance(lens, max_iters=70, tol=0.0, trace=True)
    assert_many_iterations(got, ref, allowed, "70 iterations")
    assert abs(got.max_change - ref["changes"][-1]) <= 1e-6 * ref["changes"][-1]
    del t
    eq.close(); col.close()


# ---- 4. the accumulator is left as it was found ----------------------------------------------------------------------------------------
def test_non_interference(small):
    p, g, _ = small
    n_colors = 100
    rng = np.random.default_rng(2480)
    rows, reads = random_classes(rng, 500, n_colors, max_reads=3)
    col = p.colors(n_colors)
    eq = col.eqclasses(2048)
    empty = eq.abundance(trace=True)
    assert np.array_equal(empty.alpha, np.zeros(n_colors)) and empty.iters == 0 and empty.converged and empty.loglik == 0.0 and empty.n_classes == 0 and len(empty.trace) == 0
    t = fill(eq, rows, reads, rng)
    before, stats = eq.download(), eq.stats()
    got = eq.abundance(max_iters=10, tol=0.0)
    after = eq.download()
    assert all(np.array_equal(a, b) for a, b in zip(before[:2], after[:2])) and before[2] == after[2] and eq.stats() == stats
    more, more_reads = random_classes(rng, 300, n_colors, max_reads=2)
    zeros = on_device(np.zeros((5, words_of(n_colors)), dtype=np.uint64))
    t2 = fill(eq, more, more_reads, rng, reset=False)
    eq.add_rows(zeros.data_ptr(), 5)                                        # unaligned rows take no part
    crows, creads, un = classes_on(eq)
    assert un == 5 and len(crows) > 500 and int(creads.sum()) == int(reads.sum() + more_reads.sum())
    again = eq.abundance(max_iters=1, tol=0.0, trace=True)
    assert_one_iteration(again, Model(crows, creads, n_colors).run(1, 0.0), len(crows), n_colors, "after more adds")
    assert again.n_unaligned == 5 and again.n_reads == int(creads.sum()) and again.n_reads == eq.stats()[0] - eq.stats()[1]
    only_unaligned = eq.reset().add_rows(zeros.data_ptr(), 5).abundance()
    assert only_unaligned.iters == 0 and only_unaligned.n_unaligned == 5 and not only_unaligned.alpha.any()
    after_reset = eq.reset().abundance()
    assert np.array_equal(after_reset.alpha, np.zeros(n_colors)) and after_reset.iters == 0 and after_reset.converged and after_reset.n_unaligned == 0
    del t, t2
    eq.close(); col.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(small):
    p, g, _ = small
    n_colors = 70
    rng = np.random.default_rng(2490)
    rows, reads = random_classes(rng, 40, n_colors, max_reads=2)
    col = p.colors(n_colors)
    eq = col.eqclasses(32)
    t = fill(eq, rows, reads)                                               # 40 classes, room for 32
    with pytest.raises(fa.FinitoError) as e:
        eq.abundance()
    assert e.value.code == fa.FIN_ELIMIT and "max_classes" in str(e.value)
    t = fill(eq, rows[:20], reads[:20])                                     # (the reset clears it)
    assert eq.abundance(max_iters=2).iters == 2
    bad = rows[:20].copy(); bad[3, 1] |= np.uint64(1) << np.uint64(n_colors & 63)
    t = fill(eq, bad, np.ones(20, dtype=np.int64))
    with pytest.raises(fa.FinitoError) as e:
        eq.abundance()
    assert e.value.code == fa.FIN_EINVAL and "n_colors" in str(e.value)
    t = fill(eq, rows[:20], reads[:20])
    assert eq.abundance(max_iters=2).iters == 2
    # arguments, refused before anything is launched
    for kw, code in ((dict(max_iters=0), fa.FIN_EINVAL), (dict(max_iters=100001), fa.FIN_ELIMIT), (dict(tol=-1.0), fa.FIN_EINVAL), (dict(tol=float("nan")), fa.FIN_EINVAL),
                     (dict(lengths=np.ones(69)), fa.FIN_EINVAL)):
        with pytest.raises(fa.FinitoError) as e:
            eq.abundance(**kw)
        assert e.value.code == code, kw
    err = fa.C.create_string_buffer(512)
    f64p = fa.C.POINTER(fa.C.c_double)
    alpha = np.zeros(n_colors)
    for bad_len in (0.0, -1.0, float("inf"), float("nan")):
        lens = np.ones(n_colors); lens[42] = bad_len
        with pytest.raises(fa.FinitoError) as e:
            eq.abundance(lens)
        assert e.value.code == fa.FIN_EINVAL and "colour 42" in str(e.value)
        assert fa.lib().fin_eqclasses_abundance(eq.h, lens.ctypes.data_as(f64p), 10, 1e-6, alpha.ctypes.data_as(f64p), None, None, err, 512) == fa.FIN_EINVAL and b"colour 42" in err.value
    assert fa.lib().fin_eqclasses_abundance(eq.h, None, 0, 1e-6, alpha.ctypes.data_as(f64p), None, None, err, 512) == fa.FIN_EINVAL
    assert fa.lib().fin_eqclasses_abundance(eq.h, None, 100001, 1e-6, alpha.ctypes.data_as(f64p), None, None, err, 512) == fa.FIN_ELIMIT
    assert fa.lib().fin_eqclasses_abundance(eq.h, None, 5, 1e-6, alpha.ctypes.data_as(f64p), None, None, err, 512) == fa.FIN_OK and abs(alpha.sum() - int(reads[:20].sum())) < 1e-9
    del t
    eq.close(); col.close()


# ---- 6. order --------------------------------------------------------------------------------------------------------------------------
def test_the_estimate_waits_for_an_add_behind_a_delay(small):
    """tests/test_streams.py's download case: the add sits behind a delay on a non-blocking stream when the estimate is issued, and the result includes it"""
    p, g, _ = small
    n_colors = 70
    rng = np.random.default_rng(2500)
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
    got = eq.abundance(max_iters=1, tol=0.0, trace=True)
    assert got.n_reads == int(reads.sum()) and got.n_classes == 200
    crows, creads, _ = classes_on(eq)
    assert_one_iteration(got, Model(crows, creads, n_colors).run(1, 0.0), 200, n_colors, "behind a delay")
    del t, late
    eq.close(); col.close()


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------------
def test_end_to_end_three_references():
    """three references with a shared stretch and a private one each, reads drawn 70 / 20 / 10.  The estimate equals the model over the downloaded classes:
    one iteration under RTOL1; run to convergence at tol, both stop within an iteration of each other and each is within a step of its limit, a step being at
    most tol max(alpha, 1) there -- so they differ by at most 2 tol max(alpha, 1).  The order of alpha is the mixture's: the only statement about the truth,
    asserted on the model first"""
    k, tol = 31, 1e-7
    rng = np.random.default_rng(2510)
    shared, priv = random_genome(rng, 6000), [random_genome(rng, 3000) for _ in range(3)]
    unitigs = []
    for piece in [shared] + priv:
        unitigs += cut_unitigs(rng, piece, k, max_len=300)
    refs = [shared + x for x in priv]
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    col = p.colors(3)
    for c, ref in enumerate(refs):
        col.add_reads([shared, priv[c]], c)
    reads = []
    for ref, n in zip(refs, (700, 200, 100)):
        reads += sample_reads(rng, ref, n, 100, err=0.0, random_frac=0.05)
    reads = [reads[i] for i in rng.permutation(len(reads))]
    eq = col.eqclasses(64)
    eq.add_reads(reads)
    crows, creads, un = classes_on(eq)
    st = eq.stats()
    assert len(crows) >= 4 and un > 0 and st[0] == len(reads)
    lens = np.array([len(r) for r in refs], dtype=np.float64)
    m = Model(crows, creads, 3, lens).run(1000, tol)
    assert m["converged"] and m["alpha"][0] > m["alpha"][1] > m["alpha"][2] > 0
    one = eq.abundance(lens, max_iters=1, tol=0.0, trace=True)
    assert_one_iteration(one, Model(crows, creads, 3, lens).run(1, 0.0), len(crows), 3, "end to end")
    got = eq.abundance(lens, max_iters=1000, tol=tol, trace=True)
    assert got.converged and abs(got.iters - m["iters"]) <= 1
    assert (np.abs(got.alpha - m["alpha"]) <= 2 * tol * np.maximum(m["alpha"], 1)).all()
    assert abs(got.alpha.sum() - (st[0] - st[1])) <= rtol1(len(crows), 3) * (st[0] - st[1]) and got.n_unaligned == st[1]
    assert got.alpha[0] > got.alpha[1] > got.alpha[2] > 0 and got.rho[0] > got.rho[1] > got.rho[2]
    eq.close(); col.close(); p.close()
