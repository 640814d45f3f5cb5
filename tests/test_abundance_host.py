"""Abundances from equivalence classes (include/finito_amd.h: fin_classes_abundance, the host twin of fin_eqclasses_abundance) against a NUMPY
MODEL of the definition, written here and never the library: the rows unpacked to a boolean C x n_colors matrix M, d = M @ x, S = M.T @ (n / d), the stopping
rule as defined; parametrised by dtype (float64, np.longdouble) and by a permutation of the classes.  Where C * n_colors is large the two products are taken
over M's index lists instead of the dense matrix (the same sums in index order: a dense longdouble product of 20000 x 4096 takes minutes).

Bounds.  One iteration: both sides sum non-negative terms, at most n_colors for a denominator and C for a column, so two implementations differ by at most
RTOL1 = 4 (C + n_colors + 4) 2^-53 relative to the value (2 sides, x 2 for second order); the same bound, as an absolute one scaled by sum n_j |log(d_j / N)|,
holds for the log-likelihood.  Many iterations: the tolerance is MEASURED, not chosen -- D = the largest |a - b| / max(|b|, 1) between the float64 model under
three random class orders and the longdouble model, on that very case; allowed is 16 D and never below RTOL1 (another summation order moves the result by about
D itself, the rest is for contraction into fma and for log)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import finito_amd as fa
from tests.test_colors_host import pack, words_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE_LIMIT = 1 << 22


def rtol1(n_classes, n_colors):
    return 4.0 * (n_classes + n_colors + 4) * 2.0 ** -53


def unpack(rows, n_colors):
    """the boolean C x n_colors matrix of rows uint64[C, W]"""
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, words_of(n_colors))
    bits = np.unpackbits(rows.view(np.uint8).reshape(len(rows), -1), axis=1, bitorder="little")   # (little-endian words: byte b of a word holds bits 8 b ..)
    return bits[:, :n_colors].astype(bool)


class Model:
    """the definition.  run() returns a dict: alpha, iters, converged, loglik, max_change, trace (ll_t, t < iters), absll (sum n_j |log(d_j / N)| per iteration),
    changes (the largest relative change per iteration)"""

    def __init__(self, rows, reads, n_colors, lengths=None, dtype=np.float64, perm=None):
        M = unpack(rows, n_colors)
        n = np.asarray(reads, dtype=np.uint64)
        if perm is not None:
            M, n = M[perm], n[perm]
        assert len(M) == len(n) and (len(M) == 0 or (M.any(axis=1).all() and (n >= 1).all()))
        self.dt, self.nc, self.C = dtype, n_colors, len(M)
        self.n = n.astype(dtype)
        self.N = dtype(int(n.astype(object).sum())) if len(n) else dtype(0)
        self.len = np.ones(n_colors, dtype=dtype) if lengths is None else np.asarray(lengths, dtype=np.float64).astype(dtype)
        self.dense = M.size <= DENSE_LIMIT
        if self.dense:
            self.M = M.astype(dtype)
        else:
            jj, cc = np.nonzero(M)                                    # class-major: jj ascending, cc ascending inside a class
            self.cc, self.row_start = cc, np.searchsorted(jj, np.arange(self.C))
            o = np.argsort(cc, kind="stable")                         # colour-major: classes ascending inside a colour
            self.jj_by_c, cs = jj[o], cc[o]
            self.cols = np.unique(cs)
            self.col_start = np.searchsorted(cs, self.cols)

    def denoms(self, x):
        return self.M @ x if self.dense else np.add.reduceat(x[self.cc], self.row_start)

    def colsums(self, q):
        if self.dense:
            return self.M.T @ q
        S = np.zeros(self.nc, dtype=self.dt)
        S[self.cols] = np.add.reduceat(q[self.jj_by_c], self.col_start)
        return S

    def run(self, max_iters=1000, tol=1e-6):
        dt = self.dt
        out = dict(alpha=np.zeros(self.nc, dtype=dt), iters=0, converged=True, loglik=0.0, max_change=0.0, trace=[], absll=[], changes=[])
        if self.C == 0:
            return out
        alpha = np.full(self.nc, self.N / dt(self.nc), dtype=dt)
        out["converged"] = False
        for t in range(max_iters):
            x = alpha / self.len
            d = self.denoms(x)
            lg = np.log(d / self.N)
            out["trace"].append((self.n * lg).sum())
            out["absll"].append(float((self.n * np.abs(lg)).sum()))
            new = x * self.colsums(self.n / d)
            diff, scale = np.abs(new - alpha), np.maximum(new, dt(1))
            out["changes"].append(float((diff / scale).max()))
            alpha = new
            out["iters"] = t + 1
            if (diff <= dt(tol) * scale).all():
                out["converged"] = True
                break
        out.update(alpha=alpha, loglik=out["trace"][-1], max_change=out["changes"][-1], trace=np.array(out["trace"], dtype=dt))
        return out


def random_classes(rng, n_classes, n_colors, max_per_class=8, max_reads=50, skip=()):
    """distinct random classes in np.unique's order: rows uint64[C, W], reads uint64[C]; the colours in `skip` are in no class"""
    allowed = np.array([c for c in range(n_colors) if c not in set(skip)])
    rows = np.zeros((0, words_of(n_colors)), dtype=np.uint64)
    while len(rows) < n_classes:
        want = n_classes - len(rows)
        sets = [rng.choice(allowed, size=min(len(allowed), int(rng.integers(1, max_per_class + 1))), replace=False) for _ in range(want + want // 4 + 4)]
        rows = np.unique(np.concatenate([rows, pack(sets, n_colors)]), axis=0)
        if len(rows) == (1 << min(len(allowed), 62)) - 1:
            break
    rows = rows[np.sort(rng.permutation(len(rows))[:n_classes])]
    return rows, rng.integers(1, max_reads + 1, size=len(rows)).astype(np.uint64)


def measured_tolerance(rows, reads, n_colors, lengths, iters, rng, what):
    """(allowed, the longdouble model's result): D measured on this case as the module's docstring says; the model asserts that nothing stops before `iters`"""
    ref = Model(rows, reads, n_colors, lengths, np.longdouble).run(iters, 0.0)
    assert ref["iters"] == iters and ref["changes"][-1] > 1e-6, "%s: the model's change at iteration %d is %.3g: the case converges too early" % (what, iters, ref["changes"][-1])
    b = ref["alpha"]
    D = 0.0
    for _ in range(3):
        a = Model(rows, reads, n_colors, lengths, np.float64, rng.permutation(len(rows))).run(iters, 0.0)["alpha"]
        D = max(D, float((np.abs(a - b) / np.maximum(np.abs(b), 1)).max()))
    allowed = max(16 * D, rtol1(len(rows), n_colors))
    print("%s: D = %.3g, allowed %.3g" % (what, D, allowed))
    return allowed, ref


def assert_one_iteration(got, want, n_classes, n_colors, what):
    """rule 2: alpha relative to the value, an exactly-zero colour exactly zero, loglik and trace absolute under the scaled bound"""
    r = rtol1(n_classes, n_colors)
    a, b = np.asarray(got.alpha, dtype=np.float64), np.asarray(want["alpha"], dtype=np.float64)
    assert got.iters == 1 and want["iters"] == 1, what
    assert np.array_equal(a == 0.0, b == 0.0), what + ": the colours that are exactly zero"
    assert (np.abs(a - b) <= r * np.abs(b)).all(), "%s: alpha off by %.3g relative, bound %.3g" % (what, (np.abs(a - b) / np.maximum(np.abs(b), 1e-300)).max(), r)
    bound = r * want["absll"][0]
    assert abs(got.loglik - float(want["loglik"])) <= bound, "%s: loglik %r against %r, bound %.3g" % (what, got.loglik, float(want["loglik"]), bound)
    if got.trace is not None:
        assert len(got.trace) == 1 and got.trace[0] == got.loglik, what


def assert_many_iterations(got, ref, allowed, what):
    """rule 3: alpha within `allowed` of the longdouble model relative to max(|value|, 1), the trace within allowed * sum n_j |log(d_j / N)|"""
    a, b = np.asarray(got.alpha, dtype=np.float64), ref["alpha"].astype(np.float64)
    assert got.iters == ref["iters"] and not got.converged, what
    off = float((np.abs(a - b) / np.maximum(np.abs(b), 1)).max())
    assert off <= allowed, "%s: alpha off by %.3g, allowed %.3g" % (what, off, allowed)
    assert np.array_equal(a == 0.0, b == 0.0), what
    if got.trace is not None:
        t = np.abs(np.asarray(got.trace) - ref["trace"].astype(np.float64))
        assert len(got.trace) == ref["iters"] and (t <= allowed * np.array(ref["absll"])).all(), "%s: the trace is off by %.3g" % (what, t.max())
    assert abs(got.loglik - float(ref["loglik"])) <= allowed * ref["absll"][-1], what


def assert_sum_and_trace(alpha, trace, n_reads, absll, n_classes, n_colors, what):
    r = rtol1(n_classes, n_colors)
    assert abs(float(np.asarray(alpha, dtype=np.float64).sum()) - n_reads) <= r * n_reads, "%s: alpha sums to %r, N = %d" % (what, float(alpha.sum()), n_reads)
    tr = np.asarray(trace, dtype=np.float64)
    assert (tr[1:] >= tr[:-1] - r * np.asarray(absll[1:])).all(), what + ": the log-likelihood decreases"


TWO = (pack([[0], [1], [0, 1]], 2), np.array([30, 10, 40], dtype=np.uint64))   # {A}: 30, {B}: 10, {A, B}: 40


# ---- 1. guards on the model itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_model_closed_forms(dtype):
    # singleton classes only: alpha_c = n_c after one iteration
    n = np.array([7, 1, 1 << 40, 12], dtype=np.uint64)
    m = Model(pack([[0], [2], [3], [5]], 6), n, 6, None, dtype, np.array([2, 0, 3, 1])).run(5, 1e-9)
    assert np.array_equal(m["alpha"], np.array([7, 0, 1, 1 << 40, 0, 12], dtype=dtype)) and m["iters"] == 2 and m["converged"]
    # two colours: the map is exactly linear, alpha_A' = 30 + 40 alpha_A / 80, rate 0.5, fixed point 60; at the stop the remaining error is at most the last step
    m = Model(*TWO, 2, None, dtype).run(1000, 1e-9)
    assert m["converged"] and m["iters"] == 30 and abs(float(m["alpha"][0]) - 60) <= 2 * 1e-9 * 60 and abs(float(m["alpha"][0]) - 59.99999998) < 2e-8
    assert abs(float(m["alpha"][1]) - 20) <= 2 * 1e-9 * 60
    assert_sum_and_trace(m["alpha"], m["trace"], 80, m["absll"], 3, 2, "two colours")


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
@pytest.mark.parametrize("n_classes,n_colors", [(300, 5), (3000, 130), (2000, 4096)])
def test_model_sum_and_monotone_trace(dtype, n_classes, n_colors):
    rng = np.random.default_rng(2400 + n_colors)
    rows, reads = random_classes(rng, n_classes, n_colors, skip=(1,))
    lens = rng.uniform(0.5, 2000, n_colors)
    perm = rng.permutation(len(rows))
    m = Model(rows, reads, n_colors, lens, dtype, perm).run(40, 0.0)
    assert m["alpha"][1] == 0 and m["iters"] == 40
    assert_sum_and_trace(m["alpha"], m["trace"], int(reads.sum()), m["absll"], len(rows), n_colors, "%d x %d" % (n_classes, n_colors))
    if n_colors == 4096:   # the index-list form of the two products is the dense one
        assert not Model(rows, reads, n_colors, lens, dtype).dense
        small = Model(rows[:500], reads[:500], n_colors, lens, dtype)
        assert small.dense
        x = rng.uniform(0, 3, n_colors).astype(dtype); q = rng.uniform(0, 3, 500).astype(dtype)
        d0, s0 = small.denoms(x), small.colsums(q)
        small.dense = False
        jj, cc = np.nonzero(unpack(rows[:500], n_colors))
        o = np.argsort(cc, kind="stable")
        small.cc, small.row_start, small.jj_by_c, small.cols = cc, np.searchsorted(jj, np.arange(500)), jj[o], np.unique(cc)
        small.col_start = np.searchsorted(cc[o], small.cols)
        assert np.allclose(small.denoms(x).astype(np.float64), d0.astype(np.float64), rtol=1e-13) and np.allclose(small.colsums(q).astype(np.float64), s0.astype(np.float64), rtol=1e-13)


# ---- 2. one iteration ------------------------------------------------------------------------------------------------------------------
CASES = [(1, 1), (40, 5), (300, 64), (700, 65), (3000, 130), (2500, 4096)]


@pytest.mark.parametrize("n_classes,n_colors", CASES)
@pytest.mark.parametrize("with_lengths", [False, True])
def test_host_twin_one_iteration(n_classes, n_colors, with_lengths):
    rng = np.random.default_rng(2410 + n_colors + with_lengths)
    rows, reads = random_classes(rng, n_classes, n_colors, skip=(1,) if n_colors > 1 else ())
    reads[0] = 1; reads[-1] = 1 << 40          # reads 1 and 2^40
    lens = rng.uniform(0.5, 2000, n_colors) if with_lengths else None
    perm = rng.permutation(len(rows))
    for dtype in (np.float64, np.longdouble):
        want = Model(rows, reads, n_colors, lens, dtype, perm).run(1, 0.0)
        for threads in (1, 3):
            got = fa.classes_abundance(rows, reads, n_colors, lens, max_iters=1, tol=0.0, trace=True, n_threads=threads)
            assert_one_iteration(got, want, len(rows), n_colors, "%d x %d, %s" % (n_classes, n_colors, dtype.__name__))
            assert got.n_reads == int(reads.astype(object).sum()) and got.n_classes == len(rows) and got.n_unaligned == 0
    if n_colors > 1:
        assert got.alpha[1] == 0.0 and got.theta[1] == 0.0 and got.rho[1] == 0.0
    assert abs(got.theta.sum() - 1) < 1e-9 and abs(got.rho.sum() - 1) < 1e-9
    ln = np.ones(n_colors) if lens is None else lens
    assert np.allclose(got.rho, (got.alpha / ln) / (got.alpha / ln).sum(), rtol=1e-14)


def test_host_twin_does_not_depend_on_the_threads():
    rng = np.random.default_rng(2419)
    rows, reads = random_classes(rng, 9000, 130)
    a = [fa.classes_abundance(rows, reads, 130, max_iters=20, tol=0.0, trace=True, n_threads=t) for t in (1, 2, 7)]
    for b in a[1:]:
        assert np.array_equal(a[0].alpha, b.alpha) and np.array_equal(a[0].trace, b.trace) and a[0].loglik == b.loglik


# ---- 3. fifty iterations ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_classes,n_colors", [(3000, 130), (20000, 4096)])
def test_host_twin_fifty_iterations(n_classes, n_colors):
    rng = np.random.default_rng(2420 + n_colors)
    rows, reads = random_classes(rng, n_classes, n_colors, skip=(1,))
    lens = rng.uniform(0.5, 2000, n_colors)
    allowed, ref = measured_tolerance(rows, reads, n_colors, lens, 50, rng, "%d x %d" % (n_classes, n_colors))
    got = fa.classes_abundance(rows, reads, n_colors, lens, max_iters=50, tol=0.0, trace=True)
    assert_many_iterations(got, ref, allowed, "%d x %d" % (n_classes, n_colors))
    assert_sum_and_trace(got.alpha, got.trace, int(reads.sum()), ref["absll"], len(rows), n_colors, "the host twin")
    assert abs(got.max_change - ref["changes"][-1]) <= 1e-6 * ref["changes"][-1]


def test_host_twin_closed_forms_and_stopping():
    got = fa.classes_abundance(pack([[0], [2], [3], [5]], 6), [7, 1, 1 << 40, 12], 6, max_iters=5, tol=1e-9, trace=True)
    assert np.array_equal(got.alpha, [7, 0, 1, float(1 << 40), 0, 12]) and got.iters == 2 and got.converged and got.max_change == 0.0
    sentinel = np.full(1000, -7.5)
    got = fa.classes_abundance(*TWO, 2, max_iters=1000, tol=1e-9, trace=sentinel)
    assert got.converged and got.iters == 30 and abs(got.alpha[0] - 60) <= 2 * 1e-9 * 60 and abs(got.alpha[1] - 20) <= 2 * 1e-9 * 60
    assert (sentinel[30:] == -7.5).all() and (sentinel[:30] != -7.5).all() and len(got.trace) == 30 and got.loglik == sentinel[29]
    got = fa.classes_abundance(*TWO, 2, max_iters=3, tol=1e-9)
    assert not got.converged and got.iters == 3 and got.trace is None and abs(got.alpha[0] - 57.5) <= 57.5 * rtol1(3, 2) * 3   # 40, 50, 55, 57.5: three iterations under rule 2
    # no classes
    got = fa.classes_abundance(np.zeros((0, 1), dtype=np.uint64), [], 7, trace=True)
    assert np.array_equal(got.alpha, np.zeros(7)) and got.iters == 0 and got.converged and got.loglik == 0.0 and got.n_reads == 0 and len(got.trace) == 0
    assert np.array_equal(got.theta, np.zeros(7)) and np.array_equal(got.rho, np.zeros(7))


# ---- 4. arguments ----------------------------------------------------------------------------------------------------------------------
def test_arguments():
    rows, reads = TWO
    for kw, code in ((dict(max_iters=0), fa.FIN_EINVAL), (dict(max_iters=100001), fa.FIN_ELIMIT), (dict(tol=-1e-9), fa.FIN_EINVAL), (dict(tol=float("nan")), fa.FIN_EINVAL)):
        with pytest.raises(fa.FinitoError) as e:
            fa.classes_abundance(rows, reads, 2, **kw)
        assert e.value.code == code, kw
    assert fa.classes_abundance(rows, reads, 2, max_iters=100000, tol=0.5).converged
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(fa.FinitoError) as e:
            fa.classes_abundance(rows, reads, 2, lengths=[1.0, bad])
        assert e.value.code == fa.FIN_EINVAL and "colour 1" in str(e.value), bad
    with pytest.raises(fa.FinitoError) as e:
        fa.classes_abundance(rows, reads, 2, lengths=[1.0, 2.0, 3.0])
    assert e.value.code == fa.FIN_EINVAL
    for nc in (0, 4097):
        with pytest.raises(fa.FinitoError) as e:
            fa.classes_abundance(np.zeros((1, max(1, (nc + 63) // 64)), dtype=np.uint64), [1], nc)
        assert e.value.code == fa.FIN_ELIMIT
    stray = rows.copy(); stray[2, 0] |= np.uint64(4)
    for r, n in ((stray, reads), (np.array([[1], [0]], dtype=np.uint64), [3, 4]), (rows, [30, 0, 40])):   # a stray bit, an empty row, a class of no reads
        with pytest.raises(fa.FinitoError) as e:
            fa.classes_abundance(r, n, 2)
        assert e.value.code == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError):
        fa.classes_abundance(rows, reads[:2], 2)
    # the C entry point makes the same checks by itself
    L = fa.lib()
    u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    alpha = np.zeros(2); info = fa.AbundanceInfo()
    call = lambda lens, mi, tol, nc=2: L.fin_classes_abundance(rows.ctypes.data_as(u64p), reads.ctypes.data_as(u64p), 3, nc, lens.ctypes.data_as(f64p) if lens is not None else None,
                                                               mi, tol, alpha.ctypes.data_as(f64p), None, C.byref(info), 1)
    assert call(None, 0, 1e-6) == fa.FIN_EINVAL and call(None, 100001, 1e-6) == fa.FIN_ELIMIT and call(None, 10, -1.0) == fa.FIN_EINVAL
    assert call(None, 10, float("nan")) == fa.FIN_EINVAL and call(None, 10, 1e-6, 0) == fa.FIN_ELIMIT and call(None, 10, 1e-6, 4097) == fa.FIN_ELIMIT
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(np.array([bad, 1.0]), 10, 1e-6) == fa.FIN_EINVAL
    assert call(np.array([2.0, 1.0]), 10, 1e-6) == fa.FIN_OK and info.iters == 10 and info.n_reads == 80
    assert L.fin_classes_abundance(rows.ctypes.data_as(u64p), reads.ctypes.data_as(u64p), 3, 2, None, 10, 1e-6, None, None, None, 1) == fa.FIN_EINVAL


# ---- 5. symbols ------------------------------------------------------------------------------------------------------------------------
def test_header_and_library_have_both_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "finito_amd.h")).read(), flags=re.S)
    for name in ("fin_eqclasses_abundance", "fin_classes_abundance"):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(fa.lib(), name)
    assert "fin_abundance_info" in src and C.sizeof(fa.AbundanceInfo) == 48
    assert fa.lib().fin_set_option(b"ab_chunk", 64) == 0 and fa.lib().fin_set_option(b"ab_chunk", -1) != 0 and fa.lib().fin_set_option(b"ab_chunk", 0) == 0
