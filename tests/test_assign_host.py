"""Reads assigned to references from per-colour weights (include/finito_amd.h: fin_rows_assign, the host twin of fin_assign_rows) against a
NUMPY MODEL of the definition, written here and never the library.  All expectations are exact.

Two weight families.  DYADIC weights m * 2^-e with small m: every sum of them is exact in any order, so the model takes d as a plain sum (np.bincount) and is
independent of the stated order; thresholds are chosen so that x[c] == thr[c] * d holds with equality, which must assign.  RANDOM doubles: the model folds in the
stated order -- s_w over the set bits of word w ascending from 0.0, then v = v[:h] + v[h:] over the power of two at or above W -- and host twin and model must
agree bit for bit."""
import numpy as np
import pytest

import finito_amd as fa
from tests.test_colors_host import pack, words_of

N_COLORS = [1, 5, 64, 65, 130, 4096]
NO = fa.FIN_NO_COLOR


def unpack_bool(rows, n_colors):
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, words_of(n_colors))
    bits = np.unpackbits(rows.view(np.uint8).reshape(len(rows), 8 * words_of(n_colors)), axis=1, bitorder="little")
    return bits[:, :n_colors].astype(bool)


def pack_pairs(jj, cc, n, n_colors):
    """uint64[n, W] with bit cc[i] of row jj[i] set"""
    out = np.zeros((n, words_of(n_colors)), dtype=np.uint64)
    np.bitwise_or.at(out, (jj, cc >> 6), np.uint64(1) << (cc & 63).astype(np.uint64))
    return out


def model(rows, n_colors, x, thr, fold):
    """the definition: (assigned rows, heads, assigned, sole, counters).  fold: d in the stated order; else a plain sum (exact weights only)"""
    x = np.asarray(x, dtype=np.float64)
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float64), (n_colors,))
    M = unpack_bool(rows, n_colors)
    n, W = len(M), words_of(n_colors)
    jj, cc = np.nonzero(M)                  # row-major: cc ascending inside a row
    if fold:
        wp2 = 1
        while wp2 < W:
            wp2 *= 2
        s = np.zeros((n, wp2), dtype=np.float64)
        for c in np.unique(cc):             # ascending: word c >> 6 gains x[c] where the bit is set (+ 0.0 elsewhere changes nothing)
            s[:, c >> 6] = s[:, c >> 6] + np.where(M[:, c], x[c], 0.0)
        while s.shape[1] > 1:
            h = s.shape[1] // 2
            s = s[:, :h] + s[:, h:]
        d = s[:, 0]
    else:
        d = np.bincount(jj, weights=x[cc], minlength=n).astype(np.float64)
    keep = (x[cc] > 0) & (d[jj] > 0) & (x[cc] >= thr[cc] * d[jj])
    aj, ac = jj[keep], cc[keep]
    arows = pack_pairs(aj, ac, n, n_colors)
    heads = np.zeros(n, dtype=fa.READ_ASSIGN_DTYPE)
    heads["n_assigned"] = np.bincount(aj, minlength=n)
    best = np.full(n, NO, dtype=np.uint32)
    if len(jj):
        o = np.lexsort((cc, -x[cc], jj))    # per row: the largest weight first, the smaller colour first among equal ones
        first = np.concatenate([[True], jj[o][1:] != jj[o][:-1]])
        best[jj[o][first]] = cc[o][first]
    best[~(d > 0)] = NO
    heads["best"] = best
    assigned = np.bincount(ac, minlength=n_colors).astype(np.uint64)
    one = heads["n_assigned"][aj] == 1
    sole = np.bincount(ac[one], minlength=n_colors).astype(np.uint64)
    ne = M.any(axis=1)
    counters = np.array([n, int((~ne).sum()), int((ne & (heads["n_assigned"] == 0)).sum()), int((heads["n_assigned"] >= 2).sum())], dtype=np.uint64)
    return arows, heads, assigned, sole, counters


def dyadic_weights(rng, n_colors):
    """m * 2^-e, m in 0 .. 7: sums of up to 4096 of them are exact; colour 1 (where there is one) weighs nothing, neighbours tie"""
    x = rng.integers(1, 8, n_colors).astype(np.float64) * 2.0 ** -rng.integers(0, 6, n_colors)
    if n_colors > 1:
        x[1] = 0.0
    if n_colors > 4:
        x[4] = x[3]
    return x


def random_weights(rng, n_colors):
    x = rng.uniform(0.0, 1.0, n_colors) * 10.0 ** rng.integers(-6, 4, n_colors)
    if n_colors > 1:
        x[1] = 0.0
    if n_colors > 4:
        x[4] = x[3]
    return x


def rows_of_interest(n_colors):
    """a zero row, single colours, only the last bit of the last word, a full row, rows whose weights are all 0, ties"""
    top = n_colors - 1
    sets = [[], [0], [top], list(range(n_colors)), [0, top]]
    if n_colors > 1:
        sets += [[1], [0, 1]]               # x[1] = 0: d = 0 for {1}
    if n_colors > 4:
        sets += [[3, 4], [4, 3, top], [1, 3, 4]]   # x[3] == x[4]: best is 3
    return pack(sets, n_colors)


def random_rows(rng, n, n_colors, max_set=8):
    """n rows of 1 .. max_set colours, some empty, and the rows of interest in front (n permitting)"""
    sizes = rng.integers(1, min(max_set, n_colors) + 1, n)
    jj = np.repeat(np.arange(n), sizes)
    cc = rng.integers(0, n_colors, len(jj))
    rows = pack_pairs(jj, cc, n, n_colors)
    rows[rng.random(n) < 0.1] = 0
    special = rows_of_interest(n_colors)[:n]
    rows[: len(special)] = special
    return rows


def assert_same(got, want, what):
    names = ("assigned rows", "heads", "assigned", "sole", "counters")
    for g, w, name in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), "%s: %s differ" % (what, name)


def assert_identities(rows, res, what):
    arows, heads, assigned, sole, counters = res
    na = heads["n_assigned"].astype(np.int64)
    assert int(counters[0]) == len(rows) == int(counters[1]) + int(counters[2]) + int((na >= 1).sum()), what
    assert int(assigned.sum()) == int(na.sum()) and int(sole.sum()) == int((na == 1).sum()) and int(counters[3]) == int((na >= 2).sum()), what
    assert not (arows & ~rows).any(), what + ": an assigned colour outside the row"


@pytest.mark.parametrize("n_colors", N_COLORS)
def test_dyadic_weights_against_the_plain_model(n_colors):
    rng = np.random.default_rng(3200 + n_colors)
    x = dyadic_weights(rng, n_colors)
    rows = random_rows(rng, 300, n_colors)
    for thr in (0.0, 1.0, 0.5, 0.25, rng.integers(0, 9, n_colors) / 8.0):
        what = "%d colours, thr %s" % (n_colors, thr if np.isscalar(thr) else "per colour")
        got = fa.rows_assign(rows, n_colors, x, thr)
        assert_same(got, model(rows, n_colors, x, thr, fold=False), what)
        assert_same(got, model(rows, n_colors, x, thr, fold=True), what + " (folded)")
        assert_identities(rows, got, what)


@pytest.mark.parametrize("n_colors", N_COLORS)
def test_a_threshold_met_with_equality_assigns(n_colors):
    """rows {a, b} with x[a] = 3/4, x[b] = 1/4, d = 1: thr[a] = 3/4 and thr[b] = 1/4 are met exactly; one step above and the colour is not assigned"""
    a, b = 0, n_colors - 1
    x = np.ones(n_colors)
    if n_colors == 1:
        rows = pack([[0]], 1)
        got = fa.rows_assign(rows, 1, [0.75], 1.0)
        assert got[0][0, 0] == 1 and got[1][0]["n_assigned"] == 1 and got[1][0]["best"] == 0
        return
    x[a], x[b] = 0.75, 0.25
    rows = pack([[a, b]], n_colors)
    thr = np.zeros(n_colors)
    thr[a], thr[b] = 0.75, 0.25
    arows, heads, assigned, sole, counters = fa.rows_assign(rows, n_colors, x, thr)
    assert arows.tobytes() == rows.tobytes() and heads[0]["n_assigned"] == 2 and heads[0]["best"] == a and counters.tolist() == [1, 0, 0, 1]
    thr[b] = np.nextafter(0.25, 1.0)
    arows, heads, assigned, sole, counters = fa.rows_assign(rows, n_colors, x, thr)
    assert arows.tobytes() == pack([[a]], n_colors).tobytes() and heads[0]["n_assigned"] == 1 and sole[a] == 1 and assigned[b] == 0 and counters.tolist() == [1, 0, 0, 0]
    assert_same((arows, heads, assigned, sole, counters), model(rows, n_colors, x, thr, fold=False), "one step above")


@pytest.mark.parametrize("n_colors", N_COLORS)
def test_random_doubles_against_the_folded_model(n_colors):
    rng = np.random.default_rng(3300 + n_colors)
    x = random_weights(rng, n_colors)
    rows = random_rows(rng, 300, n_colors, max_set=min(n_colors, 40))
    for thr in (0.0, 1.0, 0.5, rng.uniform(0, 1, n_colors)):
        what = "%d colours, thr %s" % (n_colors, thr if np.isscalar(thr) else "per colour")
        got = fa.rows_assign(rows, n_colors, x, thr)
        assert_same(got, model(rows, n_colors, x, thr, fold=True), what)
        assert_identities(rows, got, what)


@pytest.mark.parametrize("n_colors", N_COLORS)
def test_rows_of_interest(n_colors):
    rng = np.random.default_rng(3400 + n_colors)
    x = dyadic_weights(rng, n_colors)
    rows = rows_of_interest(n_colors)
    arows, heads, assigned, sole, counters = got = fa.rows_assign(rows, n_colors, x, 0.0)
    assert_same(got, model(rows, n_colors, x, 0.0, fold=False), "rows of interest")
    top = n_colors - 1
    assert not arows[0].any() and heads[0].tolist() == (0, NO)                    # the zero row: unaligned
    assert heads[1].tolist() == (1, 0) and heads[2].tolist() == (1, top)          # single colours; the last bit of the last word
    assert int(counters[1]) == 1
    if n_colors > 1:
        assert heads[5].tolist() == (0, NO) and not arows[5].any()                # weights all 0: d = 0, unassigned, no best
        assert int(counters[2]) == 1
        assert arows[6].tobytes() == pack([[0]], n_colors)[0].tobytes()           # thr = 0 still wants x > 0
        full = np.nonzero(x > 0)[0]
        assert arows[3].tobytes() == pack([full], n_colors)[0].tobytes() and heads[3]["n_assigned"] == len(full)
    if n_colors > 4:
        assert heads[7]["best"] == 3 and heads[9]["best"] == 3                    # x[3] == x[4]: the smaller colour
    # thr = 1: only a colour that is all of d
    arows1, heads1, _, _, _ = fa.rows_assign(rows, n_colors, x, 1.0)
    assert_same(fa.rows_assign(rows, n_colors, x, 1.0), model(rows, n_colors, x, 1.0, fold=False), "thr = 1")
    assert heads1[1]["n_assigned"] == 1 and (n_colors == 1 or heads1[4]["n_assigned"] == 0)
    # every thr = 0 and every x > 0: A = R
    xp = np.where(x > 0, x, 1.0)
    rr = random_rows(rng, 200, n_colors)
    assert fa.rows_assign(rr, n_colors, xp, 0.0)[0].tobytes() == rr.tobytes()


@pytest.mark.parametrize("n_colors", [5, 130, 4096])
def test_the_result_does_not_depend_on_the_threads(n_colors):
    rng = np.random.default_rng(3500 + n_colors)
    x = random_weights(rng, n_colors)
    rows = random_rows(rng, 1001, n_colors)
    one = fa.rows_assign(rows, n_colors, x, 0.3, n_threads=1)
    for t in (2, 3, 7, 16, 0):
        assert_same(fa.rows_assign(rows, n_colors, x, 0.3, n_threads=t), one, "%d threads" % t)
    empty = fa.rows_assign(np.zeros((0, words_of(n_colors)), dtype=np.uint64), n_colors, x, 0.3)
    assert len(empty[0]) == 0 and len(empty[1]) == 0 and not empty[2].any() and not empty[3].any() and empty[4].tolist() == [0, 0, 0, 0]


def test_refusals():
    rows = pack([[0, 2]], 5)
    ok = np.ones(5)
    for bad, word in ((-1.0, "weight"), (np.nan, "weight"), (np.inf, "weight")):
        w = ok.copy(); w[3] = bad
        with pytest.raises(fa.FinitoError) as e:
            fa.rows_assign(rows, 5, w, 0.5)
        assert e.value.code == fa.FIN_EINVAL and "weight of colour 3" in str(e.value)
    for bad in (-0.001, 1.001, np.nan, np.inf):
        t = np.full(5, 0.5); t[2] = bad
        with pytest.raises(fa.FinitoError) as e:
            fa.rows_assign(rows, 5, ok, t)
        assert e.value.code == fa.FIN_EINVAL and "threshold of colour 2" in str(e.value)
    with pytest.raises(fa.FinitoError) as e:
        fa.rows_assign(rows, 5, ok, 1.5)    # a scalar is broadcast, then checked
    assert e.value.code == fa.FIN_EINVAL and "threshold of colour 0" in str(e.value)
    for call, code, word in ((lambda: fa.rows_assign(rows, 5, np.ones(4), 0.5), fa.FIN_EINVAL, "4 weights for 5 colours"),
                             (lambda: fa.rows_assign(rows, 5, ok, np.ones(6)), fa.FIN_EINVAL, "6 thresholds for 5 colours"),
                             (lambda: fa.rows_assign(rows, 0, [], 0.5), fa.FIN_ELIMIT, "n_colors is 1 .. 4096"),
                             (lambda: fa.rows_assign(rows, 4097, np.ones(4097), 0.5), fa.FIN_ELIMIT, "n_colors is 1 .. 4096")):
        with pytest.raises(fa.FinitoError) as e:
            call()
        assert e.value.code == code and word in str(e.value)
    stray = pack([[0]], 5)
    stray[0, 0] |= np.uint64(1) << np.uint64(5)
    with pytest.raises(fa.FinitoError) as e:
        fa.rows_assign(stray, 5, ok, 0.5)
    assert e.value.code == fa.FIN_EINVAL and "bit at or above n_colors" in str(e.value)
    # the C function by itself makes the same refusals (it has no message)
    import ctypes as C
    L = fa.lib()
    u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    w = ok.copy(); w[1] = -2.0
    t = np.full(5, 0.5)
    assert L.fin_rows_assign(rows.ctypes.data_as(u64p), 1, 5, w.ctypes.data_as(f64p), t.ctypes.data_as(f64p), None, None, None, None, None, 1) == fa.FIN_EINVAL
    t[4] = 2.0
    assert L.fin_rows_assign(rows.ctypes.data_as(u64p), 1, 5, ok.ctypes.data_as(f64p), t.ctypes.data_as(f64p), None, None, None, None, None, 1) == fa.FIN_EINVAL
    t[4] = 1.0
    assert L.fin_rows_assign(rows.ctypes.data_as(u64p), 1, 5, ok.ctypes.data_as(f64p), t.ctypes.data_as(f64p), None, None, None, None, None, 1) == fa.FIN_OK


def test_abundance_weights():
    rows, reads = pack([[0], [0, 1], [1]], 2), np.array([6, 3, 1], dtype=np.uint64)
    lens = np.array([2.0, 4.0])
    ab = fa.classes_abundance(rows, reads, 2, lens, max_iters=50)
    assert ab.weights().tobytes() == (ab.alpha / lens).tobytes()
    assert fa.classes_abundance(rows, reads, 2, max_iters=50).weights().tobytes() == fa.classes_abundance(rows, reads, 2, max_iters=50).alpha.tobytes()
