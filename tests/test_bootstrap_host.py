"""Bootstrap replicates of the abundance estimate (include/finito_amd.h: fin_classes_resample, fin_classes_bootstrap, the host twins of fin_eqclasses_bootstrap;
DESIGN.md 4.18) against a PYTHON RESTATEMENT of the definition, written here and never the library: Philox4x32-10 and the row hash in Python integers, the
thresholds T_k recomputed with `decimal`, the counts as sums of multiplicities.  A numpy form of the same generator (uint64 products of 32-bit values, exact)
does the large classes; it is checked against the integer form first.  tests/test_bootstrap.py imports the restatement from here."""
import ctypes as C
import decimal
import os
import re

import numpy as np
import pytest

import finito_amd as fa
from tests.test_abundance_host import TWO, random_classes
from tests.test_colors_host import pack, words_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
T_HEX = "5e2d58d8, bc5ab1b1, eb715e1d, fb239797, ff1025f5, ffd90f3b, fffa8b71, ffff540c, ffffed1f, fffffe21, ffffffd4, fffffffc, ffffffff"
T = [int(x, 16) for x in T_HEX.split(", ")]
N_LIST = [1, 2, 3, 4, 5, 4095, 4096, 4097, 8193, 1 << 20]


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def philox(ctr, key):
    """Philox4x32-10 in Python integers: ctr and key are lists of 4 and 2 words"""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


def philox_np(c0, c1, c2, c3, k0, k1):
    """the same over uint64 arrays that hold 32-bit values; returns the four output words"""
    c0, c1, c2, c3 = [np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3)]
    k0, k1, m = np.uint64(k0), np.uint64(k1), np.uint64(M32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return c0, c1, c2, c3


def mix(x):
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def row_hash(row):
    """the 64-bit hash of a row of W words: the equivalence-class table's, before it is narrowed to a tag"""
    h = 0
    for i, w in enumerate(row):
        h ^= mix((int(w) + (i + 1) * 0x9E3779B97F4A7C15) & M64)
    return h


def mult(u):
    return sum(1 for t in T if u >= t)


def class_count_int(h, n, seed, b):
    """n_j^(b) in Python integers, for small n"""
    total = 0
    for i in range((n + 3) // 4):
        out = philox([h & M32, h >> 32, i & M32, (i >> 32) | (b << 8)], [seed & M32, seed >> 32])
        total += sum(mult(out[m]) for m in range(4) if 4 * i + m < n)
    return total


def class_count(h, n, seed, b):
    """n_j^(b) through the numpy generator; b may be an array: one count per replicate"""
    b = np.atleast_1d(np.asarray(b, dtype=np.uint64))
    i = np.arange((n + 3) // 4, dtype=np.uint64)
    c3 = (i >> np.uint64(32))[None, :] | (b << np.uint64(8))[:, None]
    out = philox_np(np.uint64(h & M32), np.uint64(h >> 32), np.broadcast_to(i & np.uint64(M32), c3.shape), c3, seed & M32, seed >> 32)
    u = np.stack(out, axis=-1).reshape(len(b), -1)[:, :n]                    # word m of block i is read 4 i + m
    x = np.searchsorted(np.array(T, dtype=np.uint64), u.reshape(-1), side="right").reshape(u.shape)   # the number of k with T_k <= u
    return x.sum(axis=1).astype(np.uint64)


def counts_ref(rows, reads, seed, b):
    """the resampled counts of replicate b for classes {row, reads}: uint64[C]"""
    return np.array([int(class_count(row_hash(r), int(n), seed, b)[0]) for r, n in zip(np.asarray(rows, dtype=np.uint64), reads)], dtype=np.uint64)


def classes_of_interest(rng, W, n_list=N_LIST):
    """one class per n of n_list, distinct random rows of W words (n_colors = 64 W)"""
    rows, _ = random_classes(rng, len(n_list), 64 * W, max_per_class=8)
    return rows, np.array(n_list, dtype=np.uint64)


# ---- 1. the restatement itself ---------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    hx = lambda s: [int(x, 16) for x in s.split()]
    assert philox([0] * 4, [0] * 2) == hx("6627e8d5 e169c58d bc57ac4c 9b00dbd8")
    assert philox([M32] * 4, [M32] * 2) == hx("408f276d 41c83b0e a20bc7c6 6d5451fd")
    assert philox(hx("243f6a88 85a308d3 13198a2e 03707344"), hx("a4093822 299f31d0")) == hx("d16cfe09 94fdcceb 5001e420 24126ea1")
    rng = np.random.default_rng(2600)
    ctr, key = rng.integers(0, 1 << 32, size=(50, 4), dtype=np.uint64), rng.integers(0, 1 << 32, size=2, dtype=np.uint64)
    got = np.stack(philox_np(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], int(key[0]), int(key[1])), axis=1)
    assert np.array_equal(got, np.array([philox([int(x) for x in c], [int(k) for k in key]) for c in ctr], dtype=np.uint64))


def test_thresholds_recomputed_with_decimal():
    decimal.getcontext().prec = 80
    one = decimal.Decimal(1)
    e, term = decimal.Decimal(0), one
    for i in range(1, 70):
        e += term
        term /= i
    cdf, term, want = decimal.Decimal(0), one, []
    for k in range(13):
        cdf += term
        term /= k + 1
        want.append(int((cdf / e * (1 << 32)).to_integral_value(rounding=decimal.ROUND_FLOOR)))
    assert want == T and T[12] == M32
    assert [mult(u) for u in (0, T[0] - 1, T[0], T[1], T[12] - 1, M32)] == [0, 0, 1, 2, 12, 13]


def test_the_numpy_counts_are_the_integer_counts():
    for n in (1, 2, 3, 4, 5, 9, 130):
        for b, seed, h in ((0, 0, 0), (255, 1, M64), (256, 1 << 32, 0x0123456789ABCDEF), (4095, M64, 77)):
            assert int(class_count(h, n, seed, b)[0]) == class_count_int(h, n, seed, b), (n, b, seed)
    assert np.array_equal(class_count(77, 130, 5, [0, 3, 4095]), [class_count_int(77, 130, 5, b) for b in (0, 3, 4095)])


# ---- 2. the host twin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 3, 64])
def test_host_twin_is_the_restatement(W):
    rng = np.random.default_rng(2610 + W)
    rows, reads = classes_of_interest(rng, W)
    assert list(reads) == N_LIST
    for seed in (0, 1, 1 << 32, M64):
        for b in (0, 1, 255, 256, 4095):
            want = counts_ref(rows, reads, seed, b)
            for threads in (1, 3):
                got = fa.classes_resample(rows, reads, 64 * W, seed=seed, b=b, n_threads=threads)
                assert np.array_equal(got, want), "W = %d, seed %d, b %d: %r against %r" % (W, seed, b, got, want)


def test_order_free():
    rng = np.random.default_rng(2620)
    rows, reads = random_classes(rng, 500, 130, max_reads=9000)
    a = fa.classes_resample(rows, reads, 130, seed=9, b=2)
    perm = rng.permutation(500)
    assert np.array_equal(fa.classes_resample(rows[perm], reads[perm], 130, seed=9, b=2), a[perm])
    assert np.array_equal(a[:20], counts_ref(rows[:20], reads[:20], 9, 2))


def test_replicates_are_not_copies():
    row, n = pack([[3, 70]], 130), [1000]
    get = lambda seed, b: int(fa.classes_resample(row, n, 130, seed=seed, b=b)[0])
    assert get(5, 0) != get(5, 1) and get(5, 0) != get(6, 0)
    assert get(5, 0) == int(class_count(row_hash(row[0]), 1000, 5, 0)[0]) and get(6, 1) == int(class_count(row_hash(row[0]), 1000, 6, 1)[0])


def test_distribution_at_a_fixed_seed():
    """one class of 1000 reads, replicates 0 .. 1999 under seed 2630 (the first seed tried: the restatement gave a mean and a variance inside both bounds):
    a count is a sum of 1000 Poisson(1) draws, so its mean and variance are 1000"""
    row = pack([[0, 5]], 6)
    c = class_count(row_hash(row[0]), 1000, 2630, np.arange(2000)).astype(np.float64)
    print("mean %.3f, variance %.1f" % (c.mean(), c.var(ddof=1)))
    assert abs(c.mean() - 1000) <= 5 * np.sqrt(1000 / 2000)
    assert abs(c.var(ddof=1) - 1000) <= 0.2 * 1000
    for b in (0, 1, 1999):
        assert int(fa.classes_resample(row, [1000], 6, seed=2630, b=b)[0]) == int(c[b])


# ---- 3. classes_bootstrap --------------------------------------------------------------------------------------------------------------
def assert_replicates_are_abundances(B, rows, reads, n_colors, seed, lens, max_iters, tol):
    for b in range(len(B.alpha)):
        counts = counts_ref(rows, reads, seed, b)
        nz = counts > 0
        want = fa.classes_abundance(rows[nz], counts[nz], n_colors, lens, max_iters=max_iters, tol=tol)
        assert int(B.n_reads[b]) == int(counts.sum()) and np.array_equal(B.alpha[b], want.alpha) and B.iters[b] == want.iters and B.converged[b] == want.converged, b


def test_classes_bootstrap_is_classes_abundance_over_each_replicate():
    rng = np.random.default_rng(2640)
    n_colors = 130
    rows, reads = random_classes(rng, 400, n_colors, max_reads=3)            # counts this small leave classes empty in every replicate
    lens = rng.uniform(0.5, 2000, n_colors)
    B = fa.classes_bootstrap(rows, reads, n_colors, 4, seed=11, lengths=lens, max_iters=30, tol=1e-6)
    assert any((counts_ref(rows, reads, 11, b) == 0).any() for b in range(4))
    assert_replicates_are_abundances(B, rows, reads, n_colors, 11, lens, 30, 1e-6)
    point = fa.classes_abundance(rows, reads, n_colors, lens, max_iters=30, tol=1e-6)
    assert np.array_equal(B.point.alpha, point.alpha) and B.point.iters == point.iters and B.point.loglik == point.loglik and B.point.n_reads == int(reads.sum())
    assert B.seed == 11 and B.alpha.shape == (4, n_colors) and np.array_equal(B.mean, B.alpha.mean(axis=0)) and np.array_equal(B.sd, B.alpha.std(axis=0, ddof=1))
    nr = B.n_reads.astype(np.float64)
    assert np.array_equal(B.theta, B.alpha / nr[:, None]) and np.allclose(B.theta.sum(axis=1), 1, rtol=1e-12)
    one = fa.classes_bootstrap(rows, reads, n_colors, 1, seed=11, lengths=lens, max_iters=30)
    assert np.array_equal(one.alpha[0], B.alpha[0]) and np.array_equal(one.sd, np.zeros(n_colors))   # replicate b does not depend on n_boot
    for threads in (1, 3):
        again = fa.classes_bootstrap(rows, reads, n_colors, 4, seed=11, lengths=lens, max_iters=30, tol=1e-6, n_threads=threads)
        assert np.array_equal(again.alpha, B.alpha) and np.array_equal(again.n_reads, B.n_reads)


def test_empty_replicates():
    """N = 1: a replicate is empty where the single read's multiplicity is 0, which the restatement says happens among b < 16 under seed 2650"""
    row = pack([[1]], 3)
    counts = [int(class_count(row_hash(row[0]), 1, 2650, b)[0]) for b in range(16)]
    assert 0 in counts and any(counts), counts
    B = fa.classes_bootstrap(row, [1], 3, 16, seed=2650, max_iters=10)
    assert [int(x) for x in B.n_reads] == counts
    for b, c in enumerate(counts):
        if c == 0:
            assert not B.alpha[b].any() and B.iters[b] == 0 and B.converged[b] and not B.theta[b].any()
        else:
            assert np.array_equal(B.alpha[b], [0.0, float(c), 0.0]) and B.iters[b] >= 1
    # no classes at all: the point estimate as classes_abundance gives it, every replicate empty
    B = fa.classes_bootstrap(np.zeros((0, 1), dtype=np.uint64), [], 7, 3)
    assert not B.alpha.any() and not B.n_reads.any() and not B.iters.any() and B.converged.all() and B.point.iters == 0 and B.point.converged and not B.sd.any()


def test_refusals_carry_their_codes():
    rows, reads = TWO
    for nb, code in ((0, fa.FIN_EINVAL), (-1, fa.FIN_EINVAL), (4097, fa.FIN_ELIMIT)):
        with pytest.raises(fa.FinitoError) as e:
            fa.classes_bootstrap(rows, reads, 2, nb)
        assert e.value.code == code and "n_boot" in str(e.value)
    for kw, code in ((dict(max_iters=0), fa.FIN_EINVAL), (dict(max_iters=100001), fa.FIN_ELIMIT), (dict(tol=-1.0), fa.FIN_EINVAL), (dict(lengths=[1.0, 0.0]), fa.FIN_EINVAL)):
        with pytest.raises(fa.FinitoError) as e:
            fa.classes_bootstrap(rows, reads, 2, 3, **kw)
        assert e.value.code == code, kw
    stray = rows.copy(); stray[2, 0] |= np.uint64(4)
    for r, n in ((stray, reads), (rows, [30, 0, 40])):
        with pytest.raises(fa.FinitoError) as e:
            fa.classes_bootstrap(r, n, 2, 3)
        assert e.value.code == fa.FIN_EINVAL
    for kw in (dict(b=4096), dict(b=-1)):
        with pytest.raises(fa.FinitoError) as e:
            fa.classes_resample(rows, reads, 2, **kw)
        assert e.value.code == fa.FIN_ELIMIT
    with pytest.raises(fa.FinitoError) as e:
        fa.classes_resample(rows, [1, 1 << 40, 1], 2)
    assert e.value.code == fa.FIN_ELIMIT
    # the C entry points make the same checks by themselves
    L = fa.lib()
    u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    out = fa._BootOut(4, 2)
    call = lambda nb, mi=10: L.fin_classes_bootstrap(rows.ctypes.data_as(u64p), reads.ctypes.data_as(u64p), 3, 2, None, mi, 1e-6, nb, 0, *out.args(), 1)
    assert call(0) == fa.FIN_EINVAL and call(4097) == fa.FIN_ELIMIT and call(4, 0) == fa.FIN_EINVAL and call(4) == fa.FIN_OK and out.n_reads.all()
    counts = np.zeros(3, dtype=np.uint64)
    assert L.fin_classes_resample(rows.ctypes.data_as(u64p), reads.ctypes.data_as(u64p), 3, 2, 0, 4096, counts.ctypes.data_as(u64p), 1) == fa.FIN_ELIMIT
    assert L.fin_classes_resample(rows.ctypes.data_as(u64p), reads.ctypes.data_as(u64p), 3, 0, 0, 0, counts.ctypes.data_as(u64p), 1) == fa.FIN_ELIMIT
    # N n_boot above 2^38, by the argument check alone: the message names both factors
    err = C.create_string_buffer(512)
    assert L.fin_bootstrap_check((1 << 26) + 1, 4096, err, 512) == fa.FIN_ELIMIT and b"67108865" in err.value and b"4096" in err.value and b"2^38" in err.value
    assert L.fin_bootstrap_check(1 << 26, 4096, err, 512) == fa.FIN_OK and L.fin_bootstrap_check(1 << 38, 1, err, 512) == fa.FIN_OK
    assert L.fin_bootstrap_check((1 << 38) + 1, 1, err, 512) == fa.FIN_ELIMIT
    assert L.fin_bootstrap_check(5, 0, err, 512) == fa.FIN_EINVAL and L.fin_bootstrap_check(5, 4097, err, 512) == fa.FIN_ELIMIT and b"n_boot" in err.value


# ---- 4. symbols ------------------------------------------------------------------------------------------------------------------------
def test_header_and_library_have_the_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "finito_amd.h")).read(), flags=re.S)
    for name in ("fin_eqclasses_bootstrap", "fin_classes_resample", "fin_classes_bootstrap", "fin_bootstrap_check"):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(fa.lib(), name)
    for name in ("fin_launch_ab_rowhash", "fin_launch_ab_slabs", "fin_launch_ab_resample"):
        assert hasattr(fa.lib(), name)
    header = open(os.path.join(ROOT, "include", "finito_amd.h")).read()
    assert all("%08x" % t in header for t in T)
    # the row hash has one statement, shared by the table and the bootstrap
    csrc = os.path.join(ROOT, "finito_amd", "csrc")
    has = lambda f: "0xBF58476D1CE4E5B9" in open(os.path.join(csrc, f)).read()
    assert has("fin_rowhash.h") and not has("fin_eqclasses.hip") and not has("fin_bootstrap.hip") and not has("fin_bootrng.h") and not has("fin_capi.cpp")
    assert words_of(130) == 3
