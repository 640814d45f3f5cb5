"""Equivalence classes of pseudoaligned reads, the parts that need no GPU (include/finito_amd.h: fin_rows_eqclasses, fin_eqclasses_color_tally): the host functions
against the definition written in numpy -- np.unique(rows, axis=0, return_counts=True) over the non-empty rows --, tiny cases written out by hand, what is
refused, and the command's usage rules for --eqclasses, --color-report and --eq-max-classes.  Every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from tests.test_colors_host import pack, pack_members, unpack, words_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")
U64P = C.POINTER(C.c_uint64)


def classes_of_rows(rows, n_colors):
    """the definition: (class rows uint64[n, W] in canonical order, reads uint64[n], n_unaligned)"""
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, words_of(n_colors))
    live = rows[rows.any(axis=1)]
    if len(live) == 0:
        return np.zeros((0, rows.shape[1]), dtype=np.uint64), np.zeros(0, dtype=np.uint64), len(rows)
    r, c = np.unique(live, axis=0, return_counts=True)
    return r, c.astype(np.uint64), len(rows) - len(live)


def tally_of(class_rows, class_reads, n_colors):
    """the definition: reads_with[c] = the reads of the classes that contain c; reads_only[c] = the reads of the class {c}"""
    member = unpack(class_rows, n_colors) if len(class_rows) else np.zeros((0, n_colors), dtype=np.int64)
    reads = np.asarray(class_reads, dtype=np.uint64)
    reads_with = np.array([int(reads[member[:, c] == 1].sum()) for c in range(n_colors)], dtype=np.uint64)
    alone = member.sum(axis=1) == 1
    reads_only = np.array([int(reads[alone & (member[:, c] == 1)].sum()) for c in range(n_colors)], dtype=np.uint64)
    return reads_with, reads_only


def assert_classes(got, want, what=""):
    rows, reads, un = got
    wrows, wreads, wun = want
    assert rows.dtype == np.uint64 and reads.dtype == np.uint64 and rows.shape == wrows.shape and reads.shape == wreads.shape, \
        "%s: %d classes, want %d" % (what, len(rows), len(wrows))
    assert un == wun, "%s: %d unaligned, want %d" % (what, un, wun)
    bad = np.nonzero((rows != wrows).any(axis=1) | (reads != wreads))[0]
    assert len(bad) == 0, "%s: %d classes differ, first %d: got %s x %d, want %s x %d" % (what, len(bad), bad[0], rows[bad[0]], reads[bad[0]], wrows[bad[0]], wreads[bad[0]])


def random_rows(rng, n, n_colors, n_distinct, empty_share=0.1):
    """n rows drawn from a pool of n_distinct distinct non-empty rows, skewed so that one class is large; about empty_share of them empty"""
    member = rng.random((n_distinct, n_colors)) < 0.3
    member[np.arange(n_distinct), rng.integers(0, n_colors, n_distinct)] = True
    pool = np.unique(pack_members(member), axis=0)
    pick = np.minimum(rng.integers(0, len(pool), n), rng.integers(0, len(pool), n))
    pick[: n // 3] = 0
    rows = pool[rng.permutation(pick)]
    rows[rng.random(n) < empty_share] = 0
    return rows


@pytest.mark.parametrize("n_colors", [1, 5, 64, 65, 130, 4096])
def test_host_functions_against_numpy(n_colors):
    rng = np.random.default_rng(2100 + n_colors)
    rows = random_rows(rng, 700, n_colors, 40)
    rows[5] = pack([[n_colors - 1]], n_colors)[0]   # the top colour alone
    want = classes_of_rows(rows, n_colors)
    assert want[2] > 0 and want[1].max() > 64 and len(want[0]) == (1 if n_colors == 1 else len(want[0])) and (n_colors == 1 or len(want[0]) > 5)
    got = fa.rows_eqclasses(rows, n_colors)
    assert_classes(got, want, "%d colours" % n_colors)
    assert int(got[1].sum()) + got[2] == len(rows)
    w, o = fa.eqclasses_color_tally(got[0], got[1], n_colors)
    ww, wo = tally_of(want[0], want[1], n_colors)
    assert np.array_equal(w, ww) and np.array_equal(o, wo) and wo[n_colors - 1] >= 1
    # merging two downloads is the same arithmetic: classes of the classes, weighted -- here by adding the rows twice
    twice = fa.rows_eqclasses(np.concatenate([rows, rows]), n_colors)
    assert_classes(twice, (want[0], want[1] * np.uint64(2), 2 * want[2]), "%d colours, twice" % n_colors)


def test_tiny_cases_by_hand():
    n = 70   # W = 2; the top legal bit is bit 5 of word 1
    a, b, c = pack([[0, 3], [69], [0, 3, 69]], n)
    top = np.uint64(1) << np.uint64(5)
    assert b[1] == top and c[1] == top and a[1] == 0
    zero = np.zeros(2, dtype=np.uint64)
    rows, reads, un = fa.rows_eqclasses(np.array([a, a, a]), n)                       # all equal
    assert rows.tolist() == [a.tolist()] and reads.tolist() == [3] and un == 0
    rows, reads, un = fa.rows_eqclasses(np.array([c, b, a]), n)                       # all distinct: word 0 ties between a and c, word 1 decides; b has word 0 = 0
    assert rows.tolist() == [b.tolist(), a.tolist(), c.tolist()] and reads.tolist() == [1, 1, 1] and un == 0
    rows, reads, un = fa.rows_eqclasses(np.array([zero, zero]), n)                    # all empty
    assert rows.shape == (0, 2) and len(reads) == 0 and un == 2
    rows, reads, un = fa.rows_eqclasses(np.zeros((0, 2), dtype=np.uint64), n)         # no rows
    assert rows.shape == (0, 2) and len(reads) == 0 and un == 0
    rows, reads, un = fa.rows_eqclasses(np.array([a, c, zero, c]), n)                 # two rows that differ only in the last word's top legal bit
    assert rows.tolist() == [a.tolist(), c.tolist()] and reads.tolist() == [1, 2] and un == 1
    # canonical order is unsigned: bit 63 of word 0 sorts last
    hi = pack([[63]], n)[0]
    rows, reads, un = fa.rows_eqclasses(np.array([hi, a, b]), n)
    assert rows.tolist() == [b.tolist(), a.tolist(), hi.tolist()]
    # the tally: colour 3 is in two classes and has no class of its own; colour 69 has the class {69}
    w, o = fa.eqclasses_color_tally(np.array([b, a, c]), np.array([4, 2, 7], dtype=np.uint64), n)
    assert w[0] == 9 and w[3] == 9 and w[69] == 11 and w[1] == 0 and int(w.sum()) == 29
    assert o[69] == 4 and o[3] == 0 and o[0] == 0 and int(o.sum()) == 4
    w, o = fa.eqclasses_color_tally(np.zeros((0, 2), dtype=np.uint64), np.zeros(0, dtype=np.uint64), n)
    assert not w.any() and not o.any() and len(w) == len(o) == n


def test_refusals():
    L = fa.lib()
    n = C.c_uint64(99)
    un = C.c_uint64(99)
    out, reads = np.zeros((4, 1), dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    ask = lambda rows, n_colors, cap: L.fin_rows_eqclasses(rows.ctypes.data_as(U64P), len(rows), n_colors, out.ctypes.data_as(U64P), reads.ctypes.data_as(U64P), cap,
                                                           C.byref(n), C.byref(un))
    rows = np.array([[1], [2], [3], [2]], dtype=np.uint64)
    assert ask(rows, 5, 3) == fa.FIN_OK and n.value == 3 and un.value == 0 and out[:3, 0].tolist() == [1, 2, 3] and reads[:3].tolist() == [1, 2, 1]
    n.value = 99
    assert ask(rows, 5, 2) == fa.FIN_ELIMIT and n.value == 3                  # cap one too small: the number of classes is still reported
    stray = np.array([[1], [1 << 5]], dtype=np.uint64)
    assert ask(stray, 5, 4) == fa.FIN_EINVAL and ask(stray, 6, 4) == fa.FIN_OK
    for bad in (0, 4097):
        assert ask(rows, bad, 4) == fa.FIN_ELIMIT
        with pytest.raises(fa.FinitoError) as e:
            fa.rows_eqclasses(rows, bad)
        assert e.value.code == fa.FIN_ELIMIT
        with pytest.raises(fa.FinitoError) as e:
            fa.eqclasses_color_tally(rows[:1], [1], bad)
        assert e.value.code == fa.FIN_ELIMIT
    with pytest.raises(fa.FinitoError) as e:
        fa.rows_eqclasses(stray, 5)
    assert e.value.code == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:
        fa.eqclasses_color_tally(stray, [1, 1], 5)
    assert e.value.code == fa.FIN_EINVAL
    wide = np.zeros((1, 3), dtype=np.uint64); wide[0, 2] = 1 << 2   # colour 130 of 130
    with pytest.raises(fa.FinitoError) as e:
        fa.rows_eqclasses(wide, 130)
    assert e.value.code == fa.FIN_EINVAL
    assert fa.rows_eqclasses(wide, 131)[1].tolist() == [1]


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_the_accumulator_needs_colours_on_a_device():
    """No CPU fallback: there is no accumulator without a colour matrix, and no colour matrix without a device"""
    idx = fa.FinimizerIndex.build(["ACGGT", "CGGTA"], 4)
    with pytest.raises(fa.FinitoError) as e:
        idx.colors(3).eqclasses()
    assert e.value.code == fa.FIN_ENODEV


def test_cli_usage_rules(tmp_path):
    common = [BIN, "search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq")]
    refs = tmp_path / "refs.txt"
    refs.write_text("%s\n%s\n" % (tmp_path / "a.fna", tmp_path / "b.fna"))
    col = ["--color-refs", str(refs)]
    r = subprocess.run([BIN, "search-fmin", "--help"], capture_output=True, text=True)
    assert all(x in r.stderr for x in ("--eqclasses FILE", "--color-report FILE", "--eq-max-classes N"))
    # with either option alone --no-text 1 and --pseudo-permille are legal: the run gets as far as the index it cannot find
    for flag in ("--eqclasses", "--color-report"):
        r = subprocess.run(common + col + ["--no-text", "1", "--pseudo-permille", "500", flag, str(tmp_path / "s.tsv")], capture_output=True, text=True)
        assert r.returncode == 1 and "--no-text" not in r.stderr and "--color-refs" not in r.stderr and "--pseudo-permille" not in r.stderr, r.stderr
    for flag in ("--eqclasses", "--color-report"):   # no references to colour by
        r = subprocess.run(common + [flag, str(tmp_path / "s.tsv")], capture_output=True, text=True)
        assert r.returncode == 1 and "--color-refs" in r.stderr and not r.stdout
    r = subprocess.run(common + col + ["--eqclasses", str(tmp_path / "s.tsv"), "--pseudo-permille", "1001"], capture_output=True, text=True)
    assert r.returncode == 1 and "--pseudo-permille" in r.stderr and "1000" in r.stderr
    for bad in ("0", "67108865", "-3", "many"):
        r = subprocess.run(common + col + ["--eqclasses", str(tmp_path / "s.tsv"), "--eq-max-classes", bad], capture_output=True, text=True)
        assert r.returncode == 1 and "--eq-max-classes" in r.stderr, bad
    r = subprocess.run(common + col + ["--eqclasses", str(tmp_path / "s.tsv"), "--eq-max-classes", "67108864"], capture_output=True, text=True)
    assert r.returncode == 1 and "--eq-max-classes" not in r.stderr
    r = subprocess.run(common + col + ["--pseudoalign", str(tmp_path / "s.tsv"), "--eq-max-classes", "10"], capture_output=True, text=True)   # room nobody uses
    assert r.returncode == 1 and "--eqclasses" in r.stderr
    r = subprocess.run(common + ["--no-text", "1"], capture_output=True, text=True)   # the rule's message names the new results
    assert r.returncode == 1 and "--eqclasses" in r.stderr and "--color-report" in r.stderr
