"""Colour sets per unitig and read pseudoalignment, the parts that need no GPU (include/finito_amd.h: fin_colors, fin_read_pseudo, fin_records_pseudoalign): the
definition written out in numpy over a read set's pairs, tiny reads whose answers are written out by hand, the host function against the definition on the
hand-made records of tests/util.py, what is refused, and the command's usage rules for --color-refs, --colors-out, --pseudoalign and --pseudo-permille."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from tests.test_records import brute_expand
from tests.util import hand_made_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def words_of(n_colors):
    return (n_colors + 63) // 64


def pack(sets, n_colors):
    """uint64[len(sets), W] from one collection of colours per unitig"""
    bits = np.zeros((len(sets), words_of(n_colors)), dtype=np.uint64)
    for u, cs in enumerate(sets):
        for c in cs:
            assert 0 <= c < n_colors
            bits[u, c >> 6] |= np.uint64(1) << np.uint64(c & 63)
    return bits


def pack_members(member):
    """uint64[n, W] from 0/1 [n, n_colors]"""
    member = np.asarray(member).astype(np.uint8)
    n, n_colors = member.shape
    wide = np.zeros((n, 64 * words_of(n_colors)), dtype=np.uint8)
    wide[:, :n_colors] = member
    return np.ascontiguousarray(np.packbits(wide, axis=1, bitorder="little")).view(np.uint64).reshape(n, words_of(n_colors))


def unpack(bits, n_colors):
    """0/1 [n, n_colors] from uint64[n, W]"""
    b = np.ascontiguousarray(bits, dtype=np.uint64)
    return np.unpackbits(b.view(np.uint8), axis=1, bitorder="little")[:, :n_colors].astype(np.int64)


def colors_of(row, n_colors):
    return [int(c) for c in np.nonzero(unpack(np.asarray(row, dtype=np.uint64).reshape(1, -1), n_colors)[0])[0]]


def rows_of(pairs, nks, bits, n_colors, permille):
    """the definition (include/finito_amd.h), over a read set's pairs back to back, read r has nks[r] of them; bits = the colour matrix uint64[n_unitigs, W].  A slot
    is found when its unitig number is one of the matrix's (an absent slot's -1 is not, nor is a number at or above n_unitigs), coloured when that unitig's row is not
    empty; cnt = the column sums of the coloured slots' rows; colour c is in iff cnt[c] >= 1 and 1000 * cnt[c] >= permille * n_colored, in Python integers.
    Returns (rows uint64[n_reads, W], heads READ_PSEUDO_DTYPE[n_reads])"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    nks = np.asarray(nks, dtype=np.int64)
    member = unpack(bits, n_colors)
    n_unitigs = len(member)
    rows = np.zeros((len(nks), words_of(n_colors)), dtype=np.uint64)
    heads = np.zeros(len(nks), dtype=fa.READ_PSEUDO_DTYPE)
    at = np.concatenate([[0], np.cumsum(nks)])
    for r in range(len(nks)):
        u = pairs[at[r]:at[r + 1], 0]
        u = u[(u >= 0) & (u < n_unitigs)]
        m = member[u]
        m = m[m.any(axis=1)] if len(m) else m
        n_colored = len(m)
        cnt = m.sum(axis=0) if n_colored else np.zeros(n_colors, dtype=np.int64)
        inside = (cnt >= 1) & (1000 * cnt >= permille * n_colored)   # (int64: 1000 * cnt stays far below 2^63)
        rows[r] = pack_members(inside[None, :])[0]
        heads[r] = (len(u), n_colored, int(inside.sum()), 0)
    return rows, heads


def assert_pseudo(got, want, what=""):
    rows, heads = got
    wrows, wheads = want
    assert heads.dtype == fa.READ_PSEUDO_DTYPE and heads.shape == wheads.shape and rows.dtype == np.uint64 and rows.shape == wrows.shape, what
    for f in ("n_found", "n_colored", "n_colors", "reserved"):
        bad = np.nonzero(heads[f] != wheads[f])[0]
        assert len(bad) == 0, "%s: field %s differs in %d reads, first %d: got %s, want %s" % (what, f, len(bad), bad[0], heads[bad[0]], wheads[bad[0]])
    bad = np.nonzero((rows != wrows).any(axis=1))[0]
    assert len(bad) == 0, "%s: the row differs in %d reads, first %d: got %s, want %s" % (what, len(bad), bad[0], rows[bad[0]], wrows[bad[0]])


def random_matrix(rng, n_unitigs, n_colors, empty_share=0.1):
    """about empty_share of the rows empty; the others hold one colour, several, or all of them; the top colour is used"""
    member = np.zeros((n_unitigs, n_colors), dtype=np.int64)
    how = rng.integers(0, 4, n_unitigs)
    for u in range(n_unitigs):
        if how[u] == 0:
            member[u, int(rng.integers(0, n_colors))] = 1
        elif how[u] == 1:
            member[u, rng.choice(n_colors, size=min(n_colors, int(rng.integers(2, 6))), replace=False)] = 1
        elif how[u] == 2:
            member[u] = rng.random(n_colors) < 0.6
        else:
            member[u] = 1
    member[rng.random(n_unitigs) < empty_share] = 0
    member[int(np.argmax(member.any(axis=1))), n_colors - 1] = 1
    bits = pack_members(member)
    assert not bits.any(axis=1).all() and bits.any()
    return bits


def test_the_numpy_definition_on_small_reads():
    # unitig: 0 {0,1}, 1 {1,2}, 2 {3}, 3 {} (uncoloured), 4 {0,1,2,3}
    n_colors = 4
    bits = pack([[0, 1], [1, 2], [3], [], [0, 1, 2, 3]], n_colors)
    A = (-1, -1)

    def ask(pairs, permille):
        rows, heads = rows_of(pairs, [len(pairs)], bits, n_colors, permille)
        return colors_of(rows[0], n_colors), tuple(int(x) for x in heads[0].tolist())

    # overlapping sets: the intersection is what they share, the union everything
    two = [(0, 5), (0, 6), (1, 0)]
    assert ask(two, 1000) == ([1], (3, 3, 1, 0)) and ask(two, 0) == ([0, 1, 2], (3, 3, 3, 0))
    # counts 0: 2, 1: 3, 2: 1 of 3 coloured -- 500 wants 1000 * cnt >= 1500: colours 0 and 1
    assert ask(two, 500) == ([0, 1], (3, 3, 2, 0)) and ask(two, 667) == ([1], (3, 3, 1, 0)) and ask(two, 666) == ([0, 1], (3, 3, 2, 0))
    # disjoint sets: an intersection that is empty although the union is not
    apart = [(0, 1), A, (2, 7), (2, 8)]
    assert ask(apart, 1000) == ([], (3, 3, 0, 0)) and ask(apart, 0) == ([0, 1, 3], (3, 3, 3, 0)) and ask(apart, 500) == ([3], (3, 3, 1, 0))
    # found k-mers that are all uncoloured: found, not coloured, no colour under any threshold
    for pm in (0, 500, 1000):
        assert ask([(3, 0), (3, 1), A], pm) == ([], (2, 0, 0, 0))
    # coloured and uncoloured k-mers in one read: the uncoloured ones and the absent ones do not dilute the intersection
    mixed = [(3, 0), (0, 1), A, (3, 2), (0, 2), (4, 0)]
    assert ask(mixed, 1000) == ([0, 1], (5, 3, 2, 0)) and ask(mixed, 0) == ([0, 1, 2, 3], (5, 3, 4, 0)) and ask(mixed, 334) == ([0, 1], (5, 3, 2, 0))
    assert ask(mixed, 333) == ([0, 1, 2, 3], (5, 3, 4, 0))
    # nothing found, no k-mers; a unitig number outside the matrix is an absent slot
    assert ask([A, A], 0) == ([], (0, 0, 0, 0)) and ask([], 1000) == ([], (0, 0, 0, 0)) and ask([(5, 0), (9, 1), (2, 0)], 1000) == ([3], (1, 1, 1, 0))
    # reversing the slot order changes nothing
    for pm in (0, 300, 1000):
        a, b = rows_of(mixed, [6], bits, n_colors, pm), rows_of(mixed[::-1], [6], bits, n_colors, pm)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # several reads back to back, and a matrix of more than one word: colour 64 is bit 0 of word 1
    wide = pack([[63, 64], [64, 129], []], 130)
    rows, heads = rows_of([(0, 0), (1, 0), (2, 0), A, (1, 1)], [2, 2, 1], wide, 130, 1000)
    assert rows.tolist() == [[0, 1, 0], [0, 0, 0], [0, 1, 2]] and [tuple(h) for h in heads.tolist()] == [(2, 2, 1, 0), (1, 0, 0, 0), (1, 1, 2, 0)]


@pytest.mark.parametrize("n_colors", [1, 64, 65, 130])
@pytest.mark.parametrize("k", [16, 31, 63])
def test_host_pseudoalignment_of_hand_made_records(k, n_colors):
    c = hand_made_case(k)
    rng = np.random.default_rng(1900 + 7 * k + n_colors)
    bits = random_matrix(rng, len(c.unitigs), n_colors)
    kinds, rev = c.recs["meta"] >> 16, (c.recs["meta"] >> 8) & 1
    assert all((kinds == x).sum() > 100 for x in (0, 1, 2)) and ((kinds == 1) & (rev == 1)).sum() > 100   # every kind, both strands
    assert np.array_equal(brute_expand(c.recs, c.stream, k), c.pairs)   # the pairs are what the records mean
    for permille in (0, 300, 1000):
        want = rows_of(c.pairs, c.nks, bits, n_colors, permille)
        if permille == 1000:
            assert ((want[1]["n_colored"] > 0) & (want[1]["n_colored"] < want[1]["n_found"])).any() and (want[1]["n_colors"][kinds == 1] > 0).any()
        got = fa.records_pseudoalign(c.recs, c.stream, k, bits, n_colors, permille)
        assert_pseudo(got, want, "k=%d, %d colours, permille %d" % (k, n_colors, permille))
        one, eight = fa.records_pseudoalign(c.recs, c.stream, k, bits, n_colors, permille, n_threads=1), fa.records_pseudoalign(c.recs, c.stream, k, bits, n_colors, permille, n_threads=8)
        assert one[0].tobytes() == eight[0].tobytes() == got[0].tobytes() and one[1].tobytes() == eight[1].tobytes() == got[1].tobytes()


def test_refusals():
    c = hand_made_case(31)
    nu = len(c.unitigs)
    bits = pack([[0]] * nu, 3)
    for n_colors in (0, 4097):
        with pytest.raises(fa.FinitoError) as e:
            fa.records_pseudoalign(c.recs, c.stream, 31, np.zeros((nu, max(1, words_of(n_colors))), np.uint64), n_colors)
        assert e.value.code == fa.FIN_ELIMIT
    fa.records_pseudoalign(c.recs, c.stream, 31, np.zeros((nu, 64), np.uint64), 4096)
    with pytest.raises(fa.FinitoError) as e:
        fa.records_pseudoalign(c.recs, c.stream, 31, bits, 3, permille=1001)
    assert e.value.code == fa.FIN_EINVAL
    for n_colors, stray in ((3, 3), (3, 63), (65, 65 - 64)):   # a set bit at or above n_colors, in the last word
        bad = pack([[0]] * nu, n_colors)
        bad[nu // 2, -1] |= np.uint64(1) << np.uint64(stray)
        with pytest.raises(fa.FinitoError) as e:
            fa.records_pseudoalign(c.recs, c.stream, 31, bad, n_colors)
        assert e.value.code == fa.FIN_EINVAL
    for threads in (1, 8):
        for stream in (c.stream[:-1], np.concatenate([c.stream, c.stream[:3]])):   # a truncated stream, a stream with pairs to spare
            with pytest.raises(fa.FinitoError) as e:
                fa.records_pseudoalign(c.recs, stream, 31, bits, 3, n_threads=threads)
            assert e.value.code == fa.FIN_EINVAL
        bad = np.array(c.stream); bad[len(bad) // 2] = (-2, 5)   # neither found nor (-1,-1)
        with pytest.raises(fa.FinitoError) as e:
            fa.records_pseudoalign(c.recs, bad, 31, bits, 3, n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
        top = int(max(c.stream[:, 0].max(), c.recs["u"].max()))
        with pytest.raises(fa.FinitoError) as e:   # a unitig number at or above n_unitigs
            fa.records_pseudoalign(c.recs, c.stream, 31, bits[:top], 3, n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
        bad = np.array(c.stream); bad[np.nonzero(bad[:, 0] >= 0)[0][0], 0] = nu   # ... in the stream
        with pytest.raises(fa.FinitoError) as e:
            fa.records_pseudoalign(c.recs, bad, 31, bits, 3, n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
        fa.records_pseudoalign(c.recs, c.stream, 31, bits[:top + 1], 3, n_threads=threads)
    rows, heads = fa.records_pseudoalign(np.zeros(0, fa.RECORD_DTYPE), np.zeros((0, 2), np.int32), 31, bits, 3)   # nothing is legal
    assert rows.shape == (0, 1) and len(heads) == 0


def test_null_and_bad_arguments_are_refused_before_any_device_call():
    L = fa.lib()
    err = C.create_string_buffer(512)
    h = C.c_void_p()
    assert L.fin_colors_create(None, 0, 5, C.byref(h), err, 512) == fa.FIN_EINVAL and b"null" in err.value
    assert L.fin_colors_upload(None, None, err, 512) == fa.FIN_EINVAL and L.fin_colors_download(None, None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_colors_reset(None, None) == fa.FIN_EINVAL
    assert L.fin_colors_device_bits(None) is None and L.fin_colors_n_colors(None) == 0 and L.fin_colors_words(None) == 0
    assert L.fin_batch_device_pseudo_rows(None) is None and L.fin_batch_device_pseudo_heads(None) is None
    L.fin_colors_free(None)
    assert L.fin_batch_add_colors(None, None, 0, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_batch_pseudoalign(None, None, 1000, err, 512) == fa.FIN_EINVAL
    assert L.fin_batch_download_pseudo(None, None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_search_batch_add_colors(None, None, None, 0, fa.FIN_MERGED, None, 0, err, 512) == fa.FIN_EINVAL
    assert L.fin_search_batch_pseudoalign(None, None, None, 0, fa.FIN_MERGED, None, 1000, None, None, None, err, 512) == fa.FIN_EINVAL
    out = (C.c_uint64 * 4)()
    assert L.fin_records_pseudoalign(None, 5, None, 0, 31, out, 1, 3, 1000, out, out, 1) == fa.FIN_EINVAL
    assert L.fin_records_pseudoalign(None, 0, None, 0, 31, None, 0, 3, 1000, None, None, 1) == fa.FIN_OK
    # the limit on n_colors comes before the device is asked for
    idx = fa.FinimizerIndex.build(["ACGGT", "CGGTA"], 4)
    for n in (0, 4097, 1 << 20):
        with pytest.raises(fa.FinitoError) as e:
            idx.colors(n)
        assert e.value.code == fa.FIN_ELIMIT and "4096" in str(e.value)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_colour_entry_points_fail_loudly_without_device():
    """No CPU fallback: without a HIP device the device entry points raise, they do not compute"""
    idx = fa.FinimizerIndex.build(["ACGGT", "CGGTA"], 4)
    for n in (1, 64, 4096):
        with pytest.raises(fa.FinitoError) as e:
            idx.colors(n)
        assert e.value.code == fa.FIN_ENODEV
    with pytest.raises(fa.FinitoError) as e:
        idx.colors(3, np.zeros((2, 1), np.uint64))
    assert e.value.code == fa.FIN_ENODEV


def test_cli_usage_rules(tmp_path):
    common = [BIN, "search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq")]
    refs = tmp_path / "refs.txt"
    refs.write_text("%s\n%s\n" % (tmp_path / "a.fna", tmp_path / "b.fna"))
    col = ["--color-refs", str(refs)]
    r = subprocess.run([BIN, "search-fmin", "--help"], capture_output=True, text=True)
    assert all(x in r.stderr for x in ("--color-refs", "--colors-out", "--pseudoalign", "--pseudo-permille"))
    # with --pseudoalign or --colors-out --no-text 1 is legal: the run gets as far as the index it cannot find
    for flag in ("--pseudoalign", "--colors-out"):
        r = subprocess.run(common + col + ["--no-text", "1", flag, str(tmp_path / "s.tsv")], capture_output=True, text=True)
        assert r.returncode == 1 and "--no-text" not in r.stderr and "--color-refs" not in r.stderr
    for flag in ("--pseudoalign", "--colors-out"):   # no references to colour by
        r = subprocess.run(common + [flag, str(tmp_path / "s.tsv")], capture_output=True, text=True)
        assert r.returncode == 1 and "--color-refs" in r.stderr and not r.stdout
    r = subprocess.run(common + col, capture_output=True, text=True)   # a colouring nobody uses
    assert r.returncode == 1 and "--pseudoalign" in r.stderr and "--colors-out" in r.stderr
    r = subprocess.run(common + col + ["--pseudoalign", str(tmp_path / "s.tsv"), "--pseudo-permille", "1001"], capture_output=True, text=True)
    assert r.returncode == 1 and "--pseudo-permille" in r.stderr and "1000" in r.stderr
    r = subprocess.run(common + col + ["--colors-out", str(tmp_path / "c.tsv"), "--pseudo-permille", "500"], capture_output=True, text=True)   # a threshold nobody uses
    assert r.returncode == 1 and "--pseudoalign" in r.stderr
    empty = tmp_path / "none.txt"
    empty.write_text("\n")
    r = subprocess.run(common + ["--color-refs", str(empty), "--pseudoalign", str(tmp_path / "s.tsv")], capture_output=True, text=True)
    assert r.returncode == 1 and "empty" in r.stderr
    many = tmp_path / "many.txt"
    many.write_text("".join("r%d.fna\n" % i for i in range(4097)))
    r = subprocess.run(common + ["--color-refs", str(many), "--pseudoalign", str(tmp_path / "s.tsv")], capture_output=True, text=True)
    assert r.returncode == 1 and "4096" in r.stderr
    many.write_text("".join("r%d.fna\n" % i for i in range(4096)))   # 4096 lines are legal: the run gets as far as the index
    r = subprocess.run(common + ["--color-refs", str(many), "--pseudoalign", str(tmp_path / "s.tsv")], capture_output=True, text=True)
    assert r.returncode == 1 and "4096" not in r.stderr
    r = subprocess.run(common + ["--color-refs", str(tmp_path / "absent.txt"), "--pseudoalign", str(tmp_path / "s.tsv")], capture_output=True, text=True)
    assert r.returncode == 1 and "absent.txt" in r.stderr
    # a partitioned index has no colours: known once the index is loaded, refused before it goes to a device; the usage text says so
    r = subprocess.run([BIN, "search-fmin", "--help"], capture_output=True, text=True)
    at = r.stderr.index("--color-refs LIST")
    assert "Not for a partitioned index" in r.stderr[at:r.stderr.index("--colors-out FILE", at)]
