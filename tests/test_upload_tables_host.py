"""The tables an upload derives on the device (fin_format.h: ptab, jtab, filt, safe, rcwin, cbf, fbf), the parts that need no GPU: the references of tests/util.py
against independent definitions on tiny inputs, the classes the case generator promises (tests/test_upload_tables.py runs the same cases on the device), and
what fin_index_debug_table refuses before any device call."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.util import (UPLOAD_KS, UPLOAD_SEG, bit_table_diff, bits_at, cbf_bits, cbf_hash, default_cbf_m, interval_table_diff, kmer_ends, rc, ref_absence_filter,
                        ref_prefix_intervals, ref_rcwin, ref_safe, ref_string_filter, string_key, string_keys, text_of, upload_case, upload_case_host,
                        upload_table_cases, yes_reads)

TINY = ["ACGTACGGT", "TTACG", "GGGTTACC", "CCGTA"]


def codes_and_ends(unitigs):
    return np.array(["ACGT".index(ch) for u in unitigs for ch in u], dtype=np.uint8), np.cumsum([len(u) for u in unitigs])


def substrings(unitigs, m):
    return {u[a:a + m] for u in unitigs for a in range(len(u) - m + 1)}


def words_of_bits(bits, n_words):
    w = np.zeros(n_words, dtype=np.uint32)
    for b in bits:
        w[b >> 5] |= np.uint32(1 << (b & 31))
    return w


def test_the_hash_is_the_one_the_header_spells_out():
    """fin_cbf_hash, step by step on one key, and the vectorised form the filter reference uses against it"""
    x = 0x0123456789ABCDEF
    a = x ^ (x >> 29); b = (a * 0xBF58476D1CE4E5B9) % 2**64; c = b ^ (b >> 32); d = (c * 0x94D049BB133111EB) % 2**64
    assert cbf_hash(x) == d ^ (d >> 29) and cbf_hash(0) == 0
    bits = cbf_bits(string_key("ACGTTGCA"), 6)
    assert len(bits) == 5 and len({b >> 7 for b in bits}) == 1 and 0 <= bits[0] >> 7 < 64


@pytest.mark.parametrize("m,log2", [(3, 2), (4, 4), (5, 0), (9, 3)])
def test_string_filter_reference_against_a_set_of_strings(m, log2):
    concat, ends = codes_and_ends(TINY)
    S = substrings(TINY, m)
    assert S and len(S) < len(substrings(["".join(TINY)], m))   # (the strings across two unitigs are not among them)
    for canonical in (True, False):
        want = set()
        for s in S:
            want.update(cbf_bits(min(string_key(s), string_key(rc(s))) if canonical else string_key(s), log2))
        got = ref_string_filter(concat, ends, m, log2, canonical)
        assert got.shape == (1 << log2, 4) and got.dtype == np.uint32
        assert np.array_equal(got.reshape(-1), words_of_bits(want, 4 << log2))
        flat = got.reshape(-1)
        for s in S:   # no false negative, asked the way a reader asks: every bit of the string's own key (the reverse complement's too where canonical)
            for q in ((s, rc(s)) if canonical else (s,)):
                key = min(string_key(q), string_key(rc(q))) if canonical else string_key(q)
                assert all((flat[b >> 5] >> (b & 31)) & 1 for b in cbf_bits(key, log2)), (s, q)
    # the string across two unitigs is not entered: the directional filter of ONE string holds exactly that string's bits
    one = ref_string_filter(*codes_and_ends(["ACG", "TAC"]), 3, 5, False)
    assert np.array_equal(one.reshape(-1), words_of_bits(set(cbf_bits(string_key("ACG"), 5)) | set(cbf_bits(string_key("TAC"), 5)), 128))


@pytest.mark.parametrize("F", [1, 3, 4, 5])
def test_absence_filter_reference_against_a_set_of_strings(F):
    concat, ends = codes_and_ends(TINY)
    S = substrings(TINY, F)
    if F < 3:
        return   # (fewer than 32 bits: the table has no whole word; the upload builds none below 4)
    got = ref_absence_filter(concat, ends, F)
    assert got.shape == (4 ** F // 32,)
    n = 0
    for t in itertools.product("ACGT", repeat=F):
        s = "".join(t); key = string_key(s)
        assert bool((got[key >> 5] >> (key & 31)) & 1) == (s in S), s
        n += s in S
    assert n == len(S) and 0 < n < 4 ** F


def test_string_keys_stay_inside_a_unitig_and_name_first_and_last_string():
    concat, ends = codes_and_ends(TINY)
    f, v, g = string_keys(concat, ends, 4)
    assert g.tolist() == [3, 4, 5, 6, 7, 8, 12, 13, 17, 18, 19, 20, 21, 25, 26]
    assert int(f[0]) == string_key("ACGT") and int(v[0]) == string_key("ACGT") and int(f[6]) == string_key("TTAC") and int(v[6]) == string_key("GTAA")
    assert len(string_keys(concat[:3], [3], 4)[0]) == 0


@pytest.mark.parametrize("name", ["tiny_k4", "tiny_k5"])
def test_interval_reference_against_the_node_labels(name):
    """the interval of a string = the nodes whose label ends with it (a run of neighbours in colexicographic order), from the oracle's labels where it offers them;
    and it is non-empty exactly for the strings that occur in a unitig -- the first bases of a unitig included: the dummy nodes hold them"""
    c = upload_case(name); h = upload_case_host(c)
    labels = h.oracle.labels()
    assert labels is not None and len(labels) == h.n_nodes
    for T in range(1, c.k + 1):
        l, r, ok = ref_prefix_intervals(h.C, h.planes, h.n_nodes, T)
        S = substrings(c.unitigs, T)
        n_yes = 0
        for t in itertools.product("ACGT", repeat=T):
            s = "".join(t); key = string_key(s)
            nodes = [i for i, lab in enumerate(labels) if lab.endswith(s)]
            assert bool(ok[key]) == bool(nodes) == (s in S), (T, s)
            if nodes:
                assert nodes == list(range(int(l[key]), int(r[key]) + 1)), (T, s)
                n_yes += 1
        assert 0 < n_yes and (T < 4 or n_yes < 4 ** T)   # (both answers occur from four bases on)
    # a string that only a unitig's first bases spell (it ends before the unitig's first k-mer does) has an interval: only dummy nodes end with it
    firsts = [(int(s), T) for s in h.starts for T in range(1, c.k) if h.text.count(h.text[s:s + T]) == 1]
    assert firsts or c.k == 4   # (342 bases spell every string of up to three bases more than once)
    for s, T in firsts:
        l, r, ok = ref_prefix_intervals(h.C, h.planes, h.n_nodes, T)
        key = string_key(h.text[s:s + T])
        assert ok[key] and all("$" in labels[i] for i in range(int(l[key]), int(r[key]) + 1))


def test_interval_diff_reports_what_it_should():
    c = upload_case("tiny_k5"); h = upload_case_host(c)
    l, r, ok = ref_prefix_intervals(h.C, h.planes, h.n_nodes, 4)
    tab = np.where(ok[:, None], np.stack([l, r], axis=1), np.array([[1, 0]])).astype(np.uint32)
    assert len(interval_table_diff(tab, l, r, ok)) == 0
    yes, no = int(np.nonzero(ok)[0][3]), int(np.nonzero(~ok)[0][3])
    for key, col, val in ((yes, 0, tab[yes, 0] + 1), (yes, 1, tab[yes, 1] + 1), (no, 1, 1), (no, 0, 0)):   # (an empty entry that reads l <= r: {1, 1}, {0, 0})
        t = tab.copy(); t[key, col] = val
        assert interval_table_diff(t, l, r, ok).tolist() == [key]


# three unitigs written by hand (k = 4), in the index's order: 70 C's, ACGT, 590 T's + GGGG
HAND = ["C" * 70, "ACGT", "T" * 590 + "GGGG"]


def test_rcwin_reference_on_three_hand_written_unitigs():
    """CCCC (ends at 3 .. 69: windows 0 and 1 of byte 0) and GGGG (ends at 667: window 2 of byte 1) are each other's reverse complement, ACGT (ends at 73, window
    1) is its own; TTTT, TTTG, TTGG and TGGG have none"""
    text = "".join(HAND); ends = np.cumsum([len(u) for u in HAND])
    win, n = ref_rcwin(text, ends, 4)
    assert win.tolist() == [0b011, 0b100] and n == 67 + 1 + 1
    win, n = ref_rcwin(text, ends, 5)   # k = 5: CCCCC and ACGT's unitig has no k-mer; nothing pairs
    assert win.tolist() == [0, 0] and n == 0
    assert kmer_ends(ends, 4).tolist() == list(range(3, 70)) + [73] + list(range(77, 668))


def test_safe_reference_on_three_hand_written_unitigs():
    """ACGT, TTTG, TTGG, TGGG and GGGG occur once: their places are safe.  CCCC has 67 places and TTTT 587: the reference reports one place for a k-mer, so at
    most one of them is safe -- and the bits are positions of k-mer ends only"""
    o = OracleIndex.build(HAND, 4)
    text = text_of(o.concat()); ends = o.ends()
    assert text == "".join(HAND) and ends.tolist() == [70, 74, 668]
    at, bit = ref_safe(o, text, ends, 4)
    assert at.tolist() == kmer_ends(ends, 4).tolist()
    by = dict(zip(at.tolist(), bit.tolist()))
    assert [by[g] for g in (73, 664, 665, 666, 667)] == [1] * 5
    assert sum(by[g] for g in range(3, 70)) <= 1 and sum(by[g] for g in range(77, 664)) <= 1
    for g in at[bit == 1]:   # a safe place is the answer of the k-mer it spells
        (u, off), = o.search(text[g - 3:g + 1])[0]
        assert [0, 70, 74][u] + off + 3 == g
    # a disjoint set: every place is safe
    o2 = OracleIndex.build(["ACGGTCA", "TTGAC"], 4)
    at2, bit2 = ref_safe(o2, text_of(o2.concat()), o2.ends(), 4)
    assert len(at2) == 4 + 2 and bit2.all()


def test_bit_table_diff_is_two_sided():
    want = np.array([0b1010, 0, 0xFFFFFFFF], dtype=np.uint32)
    assert bit_table_diff(want.copy(), want) == {"lacking": 0, "extra": 0, "first_lacking": None, "first_extra": None}
    got = want.copy(); got[0] &= ~np.uint32(2); got[1] |= np.uint32(5)
    assert bit_table_diff(got, want) == {"lacking": 1, "extra": 2, "first_lacking": 0, "first_extra": 1}
    assert bits_at(np.array([1 << 63, 5], dtype=np.uint64), [63, 64, 65, 66, 0]).tolist() == [1, 1, 0, 1, 0]


# ---- the generator's classes ----------------------------------------------------------------------------------------------------------------------------------
def _classes(c, h):
    k = c.k; L = len(h.text); lens = h.ends - h.starts
    n_seg = (L + UPLOAD_SEG - 1) // UPLOAD_SEG
    return {"total": L,
            "end_on_seam": any(e % UPLOAD_SEG == 0 for e in h.ends[:-1]), "start_on_seam": any(s % UPLOAD_SEG == 0 for s in h.starts[1:]),
            "seam_unitig_has_2k_1": any(e % UPLOAD_SEG == 0 and e - s >= 2 * k - 1 for s, e in zip(h.starts, h.ends[:-1])),
            "exactly_k": bool((lens == k).any()),
            "in_one_segment": max(sum(1 for s, e in zip(h.starts, h.ends) if s < UPLOAD_SEG * (j + 1) and e > UPLOAD_SEG * j) for j in range(n_seg)),
            "segments_of_one": max((int(e) - 1) // UPLOAD_SEG - int(s) // UPLOAD_SEG + 1 for s, e in zip(h.starts, h.ends)),
            "both_orientations": any(x[:k - 1] == rc(y[:k - 1]) for x in c.unitigs for y in c.unitigs if x is not y)}


def test_the_cases_are_small_and_legal():
    cases = upload_table_cases()
    assert len({c.name for c in cases}) == len(cases) and {c.k for c in cases} >= set(UPLOAD_KS)
    for c in cases:
        h = upload_case_host(c)
        assert c.k <= len(h.text) <= 8200 and all(len(u) >= c.k for u in c.unitigs) and h.ends[-1] == len(h.text) == sum(len(u) for u in c.unitigs)
        assert sorted(h.text[a:b] for a, b in zip(h.starts, h.ends)) == sorted(c.unitigs)


@pytest.mark.parametrize("k", UPLOAD_KS)
def test_general_cases_cover_their_classes(k):
    c = upload_case("general_k%d" % k); h = upload_case_host(c)
    cl = _classes(c, h)
    assert cl["end_on_seam"] and cl["start_on_seam"] and cl["seam_unitig_has_2k_1"] and cl["exactly_k"] and cl["both_orientations"], cl
    assert cl["in_one_segment"] >= 5 and cl["segments_of_one"] >= 3 and cl["total"] > 4 * UPLOAD_SEG, cl
    for m in {default_cbf_m(k), 9, 4, 8, min(k, 32), 1, 7}:   # every string length the device tests ask: strings end on, behind and before a seam; first and last of every unitig
        g = string_keys(h.concat, h.ends, m)[2]
        assert {0, 1, UPLOAD_SEG - 1} <= set((g % UPLOAD_SEG).tolist()), m
        assert set((h.starts + m - 1).tolist()) <= set(g.tolist()) and set((h.ends - 1).tolist()) <= set(g.tolist())
        assert len(g) == int((h.ends - h.starts - m + 1).sum())
    at = kmer_ends(h.ends, k)
    assert {0, 1, UPLOAD_SEG - 1} <= set((at % UPLOAD_SEG).tolist())
    if k >= 16:   # the sets the "asked where the answer is yes" test reads from: every k-mer has one place, three unitigs B with room for 2k - 1 bases
        assert h.oracle.is_disjoint()
        assert h.ends[0] - h.starts[0] >= 2 * k - 1 and h.ends[-1] - h.starts[-1] >= 2 * k - 1
        assert h.text[h.starts[0]:][:k].endswith("AAAA") and h.text[h.starts[-1]:][:k].endswith("TTTT")
    win, n = ref_rcwin(h.text, h.ends, k)
    assert k == 12 or n == 0


def test_whole_text_lengths():
    want = {"total_12_k12": 12, "total_511_k12": 511, "total_512_k12": 512, "total_513_k12": 513, "total_1031_k12": 2 * UPLOAD_SEG + default_cbf_m(12) - 2,
            "total_530_k31": UPLOAD_SEG + default_cbf_m(31) - 2, "total_1042_k63": 2 * UPLOAD_SEG + default_cbf_m(63) - 2}
    assert default_cbf_m(12) == 9 and default_cbf_m(31) == default_cbf_m(63) == 20 and default_cbf_m(16) == 11 and default_cbf_m(21) == 15
    for name, total in want.items():
        c = upload_case(name); h = upload_case_host(c)
        assert len(h.text) == total, name
        m = default_cbf_m(c.k)
        if total > UPLOAD_SEG + 1:
            assert total % UPLOAD_SEG == m - 2 and h.ends[-1] - h.starts[-1] >= m


def test_duplicates_reverse_complements_and_their_own():
    fam = [c for c in upload_table_cases() if c.name.startswith("family_")]
    assert {c.k for c in fam} == {12, 21, 33, 63}
    for c in fam:
        h = upload_case_host(c)
        at, bit = ref_safe(h.oracle, h.text, h.ends, c.k)
        assert (bit == 0).sum() > 0 and not h.oracle.is_disjoint() and ref_rcwin(h.text, h.ends, c.k)[1] > 0, c.name
        assert len(set(c.unitigs)) < len(c.unitigs)   # identical unitigs
    for c in (c for c in upload_table_cases() if c.name.startswith("rc_")):
        h = upload_case_host(c)
        win, n = ref_rcwin(h.text, h.ends, c.k)
        assert h.oracle.is_disjoint() and n >= 2 * (4 * c.k + 1) and win.any() and not win.all(), c.name
        assert ref_safe(h.oracle, h.text, h.ends, c.k)[1].all()
        own = [g for g in kmer_ends(h.ends, c.k) if h.text[g - c.k + 1:g + 1] == rc(h.text[g - c.k + 1:g + 1])]
        assert bool(own) == (c.k % 2 == 0), c.name
        for g in own:
            assert (win[g >> 9] >> ((g >> 6) & 7)) & 1


def test_yes_reads_are_what_they_say():
    c = upload_case("general_k16"); h = upload_case_host(c); k = 16
    seam = next(u for u in range(len(h.ends) - 1) if h.ends[u] % UPLOAD_SEG == 0 and h.ends[u] - h.starts[u] >= 2 * k - 1)
    for b in (0, len(h.ends) - 1, seam):
        a = max((u for u in range(len(h.ends)) if u != b), key=lambda u: h.ends[u] - h.starts[u])
        A = h.text[h.starts[a]:h.ends[a]]; B = h.text[h.starts[b]:h.ends[b]]
        assert len(B) >= 2 * k - 1
        reads = yes_reads(h.text, k, (h.starts[a], h.ends[a]), (h.starts[b], h.ends[b]))
        assert len(reads) == 4 * (len(B) - 2 * k + 2) and all(len(r) == 2 * k - 1 + k + 5 for r in reads)
        assert reads[0] == A[-(k + 5):] + B[:2 * k - 1] and reads[1] == rc(reads[0]) and reads[2] == B[:2 * k - 1] + A[:k + 5]
        assert reads[-2].startswith(B[-(2 * k - 1):])
        exp, _, _ = h.oracle.search_batch(reads)
        nk = len(reads[0]) - k + 1
        first = exp[:nk]
        assert first[:6].tolist() == [[a, len(A) - (k + 5) + i] for i in range(6)] and first[-k:].tolist() == [[b, i] for i in range(k)]
        assert (first[6:-k, 0] == -1).all()   # the k-mers across the junction are in no unitig


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_null_arguments_and_missing_replicas_are_refused_before_any_device_call():
    L = fa.lib()
    err = C.create_string_buffer(512)
    out = (C.c_uint32 * 64)()
    m, lg = C.c_uint32(7), C.c_uint32(7)
    idx = fa.FinimizerIndex.build(["ACGGT", "CGGTA"], 4)
    for what in range(7):
        assert L.fin_index_debug_table_bytes(None, 0, what) == -1 and L.fin_index_debug_table_bytes(idx.h, 0, what) == -1   # no index; no replica on that device
        assert L.fin_index_debug_table(None, 0, what, out, 256, err, 512) == fa.FIN_EINVAL and b"null" in err.value
        assert L.fin_index_debug_table(idx.h, 0, what, None, 256, err, 512) == fa.FIN_EINVAL and b"null" in err.value
        assert L.fin_index_debug_table(idx.h, 0, what, out, 256, err, 512) == fa.FIN_EINVAL and b"no replica" in err.value
        assert L.fin_index_debug_table(idx.h, 5, what, out, 256, err, 512) == fa.FIN_EINVAL and b"no replica" in err.value
    assert L.fin_index_debug_table_bytes(idx.h, 0, 7) == -1 and L.fin_index_debug_table_bytes(idx.h, 0, -1) == -1
    assert L.fin_index_string_filter_geometry(None, 0, C.byref(m), C.byref(lg)) == fa.FIN_EINVAL
    assert L.fin_index_string_filter_geometry(idx.h, 0, C.byref(m), C.byref(lg)) == fa.FIN_EINVAL and (m.value, lg.value) == (7, 7)
    with pytest.raises(fa.FinitoError) as e:
        idx.debug_table(fa.DT_CBF)
    assert e.value.code == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:
        idx.string_filter_geometry()
    assert e.value.code == fa.FIN_EINVAL
    assert (fa.DT_PTAB, fa.DT_JTAB, fa.DT_FILT, fa.DT_SAFE, fa.DT_RCWIN, fa.DT_CBF, fa.DT_FBF) == (0, 1, 2, 3, 4, 5, 6)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "finito_amd.h")).read()
    for i, n in enumerate(("PTAB", "JTAB", "FILT", "SAFE", "RCWIN", "CBF", "FBF")):
        assert "#define FIN_DT_%s %d\n" % (n, i) in src
