"""Every table an upload derives on the device -- prefix and jump table, absence filter, safe-place bitmap, reverse-complement windows, the canonical and the
directional string filter (fin_format.h: FinDevIndex) -- downloaded as it lies in HBM (fin_index_debug_table) and compared with its definition restated in
numpy over the unitig text (tests/util.py; tests/test_upload_tables_host.py checks those restatements and the classes the unitig sets cover).  The search
kernels trust these tables one-sidedly, and random reads almost never ask them where the answer is yes: here the whole table is the assertion, and the last
test reads text of another unitig behind a disagreeing base, where it is."""
import numpy as np
import pytest

import finito_amd as fa
from tests.util import (UPLOAD_KS, UPLOAD_SEG, assert_bit_tables_equal, bit_table_diff, bits_at, default_cbf_m, interval_table_diff, ref_absence_filter,
                        ref_prefix_intervals, ref_rcwin, ref_safe, ref_string_filter, upload_case, upload_case_host, upload_table_cases, yes_reads)

pytestmark = pytest.mark.gpu

CASES = [c.name for c in upload_table_cases() if c.k in UPLOAD_KS]
TINY = [c.name for c in upload_table_cases() if c.k not in UPLOAD_KS]


def upload(case, **options):
    p = fa.FinimizerIndex.build(list(case.unitigs), case.k)
    for name, value in options.items():
        p.set_option(name, value)
    return p.to_device(0)


def memo(h, key, make):
    if key not in h.memo:
        h.memo[key] = make()
    return h.memo[key]


def a_set_bit(words):
    """(flat word index, bit) of some set bit in the middle of a table"""
    flat = words.reshape(-1)
    nz = np.nonzero(flat)[0]
    w = int(nz[len(nz) // 2])
    return w, int(flat[w]).bit_length() - 1


@pytest.mark.parametrize("name", CASES)
def test_string_filters_hold_exactly_the_strings_of_the_text(name):
    """cbf and fbf, word for word, at the default string length, 9, 32 (k >= 32) and k (k <= 16), with lean tables on so that the directional filter exists"""
    c = upload_case(name); h = upload_case_host(c); k = c.k
    lg = 4
    while (8 << lg) < len(h.text):
        lg += 1
    for opt in [-1, 9] + ([32] if k >= 32 else []) + ([k] if k <= 16 else []):
        m = default_cbf_m(k) if opt < 0 else opt
        p = upload(c, lean_tables=3, cbf_m=opt)
        assert p.string_filter_geometry() == (m, lg) and p.lean_tables() and p.string_filter_bytes() == 16 << lg
        for what, canonical in ((fa.DT_CBF, True), (fa.DT_FBF, False)):
            got = p.debug_table(what)
            want = memo(h, ("sf", m, lg, canonical), lambda: ref_string_filter(h.concat, h.ends, m, lg, canonical))
            assert got is not None and got.shape == want.shape
            assert_bit_tables_equal(got, want, "%s %s m=%d" % (name, "cbf" if canonical else "fbf", m))
            w, b = a_set_bit(got)   # the comparison bites: one bit cleared in a copy is one missing entry
            hurt = got.copy(); hurt.reshape(-1)[w] &= ~np.uint32(1 << b)
            d = bit_table_diff(hurt, want)
            assert (d["lacking"], d["extra"], d["first_lacking"]) == (1, 0, w)
        p.close()
    p = upload(c, lean_tables=0)   # without lean tables: the canonical filter alone
    assert p.debug_table(fa.DT_FBF) is None and p.string_filter_geometry() == (default_cbf_m(k), lg)
    assert_bit_tables_equal(p.debug_table(fa.DT_CBF), h.memo[("sf", default_cbf_m(k), lg, True)], name + " cbf, lean tables off")
    p.close()
    p = upload(c, cbf_m=0)
    assert p.debug_table(fa.DT_CBF) is None and p.debug_table(fa.DT_FBF) is None and p.string_filter_geometry() == (0, 0)
    p.close()


@pytest.mark.parametrize("name", CASES)
def test_absence_filter_is_the_set_of_strings_inside_unitigs(name):
    """filt at F = 4, 8 and, k = 12, k - 1: bit key set iff the string with that key lies inside one unitig"""
    c = upload_case(name); h = upload_case_host(c); k = c.k
    for F in (4, 8) + ((k - 1,) if k == 12 else ()):
        p = upload(c, filt_f=F)
        assert p.filter_depth() == F
        got = p.debug_table(fa.DT_FILT)
        want = memo(h, ("filt", F), lambda: ref_absence_filter(h.concat, h.ends, F))
        assert got is not None and got.shape == want.shape == (4 ** F // 32,)
        assert_bit_tables_equal(got, want, "%s filt F=%d" % (name, F))
        w, b = a_set_bit(got)
        hurt = got.copy(); hurt[w] &= ~np.uint32(1 << b)
        d = bit_table_diff(hurt, want)
        assert (d["lacking"], d["extra"], d["first_lacking"]) == (1, 0, w)
        p.close()
    p = upload(c, filt_f=0)
    assert p.filter_depth() == 0 and p.debug_table(fa.DT_FILT) is None
    p.close()


def check_interval_table(got, h, T, what):
    l, r, ok = memo(h, ("ival", T), lambda: ref_prefix_intervals(h.C, h.planes, h.n_nodes, T))
    assert got is not None and got.shape == (4 ** T, 2)
    bad = interval_table_diff(got, l, r, ok)
    assert len(bad) == 0, "%s: %d of %d keys differ, first key %d: the device has (%d, %d), the search gives %s" % (
        what, len(bad), len(ok), bad[0], got[bad[0], 0], got[bad[0], 1], (int(l[bad[0]]), int(r[bad[0]])) if ok[bad[0]] else "an empty interval")
    assert ok.any()
    key = int(np.nonzero(ok)[0][int(ok.sum()) // 2])   # the comparison bites: one l bumped in a copy is one key reported
    hurt = got.copy(); hurt[key, 0] += 1
    assert interval_table_diff(hurt, l, r, ok).tolist() == [key]


@pytest.mark.parametrize("name", CASES + TINY)
def test_prefix_and_jump_table_are_the_sbwt_intervals(name):
    """ptab at T = 1, 4, 7 -- and T = k at k = 4, 5 --, jtab up to J = k - 1 (k = 4, 5, 9): (l, r) of every key whose string ends a node, l > r for every other"""
    c = upload_case(name); h = upload_case_host(c); k = c.k
    for T, J in ((1, 8), (4, 5), (7, 1)) if k >= 12 else ((min(k, 7), k - 1), (1, 1), (4, 2)):
        p = upload(c, ptab_t=T, jtab_t=J)
        assert p.prefix_table_depth() == T and p.jump_table_depth() == J
        check_interval_table(p.debug_table(fa.DT_PTAB), h, T, "%s ptab T=%d" % (name, T))
        check_interval_table(p.debug_table(fa.DT_JTAB), h, J, "%s jtab J=%d" % (name, J))
        p.close()
    p = upload(c, jtab_t=0)   # (lean tables, the default up to k = 63: no prefix table)
    assert p.debug_table(fa.DT_JTAB) is None and (p.debug_table(fa.DT_PTAB) is None) == (p.prefix_table_depth() == 0)
    p.close()


@pytest.mark.parametrize("name", CASES + TINY)
def test_safe_places_and_reverse_complement_windows(name):
    """safe: on every position that ends a k-mer the bit says whether the oracle, asked for that k-mer alone, reports that place; the zero bits there are
    unsafe_places(); no bitmap means no unsafe place.  rcwin: the windows in which a k-mer ends whose reverse complement the text holds too, rc_pairs() such
    places; no table means none.  With lean tables (the count's search starts at the full interval) and without (it starts from the prefix table)"""
    c = upload_case(name); h = upload_case_host(c); k = c.k
    at, bit = memo(h, "safe", lambda: ref_safe(h.oracle, h.text, h.ends, k))
    win, n_rc = memo(h, "rcwin", lambda: ref_rcwin(h.text, h.ends, k))
    for options in ({}, {"lean_tables": 0}, {"lean_tables": 0, "ptab_t": min(k, 5)}):
        p = upload(c, **options)
        what = "%s %r" % (name, options)
        safe = p.debug_table(fa.DT_SAFE)
        assert p.unsafe_places() == int((bit == 0).sum()), what
        if safe is None:
            assert bit.all(), what
        else:
            assert safe.shape == ((len(h.text) + 63) // 64,) and not bit.all()
            got = bits_at(safe, at)
            bad = np.nonzero(got != bit)[0]
            assert len(bad) == 0, "%s: %d of %d k-mer places differ, first at text position %d: the device says %d" % (what, len(bad), len(at), at[bad[0]], got[bad[0]])
            g = int(at[len(at) // 2])   # the comparison bites: one bit flipped in a copy is one place reported
            hurt = safe.copy(); hurt[g >> 6] ^= np.uint64(1 << (g & 63))
            assert np.nonzero(bits_at(hurt, at) != bit)[0].tolist() == [len(at) // 2]
        rcwin = p.debug_table(fa.DT_RCWIN)
        assert p.rc_pairs() == n_rc, what
        if rcwin is None:
            assert not win.any(), what
        else:
            assert win.any() and rcwin.shape == win.shape
            assert_bit_tables_equal(rcwin, win, what + " rcwin")
        p.close()


@pytest.mark.parametrize("k", [16, 31, 33, 63])
def test_reads_that_ask_the_tables_where_the_answer_is_yes(k):
    """A read that follows unitig A and then carries 2k - 1 bases of unitig B's text: the strings behind the disagreeing base ARE in the index, so a filter or
    bitmap that lacks an entry turns found k-mers into absent ones.  Every offset of B for B = the first unitig of the text, the last, and one that ends on a
    multiple of 512; both orders, both strands; the oracle's pairs by default, without the fast path, without lean tables and on kernel 3"""
    c = upload_case("general_k%d" % k); h = upload_case_host(c)
    nu = len(h.ends)
    seam = next(u for u in range(nu - 1) if h.ends[u] % UPLOAD_SEG == 0 and h.ends[u] - h.starts[u] >= 2 * k - 1)
    reads = []
    for b in (0, nu - 1, seam):
        a = max((u for u in range(nu) if u != b), key=lambda u: h.ends[u] - h.starts[u])
        assert h.ends[b] - h.starts[b] >= 2 * k - 1
        reads += yes_reads(h.text, k, (h.starts[a], h.ends[a]), (h.starts[b], h.ends[b]))
    exp, _, _ = h.oracle.search_batch(reads)
    assert (exp[:, 0] != -1).sum() > len(exp) // 3
    lean, full = upload(c), upload(c, lean_tables=0)
    assert lean.lean_tables() and not full.lean_tables()
    for p, options in ((lean, {}), (lean, {"fast_path": 0}), (full, {}), (lean, {"kernel": 3})):
        for name, value in options.items():
            p.set_option(name, value)
        try:
            got, _ = p.search_reads(reads, fa.FIN_MERGED)
        finally:
            for name in options:
                p.set_option(name, None)
        bad = np.nonzero((got.astype(np.int64) != exp).any(axis=1))[0]
        assert len(bad) == 0, "k=%d %s %r: %d of %d pairs differ, first slot %d: got %s, the oracle %s" % (
            k, "lean" if p is lean else "full", options, len(bad), len(exp), bad[0], got[bad[0]].tolist(), exp[bad[0]].tolist())
    lean.close(); full.close()
