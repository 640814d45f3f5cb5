"""Reference coordinates on the host (include/finito_amd.h: REFERENCE COORDINATES; fin_refpaths_host.cpp): the twins fin_segments_check,
fin_segments_window_depth and fin_segments_lift_variants against a plain-Python model written from the header's definitions, on hand-made path sets.  Every
comparison is exact.  No GPU."""
import numpy as np
import pytest

import finito_amd as fa

K = 5
LENS = (12, 5, 30, 9, 2000, 70)          # nk = 8, 1, 26, 5, 1996, 66
ENDS = np.cumsum(LENS).astype(np.int64)    # FIN_X_ENDS
THREADS = (1, 3, 16)
WINDOWS = (1, 7, 64, 1000, 5000)           # the last one is larger than every sequence below


def starts_of(ends):
    return np.concatenate([[0], np.asarray(ends, dtype=np.int64)[:-1]])


def seg(u, off, slot, ln):
    return (u, off, slot, ln)


def path_set(seqs):
    """[(nk, [segments])] -> (seq_nk, seg_offs, segs)"""
    nk = np.array([s[0] for s in seqs], dtype=np.uint32)
    so = np.cumsum([0] + [len(s[1]) for s in seqs]).astype(np.uint64)
    sg = np.array([x for s in seqs for x in s[1]], dtype=fa.SEGMENT_DTYPE).reshape(-1)
    return nk, so, sg


# ---- the model: the header's definitions, nothing else ----------------------------------------------------------------------------------------------
def invalid_clause(seq_nk, seg_offs, segs, k, ends):
    """None, or (segment, clause) of the first segment that is not valid"""
    ends = np.asarray(ends, dtype=np.int64); st = starts_of(ends)
    for s in range(len(seq_nk)):
        nxt = 0
        for i in range(int(seg_offs[s]), int(seg_offs[s + 1])):
            u, off, slot, ln = (int(segs[i][f]) for f in ("u", "off", "slot", "len"))
            n = abs(ln)
            if not 0 <= u < len(ends): return i, "unitig number outside the index"
            if n == 0: return i, "len is 0"
            if slot + n > int(seq_nk[s]): return i, "leaves the sequence's slots"
            if slot < nxt: return i, "overlaps or precedes"
            nxt = slot + n
            nku = max(0, int(ends[u] - st[u]) - k + 1)
            ok = (off >= 0 and off + n - 1 < nku) if ln > 0 else (off - (n - 1) >= 0 and off < nku)
            if not ok: return i, "offsets outside the unitig's k-mers"
    return None


def window_offsets(seq_nk, window):
    return np.cumsum([0] + [-(-int(x) // window) for x in seq_nk]).astype(np.uint64)


def model_windows(seq_nk, seg_offs, segs, ends, depth, window, min_depth):
    st = starts_of(ends)
    wo = window_offsets(seq_nk, window)
    out = np.zeros(int(wo[-1]), dtype=fa.REF_WINDOW_DTYPE)
    floor = max(int(min_depth), 1)
    for s in range(len(seq_nk)):
        for i in range(int(seg_offs[s]), int(seg_offs[s + 1])):
            u, off, slot, ln = (int(segs[i][f]) for f in ("u", "off", "slot", "len"))
            j = np.arange(abs(ln), dtype=np.int64)
            g = st[u] + off + (j if ln > 0 else -j)
            w = int(wo[s]) + (slot + j) // window
            d = np.asarray(depth)[g].astype(np.uint64)
            np.add.at(out["depth_sum"], w, d)
            np.add.at(out["in_graph"], w, 1)
            np.add.at(out["covered"], w, (d >= floor).astype(np.uint32))
    return wo, out


def model_lift(seq_nk, seg_offs, segs, ends, k, variants):
    v = np.asarray(variants, dtype=fa.VARIANT_DTYPE).reshape(-1)
    vu, voff = v["u"].astype(np.int64), v["off"].astype(np.int64)
    rows = []
    for s in range(len(seq_nk)):
        for i in range(int(seg_offs[s]), int(seg_offs[s + 1])):
            u, off, slot, ln = (int(segs[i][f]) for f in ("u", "off", "slot", "len"))
            n = abs(ln)
            lo, hi = (off, off + n + k - 2) if ln > 0 else (off - n + 1, off + k - 1)
            inside = np.nonzero((vu == u) & (voff >= lo) & (voff <= hi))[0]
            pos = slot + (voff[inside] - off) if ln > 0 else slot + (off + k - 1 - voff[inside])
            for q in np.argsort(pos, kind="stable"):
                rows.append((s, int(pos[q]), int(inside[q]), 0 if ln > 0 else 1))
    return np.array(rows, dtype=fa.REF_VARIANT_DTYPE).reshape(-1)


def variants_at(places, ends):
    """VARIANT_DTYPE for (u, off) places, sorted ascending in start(u) + off"""
    st = starts_of(ends)
    places = sorted(set(places), key=lambda p: st[p[0]] + p[1])
    v = np.zeros(len(places), dtype=fa.VARIANT_DTYPE)
    for i, (u, off) in enumerate(places):
        v[i] = (u, off, 10 + i, i % 4, [(i + j) % 5 if j != i % 4 else 0 for j in range(4)])
    return v


def assert_windows(got, want, what=""):
    wo, out = want
    assert got.win_offs.dtype == np.uint64 and np.array_equal(got.win_offs, wo), what
    assert got.windows.dtype == fa.REF_WINDOW_DTYPE and got.windows.shape == out.shape, what
    for f in ("depth_sum", "in_graph", "covered"):
        bad = np.nonzero(got.windows[f] != out[f])[0]
        assert len(bad) == 0, "%s: %s differs in %d windows, first %d: got %d, want %d" % (what, f, len(bad), bad[0], got.windows[f][bad[0]], out[f][bad[0]])


def assert_lift(got, want, what=""):
    assert got.dtype == fa.REF_VARIANT_DTYPE and got.shape == want.shape, "%s: %d records, want %d" % (what, len(got), len(want))
    for f in ("seq", "pos", "var", "flags"):
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, "%s: %s differs in %d records, first %d: got %s, want %s" % (what, f, len(bad), bad[0], got[bad[0]], want[bad[0]])


# ---- path sets ----------------------------------------------------------------------------------------------------------------------------------------
def hand_set():
    """every shape the issue names; unitig 4 (nk 1996) is crossed by three sequences and twice by sequence 6"""
    return [
        (1, [seg(1, 0, 0, 1)]),                                         # 0: a forward segment of one slot, n = nk(u) = 1
        (1, [seg(0, 7, 0, 1)]),                                         # 1: one slot at the last k-mer of its unitig
        (8, [seg(0, 7, 0, -8)]),                                        # 2: reverse, n = nk(u): touches both ends
        (0, []),                                                        # 3: nk = 0
        (40, []),                                                       # 4: no segment
        (30, [seg(2, 0, 2, 26)]),                                       # 5: forward, n = nk(u), touches both ends; slots 0, 1, 28, 29 have no place
        (3000, [seg(4, 0, 0, 1000), seg(4, 1995, 1000, -1000), seg(3, 4, 2100, -5), seg(2, 3, 2200, 4), seg(2, 7, 2204, 6)]),   # 6: ends exactly on the 1000 boundary; two segments sharing k - 1 bases (2200 / 2204)
        (2100, [seg(4, 5, 57, 135), seg(5, 65, 1990, -66)]),            # 7: at window 64, slots 57 .. 191 straddle three windows
        (70, [seg(4, 990, 0, 20), seg(4, 1009, 30, -20)]),              # 8: the same stretch of unitig 4 forward and reverse
        (64, [seg(4, 1900, 0, 64)]),                                    # 9: exactly one window of 64
    ]


def random_set(rng, n_seqs=40):
    nku = [max(0, l - K + 1) for l in LENS]
    seqs = []
    for _ in range(n_seqs):
        nk = int(rng.choice([0, 1, 5, 63, 64, 65, 300, 1500]))
        segs, slot = [], 0
        while slot < nk and rng.random() < 0.85:
            slot += int(rng.integers(0, 4))
            u = int(rng.integers(0, len(LENS)))
            n = int(rng.integers(1, min(nku[u], nk - slot) + 1)) if nk - slot >= 1 else 0
            if n < 1: break
            if rng.random() < 0.5: segs.append(seg(u, int(rng.integers(0, nku[u] - n + 1)), slot, n))
            else: segs.append(seg(u, int(rng.integers(n - 1, nku[u])), slot, -n if n > 1 else 1))
            slot += n
        seqs.append((nk, segs))
    return seqs


def random_depth(rng):
    d = rng.integers(0, 6, int(ENDS[-1])).astype(np.uint32)
    d[rng.integers(0, len(d), 200)] = 0xFFFFFFFF
    d[int(ENDS[3]):int(ENDS[3]) + 1200] = 0xFFFFFFF0     # a window of 1000 slots sums far beyond 2^32
    return d


@pytest.fixture(scope="module")
def depth():
    d = random_depth(np.random.default_rng(41))
    d.setflags(write=False)
    return d


def test_the_hand_set_is_valid_and_the_model_knows_a_few_numbers_by_heart(depth):
    nk, so, sg = path_set(hand_set())
    assert invalid_clause(nk, so, sg, K, ENDS) is None
    fa.segments_check(nk, so, sg, K, ENDS)
    wo, out = model_windows(nk, so, sg, ENDS, depth, 1000, 1)
    assert wo.tolist() == [0, 1, 2, 3, 3, 4, 5, 8, 11, 12, 13]
    w6 = out[5:8]
    assert w6["in_graph"].tolist() == [1000, 1000, 15]
    st4 = int(ENDS[3])
    assert int(w6["depth_sum"][0]) == int(depth[st4:st4 + 1000].astype(np.uint64).sum()) > 2**32
    assert int(w6["depth_sum"][1]) == int(depth[st4 + 996:st4 + 1996].astype(np.uint64).sum())
    one = model_windows(nk, so, sg, ENDS, depth, 1, 1)[1]
    assert len(one) == int(nk.sum()) and int(one["in_graph"].sum()) == int(np.abs(sg["len"]).sum())
    # the slot -> place map, slot by slot: sequence 2 runs down unitig 0 from its last k-mer
    assert one["depth_sum"][2:10].tolist() == depth[7::-1].tolist()


@pytest.mark.parametrize("threads", THREADS)
def test_window_depth_twin_against_the_model(depth, threads):
    rng = np.random.default_rng(5)
    for name, seqs in (("by hand", hand_set()), ("random", random_set(rng)), ("empty", []), ("no slots", [(0, []), (0, [])])):
        nk, so, sg = path_set(seqs)
        assert invalid_clause(nk, so, sg, K, ENDS) is None, name
        for window in WINDOWS:
            for md in (1, 3):
                got = fa.segments_window_depth(nk, so, sg, K, ENDS, depth, window, md, n_threads=threads)
                assert_windows(got, model_windows(nk, so, sg, ENDS, depth, window, md), "%s, window %d, min_depth %d, %d threads" % (name, window, md, threads))
        z = fa.segments_window_depth(nk, so, sg, K, ENDS, depth, 7, 0, n_threads=threads)
        assert_windows(z, model_windows(nk, so, sg, ENDS, depth, 7, 1), name + ": min_depth 0 counts as 1")
    nk, so, sg = path_set(hand_set())
    r = fa.segments_window_depth(nk, so, sg, K, ENDS, depth, 1000, 1, n_threads=threads)
    assert np.isnan(r.mean_depth[3]) and np.isnan(r.breadth[3]) and r.mean_depth[0] == float(depth[int(ENDS[0])]) and len(r.of(3)) == 0 and len(r.of(6)) == 3
    assert r.breadth[5] == r.windows["covered"][5] / 1000.0


def variant_places_for_hand_set():
    k = K
    places = []
    # sequence 6's forward segment {u 4, off 0, n 1000}: base interval [0, 1003]; its reverse one {off 1995, n 1000}: [996, 1999]
    places += [(4, 0), (4, 1003), (4, 1004), (4, 996), (4, 995), (4, 1999)]
    # sequence 7 {u 4, off 5, n 135}: [5, 143]; one outside either end
    places += [(4, 4), (4, 5), (4, 143), (4, 144)]
    # sequence 8 crosses [990, 1013] forward and [990, 1013] reverse
    places += [(4, 990), (4, 1000), (4, 1013), (4, 1014), (4, 989)]
    # the k - 1 bases the consecutive segments {u 2, off 3, n 4} and {u 2, off 7, n 6} of sequence 6 share: text offsets 7 .. 10 of unitig 2
    places += [(2, 3), (2, 7), (2, 8), (2, 10), (2, 11), (2, 16), (2, 17), (2, 2)]
    # reverse segments of one slot and of a whole unitig
    places += [(0, 0), (0, 7), (0, 11), (1, 0), (1, 4), (3, 0), (3, 4), (3, 8), (5, 0), (5, 69)]
    assert k == 5
    return places


@pytest.mark.parametrize("threads", THREADS)
def test_lift_twin_against_the_model(threads):
    rng = np.random.default_rng(6)
    nk, so, sg = path_set(hand_set())
    v = variants_at(variant_places_for_hand_set(), ENDS)
    want = model_lift(nk, so, sg, ENDS, K, v)
    assert_lift(fa.segments_lift_variants(nk, so, sg, K, ENDS, v, n_threads=threads), want, "by hand")
    # what the expectation shows: both ends of a forward and a reverse interval, the shared bases twice in one sequence, a unitig under three sequences
    by_var = {}
    for r in want:
        by_var.setdefault((int(v["u"][r["var"]]), int(v["off"][r["var"]])), []).append((int(r["seq"]), int(r["pos"]), int(r["flags"])))
    assert by_var[(4, 0)] == [(6, 0, 0)] and (6, 1003, 0) in by_var[(4, 1003)] and (4, 1004) in by_var and (6, 1003, 0) not in by_var[(4, 1004)]
    assert (6, 1000 + 1995 + K - 1 - 1999, 1) in by_var[(4, 1999)] and (6, 1000 + 1003, 1) in by_var[(4, 996)] and all(s != 6 or f == 0 for s, _, f in by_var[(4, 995)])
    assert (4, 4) not in by_var or all(s != 7 for s, _, _ in by_var[(4, 4)])
    assert (7, 57, 0) in by_var[(4, 5)] and (7, 57 + 138, 0) in by_var[(4, 143)] and all(s != 7 for s, _, _ in by_var.get((4, 144), []))
    assert sorted(by_var[(2, 8)]) == [(5, 2 + 8, 0), (6, 2200 + 5, 0), (6, 2204 + 1, 0)], "a base two consecutive segments share lies under both"
    assert {s for s, _, _ in by_var[(4, 1000)]} == {6, 8} and len([1 for s, _, _ in by_var[(4, 1000)] if s == 8]) == 2 and len([1 for s, _, _ in by_var[(4, 1000)] if s == 6]) == 2
    assert by_var[(1, 4)] == [(0, 4, 0)] and by_var[(0, 11)] == [(1, 4, 0), (2, 0, 1)] and by_var[(0, 0)] == [(2, 11, 1)]
    # pos ascends inside every segment, reverse ones included
    assert (want["flags"] & 1).sum() >= 8 and ((want["flags"] & 1) == 0).sum() >= 8
    got = fa.segments_lift_variants(nk, so, sg, K, ENDS, v, n_threads=threads)
    # pos ascends inside a segment: sequence 6 has ONE reverse segment in unitig 4 and sequence 7 ONE forward segment, each with several variants
    rev6 = got[(got["seq"] == 6) & (got["flags"] == 1) & (v["u"][got["var"]] == 4)]["pos"].astype(np.int64)
    fwd7 = got[(got["seq"] == 7) & (got["flags"] == 0)]["pos"].astype(np.int64)
    assert len(rev6) >= 5 and (np.diff(rev6) > 0).all() and len(fwd7) >= 2 and (np.diff(fwd7) > 0).all(), "pos does not ascend inside a segment"
    # n = 0, and a cap one too small
    assert len(fa.segments_lift_variants(nk, so, sg, K, ENDS, v[:0], n_threads=threads)) == 0
    assert len(fa.segments_lift_variants(nk, so, sg, K, ENDS, v, n_threads=threads, cap=len(want))) == len(want)
    with pytest.raises(fa.FinitoError) as e:
        fa.segments_lift_variants(nk, so, sg, K, ENDS, v, n_threads=threads, cap=len(want) - 1)
    assert e.value.code == fa.FIN_ELIMIT and e.value.n_out == len(want)
    with pytest.raises(fa.FinitoError) as e:
        fa.segments_window_depth(nk, so, sg, K, ENDS, np.zeros(int(ENDS[-1]), dtype=np.uint32), 7, 1, n_threads=threads, cap=int(window_offsets(nk, 7)[-1]) - 1)
    assert e.value.code == fa.FIN_ELIMIT and e.value.n_windows == int(window_offsets(nk, 7)[-1])
    # random path sets under random variants
    for trial in range(3):
        nk, so, sg = path_set(random_set(rng))
        st = starts_of(ENDS)
        g = np.sort(rng.choice(int(ENDS[-1]), 400, replace=False))
        u = np.searchsorted(ENDS, g, side="right")
        v = variants_at([(int(a), int(b)) for a, b in zip(u, g - st[u])], ENDS)
        assert_lift(fa.segments_lift_variants(nk, so, sg, K, ENDS, v, n_threads=threads), model_lift(nk, so, sg, ENDS, K, v), "random %d" % trial)


def ref_bases_by_hand():
    v = np.zeros(2, dtype=fa.VARIANT_DTYPE)
    v[0] = (0, 1, 9, 0, [0, 1, 2, 3]); v[1] = (0, 2, 9, 2, [5, 6, 0, 7])
    l = np.array([(0, 4, 0, 0), (0, 9, 1, 1), (1, 2, 0, 1)], dtype=fa.REF_VARIANT_DTYPE)
    return v, l


def test_ref_variant_bases_complements_reverse_records():
    v, l = ref_bases_by_hand()
    ref, alt = fa.ref_variant_bases(l, v)
    assert ref.tolist() == [0, 1, 3] and alt.tolist() == [[0, 1, 2, 3], [7, 0, 6, 5], [3, 2, 1, 0]]


BAD = [
    ("unitig number outside the index", [(10, [seg(6, 0, 0, 2)])]),
    ("unitig number outside the index", [(10, [seg(-1, 0, 0, 2)])]),
    ("len is 0", [(10, [seg(0, 0, 0, 0)])]),
    ("leaves the sequence's slots", [(10, [seg(2, 0, 5, 6)])]),
    ("overlaps or precedes", [(20, [seg(2, 0, 0, 6), seg(2, 10, 5, 3)])]),
    ("overlaps or precedes", [(20, [seg(2, 0, 8, 3), seg(2, 10, 2, 3)])]),
    ("offsets outside the unitig's k-mers", [(10, [seg(0, -1, 0, 2)])]),
    ("offsets outside the unitig's k-mers", [(10, [seg(0, 6, 0, 3)])]),       # forward: off + n - 1 = 8 = nk(u)
    ("offsets outside the unitig's k-mers", [(10, [seg(0, 1, 0, -3)])]),      # reverse: off - (n - 1) = -1
    ("offsets outside the unitig's k-mers", [(10, [seg(0, 8, 0, -3)])]),      # reverse: off = nk(u)
]


@pytest.mark.parametrize("clause,seqs", BAD, ids=["%d-%s" % (i, b[0].split()[0]) for i, b in enumerate(BAD)])
def test_every_clause_of_the_validity_rule_is_refused_by_name(clause, seqs):
    good = hand_set()
    nk, so, sg = path_set(good + seqs)
    first = invalid_clause(nk, so, sg, K, ENDS)
    assert first is not None and first[1] == clause and first[0] >= int(path_set(good)[1][-1])
    depth = np.zeros(int(ENDS[-1]), dtype=np.uint32)
    calls = (lambda: fa.segments_check(nk, so, sg, K, ENDS), lambda: fa.segments_window_depth(nk, so, sg, K, ENDS, depth, 7, 1),
             lambda: fa.segments_lift_variants(nk, so, sg, K, ENDS, variants_at([(0, 1)], ENDS)))
    for call in calls:
        with pytest.raises(fa.FinitoError) as e:
            call()
        assert e.value.code == fa.FIN_EINVAL and clause in str(e.value) and "segment %d " % first[0] in str(e.value), str(e.value)


def test_variants_that_do_not_ascend_or_lie_outside_the_index_are_refused_by_name():
    nk, so, sg = path_set(hand_set())
    good = variants_at([(0, 1), (0, 5), (2, 3)], ENDS)
    for what, edit in (("does not ascend", lambda v: v.__setitem__(1, v[0])), ("does not ascend", lambda v: v.__setitem__(slice(0, 2), v[[1, 0]])),
                       ("outside the index", lambda v: v["u"].__setitem__(2, 6)), ("outside the index", lambda v: v["off"].__setitem__(2, 30))):
        v = good.copy(); edit(v)
        with pytest.raises(fa.FinitoError) as e:
            fa.segments_lift_variants(nk, so, sg, K, ENDS, v)
        assert e.value.code == fa.FIN_EINVAL and what in str(e.value), str(e.value)
    with pytest.raises(fa.FinitoError) as e:
        fa.segments_window_depth(nk, so, sg, K, ENDS, np.zeros(int(ENDS[-1]), dtype=np.uint32), 0, 1)
    assert e.value.code == fa.FIN_EINVAL and "window" in str(e.value)
