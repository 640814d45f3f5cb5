"""Results as segments, the parts that need no GPU (include/finito_amd.h: fin_segment, fin_records_segments, fin_expand_segments): the host-side segmentation
against the definition written out in numpy over fin_expand_records' pairs, the rule's edges on hand-made slots, what is refused, loud failure of the device entry
points on a box without a device, and the command's usage rules for --segments."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from tests.test_unitig_coverage_host import made_up_ends, random_record_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def segments_of_read(pairs):
    """the definition (include/finito_amd.h), over one read's pairs [nk, 2]: links from neighbouring slots, heads from two links, a segment from its head to the
    slot before the next head or the next absent slot"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    nk = len(p)
    found = p[:, 0] != -1
    link = np.zeros(nk, dtype=np.int64)
    if nk > 1:
        both = found[1:] & found[:-1] & (p[1:, 0] == p[:-1, 0])
        d = p[1:, 1] - p[:-1, 1]
        link[1:] = np.where(both & (d == 1), 1, np.where(both & (d == -1), -1, 0))
    before = np.concatenate([[0], link[:-1]])
    head = found & ((link == 0) | ((before != 0) & (before != link)))
    heads = np.nonzero(head)[0]
    stops = np.concatenate([np.nonzero(head | ~found)[0], [nk]])
    n = stops[np.searchsorted(stops, heads, side="right")] - heads
    out = np.zeros(len(heads), dtype=fa.SEGMENT_DTYPE)
    out["u"], out["off"], out["slot"] = p[heads, 0], p[heads, 1], heads
    out["len"] = np.where(n > 1, n * link[np.minimum(heads + 1, max(nk - 1, 0))], 1) if len(heads) else 0
    return out


def segments_of(pairs, nks):
    """(seg_offs, segs) of a read set: `pairs` back to back, read r has nks[r] of them"""
    at, parts, offs = 0, [], [0]
    for nk in np.asarray(nks, dtype=np.int64):
        parts.append(segments_of_read(pairs[at:at + nk])); at += int(nk)
        offs.append(offs[-1] + len(parts[-1]))
    assert at == len(pairs)
    return np.array(offs, dtype=np.uint64), (np.concatenate(parts) if parts else np.zeros(0, dtype=fa.SEGMENT_DTYPE))


def assert_segments(got, want, what=""):
    (go, gs), (wo, ws) = got, want
    assert go.dtype == np.uint64 and gs.dtype == fa.SEGMENT_DTYPE, what
    assert np.array_equal(go, wo), "%s: seg_offs differ, first at read %d" % (what, int(np.nonzero(go != wo)[0][0]) if go.shape == wo.shape else -1)
    for f in ("u", "off", "slot", "len"):
        bad = np.nonzero(gs[f] != ws[f])[0]
        assert len(bad) == 0, "%s: field %s differs in %d segments, first %d: got %s, want %s" % (what, f, len(bad), bad[0], gs[bad[0]], ws[bad[0]])


def one_read(slots):
    """a record set of one kind-0 read with the given (u, off) slots"""
    recs = np.zeros(1, dtype=fa.RECORD_DTYPE)
    recs["nk"] = len(slots)
    return recs, np.array(slots, dtype=np.int32).reshape(-1, 2)


def test_the_numpy_definition_on_the_issue_examples():
    s = segments_of_read([(3, o) for o in (5, 6, 5, 6, 5)])
    assert [tuple(x) for x in s.tolist()] == [(3, 5, 0, 2), (3, 5, 2, 1), (3, 6, 3, 1), (3, 5, 4, 1)]
    s = segments_of_read([(3, o) for o in (6, 5, 6, 7)])
    assert [tuple(x) for x in s.tolist()] == [(3, 6, 0, -2), (3, 6, 2, 2)]


def test_host_segments_against_the_definition_over_the_expanded_pairs():
    rng = np.random.default_rng(410)
    nine = 0
    for k in (4, 21, 31, 63):
        ends = made_up_ends(rng, k)
        recs, stream = random_record_set(rng, k, ends)
        pairs, npos = fa.expand_records(recs, stream, k)
        want = segments_of(pairs, recs["nk"])
        per_read = np.diff(want[0].astype(np.int64))
        # conditions on the inputs
        assert (want[1]["len"] < -1).any() and (want[1]["len"] > 1).any() and (want[1]["len"] == 1).any() and (per_read >= 3).any()
        assert (recs["meta"] >> 16 == 1).sum() > 500 and (recs["meta"] >> 16 == 2).sum() > 500 and len(stream) > 10000
        nine += int(((recs["meta"] >> 16 == 1) & (per_read == 9)).sum())
        for threads in (1, 3, 0):
            got = fa.records_segments(recs, stream, k, n_threads=threads)
            assert_segments(got, want, "k=%d threads=%d" % (k, threads))
            back, pos = fa.expand_segments(got[0], got[1], recs["nk"], n_threads=threads)
            assert np.array_equal(back, pairs) and pos == npos == int((pairs[:, 0] != -1).sum()) == int(np.abs(got[1]["len"].astype(np.int64)).sum())
        # a read's segments are ordered by slot and do not overlap
        so, sg = want
        ends_of = sg["slot"].astype(np.int64) + np.abs(sg["len"].astype(np.int64))
        inner = np.ones(len(sg), dtype=bool); inner[so[:-1][per_read > 0].astype(np.int64)] = False
        assert (sg["slot"].astype(np.int64)[inner] >= ends_of[np.nonzero(inner)[0] - 1]).all()
    assert nine > 0, "no kind-1 read with nine segments"


def test_a_record_with_eight_gaps_is_nine_segments_on_either_strand():
    k = 4
    for rev in (0, 1):
        recs = np.zeros(1, dtype=fa.RECORD_DTYPE)
        Es = [10 + 12 * e for e in range(8)]
        recs["u"], recs["off0"], recs["nk"], recs["meta"] = 7, 100, 120, 8 | (rev << 8) | (1 << 16)
        recs["Es"] = sum(E << (16 * e) for e, E in enumerate(Es[:4])); recs["Es2"] = sum(E << (16 * e) for e, E in enumerate(Es[4:]))
        pairs, _ = fa.expand_records(recs, np.zeros((0, 2), np.int32), k)
        got = fa.records_segments(recs, np.zeros((0, 2), np.int32), k)
        assert len(got[1]) == 9 and ((got[1]["len"] < 0).all() if rev else (got[1]["len"] > 0).all())
        assert_segments(got, segments_of(pairs, recs["nk"]), "rev=%d" % rev)
        if rev:   # `off` is the stretch's highest offset
            assert got[1]["off"][0] == 100 + 119 and got[1]["slot"][0] == 0


def test_the_rules_edges_on_hand_made_slots():
    def seg(slots):
        recs, stream = one_read(slots)
        got = fa.records_segments(recs, stream, 31)
        assert_segments(got, segments_of(stream, [len(slots)]), str(slots[:8]))
        assert np.array_equal(fa.expand_segments(got[0], got[1], [len(slots)])[0], stream.reshape(-1, 2))
        return [tuple(int(v) for v in x) for x in got[1].tolist()]
    assert seg([(2, o) for o in (5, 6, 5, 6, 5)]) == [(2, 5, 0, 2), (2, 5, 2, 1), (2, 6, 3, 1), (2, 5, 4, 1)]
    assert seg([(2, o) for o in (6, 5, 6, 7)]) == [(2, 6, 0, -2), (2, 6, 2, 2)]
    assert seg([(2, o) for o in (5, 6, 5, 4)]) == [(2, 5, 0, 2), (2, 5, 2, -2)]
    assert seg([(2, 5), (2, 6), (2, 6), (2, 7)]) == [(2, 5, 0, 2), (2, 6, 2, 2)]            # a repeated identical pair
    assert seg([(2, 9), (2, 9), (2, 9)]) == [(2, 9, 0, 1), (2, 9, 1, 1), (2, 9, 2, 1)]        # a homopolymer's slots
    assert seg([(2, 5), (2, 6), (3, 7), (3, 8)]) == [(2, 5, 0, 2), (3, 7, 2, 2)]            # a unitig change with consecutive offsets
    assert seg([(2, 5), (-1, -1), (2, 6), (2, 7)]) == [(2, 5, 0, 1), (2, 6, 2, 2)]          # an absent slot between consecutive offsets
    assert seg([(4, o) for o in range(40, 50)]) == [(4, 40, 0, 10)]                         # a run that touches slot 0 and slot nk - 1
    assert seg([(4, o) for o in range(49, 39, -1)]) == [(4, 49, 0, -10)]
    assert seg([(-1, -1)] * 3 + [(4, 40)] + [(-1, -1)] * 2) == [(4, 40, 3, 1)]
    assert seg([]) == [] and seg([(1, 0)]) == [(1, 0, 0, 1)] and seg([(-1, -1)]) == []      # nk = 0, nk = 1
    assert seg([(4, o) for o in range(100, 200)]) == [(4, 100, 0, 100)]                     # a run longer than 64
    assert seg([(-1, -1)] + [(4, o) for o in range(6000, 1000, -1)] + [(4, 7)]) == [(4, 6000, 1, -5000), (4, 7, 5001, 1)]   # longer than 4 096
    assert seg([(4, o) for o in range(0, 63)] + [(4, 63), (4, 62)]) == [(4, 0, 0, 64), (4, 62, 64, 1)]


def test_refusals():
    rng = np.random.default_rng(411)
    ends = made_up_ends(rng, 31)
    recs, stream = random_record_set(rng, 31, ends, n=2500)
    seg_offs, segs = fa.records_segments(recs, stream, 31)
    for threads in (1, 3):
        with pytest.raises(fa.FinitoError) as e:   # a truncated stream
            fa.records_segments(recs, stream[:-1], 31, n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
        with pytest.raises(fa.FinitoError) as e:   # a stream with pairs to spare
            fa.records_segments(recs, np.concatenate([stream, stream[:3]]), 31, n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
        with pytest.raises(fa.FinitoError) as e:   # room for one segment too few
            fa.records_segments(recs, stream, 31, seg_cap=len(segs) - 1, n_threads=threads)
        assert e.value.code == fa.FIN_ELIMIT
        assert_segments(fa.records_segments(recs, stream, 31, seg_cap=len(segs), n_threads=threads), (seg_offs, segs))
        r = int(np.nonzero(np.diff(seg_offs.astype(np.int64)) >= 2)[0][0]); a = int(seg_offs[r])
        def refused(change):
            bad = segs.copy(); change(bad)
            with pytest.raises(fa.FinitoError) as e:
                fa.expand_segments(seg_offs, bad, recs["nk"], n_threads=threads)
            assert e.value.code == fa.FIN_EINVAL
        def overlap(s): s["slot"][a + 1] = s["slot"][a] + abs(int(s["len"][a])) - 1
        def unsorted(s): s[[a, a + 1]] = s[[a + 1, a]]
        def outside(s): s["slot"][a + 1] = int(recs["nk"][r]) - abs(int(s["len"][a + 1])) + 1
        def empty(s): s["len"][a] = 0
        for change in (overlap, unsorted, outside, empty):
            refused(change)
        one = np.zeros(1, dtype=fa.SEGMENT_DTYPE)
        one["u"], one["off"], one["slot"], one["len"] = 1, 1, 0, -2
        assert fa.expand_segments([0, 1], one, [5], n_threads=threads)[0].tolist() == [[1, 1], [1, 0], [-1, -1], [-1, -1], [-1, -1]]
        one["off"] = 0                           # the offset sequence would go negative
        with pytest.raises(fa.FinitoError) as e:
            fa.expand_segments([0, 1], one, [5], n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
        fa.expand_segments(seg_offs, segs, recs["nk"], n_threads=threads)   # the untouched set passes
    with pytest.raises(fa.FinitoError):   # seg_offs that does not fit the reads
        fa.expand_segments(seg_offs[:-1], segs, recs["nk"])


def test_null_arguments_are_refused_before_any_device_call():
    L = fa.lib()
    err = C.create_string_buffer(512)
    n = C.c_uint64(0)
    assert L.fin_batch_segments(None, C.byref(n), err, 512) == fa.FIN_EINVAL and b"null" in err.value
    assert L.fin_batch_download_segments(None, None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_batch_device_segments(None) is None and L.fin_batch_device_segment_offsets(None) is None
    assert L.fin_search_batch_segments(None, None, None, 0, fa.FIN_MERGED, None, None, 0, None, None, err, 512) == fa.FIN_EINVAL
    idx = fa.FinimizerIndex.build(["ACGGT", "CGGTA"], 4)
    offs = (C.c_uint64 * 2)(0, 6)
    so = (C.c_uint64 * 2)()
    assert L.fin_search_batch_segments(idx.h, b"ACGGTA", offs, 1, fa.FIN_MERGED, None, None, 0, None, None, err, 512) == fa.FIN_EINVAL     # no seg_offs
    assert L.fin_search_batch_segments(idx.h, b"ACGGTA", offs, 1, 7, so, None, 0, None, None, err, 512) == fa.FIN_EINVAL                   # strands
    assert L.fin_search_batch_segments(idx.h, b"ACGGTA", offs, 1, fa.FIN_MERGED, so, None, 3, None, None, err, 512) == fa.FIN_EINVAL       # room without a buffer
    assert L.fin_expand_segments(None, None, 0, None, None, None, 1) == fa.FIN_EINVAL
    assert L.fin_expand_segments(so, None, 1, None, None, None, 1) == fa.FIN_EINVAL
    assert L.fin_records_segments(None, 5, None, 0, 31, so, None, 0, None, 1) == fa.FIN_EINVAL
    assert L.fin_records_segments(None, 0, None, 0, 31, None, None, 0, None, 1) == fa.FIN_EINVAL
    assert L.fin_records_segments(None, 0, None, 0, 31, so, None, 0, C.byref(n), 1) == fa.FIN_OK and n.value == 0 and so[0] == 0   # nothing is legal


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_segment_entry_points_fail_loudly_without_device():
    """No CPU fallback: without a HIP device the device entry points raise, they do not compute"""
    idx = fa.FinimizerIndex.build(["ACGGT", "CGGTA"], 4)
    with pytest.raises(fa.FinitoError) as e:
        idx.search_reads_segments(["ACGGTA"])
    assert e.value.code == -3
    with pytest.raises(fa.FinitoError) as e:
        idx.search_reads_segments([])
    assert e.value.code == -3
    with pytest.raises(fa.FinitoError) as e:
        idx.batch(["ACGGTA"]).segments()
    assert e.value.code == -3


def test_cli_usage_rules(tmp_path):
    common = [BIN, "search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq")]
    r = subprocess.run([BIN, "search-fmin", "--help"], capture_output=True, text=True)
    assert "--segments" in r.stderr and "--unitig-coverage" in r.stderr and "--no-text" in r.stderr
    r = subprocess.run(common + ["--no-text", "1"], capture_output=True, text=True)
    assert r.returncode == 1 and "--segments" in r.stderr and "--unitig-counts" in r.stderr and "--unitig-coverage" in r.stderr and not r.stdout
    # with --segments, --no-text 1 is legal: the run gets as far as the query file / index it cannot find
    r = subprocess.run(common + ["--no-text", "1", "--segments", str(tmp_path / "s.tsv")], capture_output=True, text=True)
    assert r.returncode == 1 and "--no-text" not in r.stderr
