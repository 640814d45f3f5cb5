"""Per-read summaries, the parts that need no GPU (include/finito_amd.h: fin_read_summary, fin_records_read_summaries): the definition written out in numpy over
the pairs a record set means (tests/test_records.py::brute_expand), the host function against it on the hand-made records of tests/util.py, what is refused, and
the command's usage rules for --read-summary and --screen."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from tests.test_records import brute_expand
from tests.test_segments_host import segments_of
from tests.util import hand_made_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def summaries_of(pairs, nks):
    """the definition (include/finito_amd.h), over a read set's pairs back to back, read r has nks[r] of them: n_segments and longest from the segments of
    tests/test_segments_host.py::segments_of, n_found and span straight from the pair column"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    nks = np.asarray(nks, dtype=np.int64)
    seg_offs, segs = segments_of(pairs, nks)
    seg_offs = seg_offs.astype(np.int64)
    out = np.zeros(len(nks), dtype=fa.READ_SUMMARY_DTYPE)
    out["n_segments"] = np.diff(seg_offs)
    n_abs = np.abs(segs["len"].astype(np.int64))
    at = np.concatenate([[0], np.cumsum(nks)])
    for r in range(len(nks)):
        if seg_offs[r + 1] > seg_offs[r]:
            out["longest"][r] = n_abs[seg_offs[r]:seg_offs[r + 1]].max()
        found = np.nonzero(pairs[at[r]:at[r + 1], 0] != -1)[0]
        out["n_found"][r] = len(found)
        out["span"][r] = found[-1] - found[0] + 1 if len(found) else 0
    return out


def assert_summaries(got, want, what=""):
    assert got.dtype == fa.READ_SUMMARY_DTYPE and got.shape == want.shape, what
    for f in ("n_found", "n_segments", "longest", "span"):
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, "%s: field %s differs in %d reads, first %d: got %s, want %s" % (what, f, len(bad), bad[0], got[bad[0]], want[bad[0]])


def rule(summ, nks, min_found, min_permille, invert):
    """the screen's rule, literally, in Python integers"""
    return np.array([(int(f) >= min_found and 1000 * int(f) >= min_permille * int(nk)) != bool(invert) for f, nk in zip(summ["n_found"], nks)], dtype=bool)


def test_the_numpy_definition_on_small_reads():
    two = summaries_of([(3, o) for o in (5, 6, 5, 6, 5)] + [(-1, -1), (2, 9), (2, 8), (-1, -1), (4, 1), (-1, -1)], [5, 6])
    assert [tuple(x) for x in two.tolist()] == [(5, 4, 2, 5), (3, 2, 2, 4)]
    assert [tuple(x) for x in summaries_of(np.zeros((0, 2)), [0, 0]).tolist()] == [(0, 0, 0, 0)] * 2
    assert [tuple(x) for x in summaries_of([(-1, -1)] * 3, [3]).tolist()] == [(0, 0, 0, 0)]
    # reversing the slot order changes none of the four
    p = np.array([(-1, -1), (2, 9), (2, 8), (2, 7), (-1, -1), (4, 1), (4, 2), (-1, -1), (-1, -1)])
    assert summaries_of(p, [9]).tolist() == summaries_of(p[::-1], [9]).tolist() == [(5, 2, 3, 6)]


@pytest.mark.parametrize("k", [16, 31, 63])
def test_host_summaries_of_hand_made_records(k):
    c = hand_made_case(k)
    want = summaries_of(c.pairs, c.nks)
    kinds = c.recs["meta"] >> 16
    rev = (c.recs["meta"] >> 8) & 1
    # conditions on the input: every kind, both strands, 5 to 8 positions, reads of 0, 1 and several stretches, gaps inside and clipped ends
    assert all((kinds == x).sum() > 100 for x in (0, 1, 2)) and ((kinds == 1) & (rev == 1)).sum() > 100
    assert (((c.recs["meta"] & 0xFF) >= 5) & (kinds == 1)).sum() > 100
    one = want[kinds == 1]
    assert (one["n_segments"] == 0).any() and (one["n_segments"] == 1).any() and (one["n_segments"] >= 3).any()   # (nine: the test below; reads of 300 bases have no room)
    assert (one["span"] > one["n_found"]).any() and (one["span"] < c.nks[kinds == 1]).any()
    assert (want["n_found"][kinds == 2] == 0).all() and (want[kinds == 0]["n_segments"] >= 3).any()
    got = fa.records_read_summaries(c.recs, c.stream, k)
    assert_summaries(got, want, "k=%d" % k)
    assert int(got["n_found"].astype(np.int64).sum()) == int((c.pairs[:, 0] != -1).sum())
    one_thread, eight = fa.records_read_summaries(c.recs, c.stream, k, n_threads=1), fa.records_read_summaries(c.recs, c.stream, k, n_threads=8)
    assert one_thread.tobytes() == eight.tobytes() == got.tobytes()


def test_a_record_with_eight_gaps_is_nine_stretches_on_either_strand():
    k = 4
    for rev in (0, 1):
        recs = np.zeros(1, dtype=fa.RECORD_DTYPE)
        Es = [10 + 12 * e for e in range(8)]
        recs["u"], recs["off0"], recs["nk"], recs["meta"] = 7, 100, 120, 8 | (rev << 8) | (1 << 16)
        recs["Es"] = sum(E << (16 * e) for e, E in enumerate(Es[:4])); recs["Es2"] = sum(E << (16 * e) for e, E in enumerate(Es[4:]))
        pairs = brute_expand(recs, np.zeros((0, 2), np.int32), k)
        got = fa.records_read_summaries(recs, np.zeros((0, 2), np.int32), k)
        assert_summaries(got, summaries_of(pairs, recs["nk"]), "rev=%d" % rev)
        assert tuple(got[0].tolist()) == (120 - 8 * 4, 9, 25, 120)   # gaps [7, 10], [19, 22] .. [91, 94]: stretches of 7, seven of 8, and [95, 119] = 25


def test_refusals():
    c = hand_made_case(31)
    for threads in (1, 8):
        with pytest.raises(fa.FinitoError) as e:   # a truncated stream
            fa.records_read_summaries(c.recs, c.stream[:-1], 31, n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
        with pytest.raises(fa.FinitoError) as e:   # a stream with pairs to spare
            fa.records_read_summaries(c.recs, np.concatenate([c.stream, c.stream[:3]]), 31, n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
        bad = np.array(c.stream); bad[len(bad) // 2] = (-2, 5)   # neither found nor (-1,-1)
        with pytest.raises(fa.FinitoError) as e:
            fa.records_read_summaries(c.recs, bad, 31, n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
    assert len(fa.records_read_summaries(np.zeros(0, fa.RECORD_DTYPE), np.zeros((0, 2), np.int32), 31)) == 0   # nothing is legal


def test_null_arguments_are_refused_before_any_device_call():
    L = fa.lib()
    err = C.create_string_buffer(512)
    n = C.c_uint64(0)
    assert L.fin_batch_read_summaries(None, err, 512) == fa.FIN_EINVAL and b"null" in err.value
    assert L.fin_batch_download_read_summaries(None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_batch_screen(None, 1, 0, 0, C.byref(n), err, 512) == fa.FIN_EINVAL
    assert L.fin_batch_download_screen(None, None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_batch_device_read_summaries(None) is None and L.fin_batch_device_screen_ids(None) is None and L.fin_batch_device_screen_bits(None) is None
    assert L.fin_search_batch_read_summaries(None, None, None, 0, fa.FIN_MERGED, None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_search_batch_screen(None, None, None, 0, fa.FIN_MERGED, 1, 0, 0, None, None, err, 512) == fa.FIN_EINVAL
    idx = fa.FinimizerIndex.build(["ACGGT", "CGGTA"], 4)
    offs = (C.c_uint64 * 2)(0, 6)
    out = (C.c_uint32 * 4)()
    assert L.fin_search_batch_read_summaries(idx.h, b"ACGGTA", offs, 1, fa.FIN_MERGED, None, None, err, 512) == fa.FIN_EINVAL   # no room for the summaries
    assert L.fin_search_batch_read_summaries(idx.h, b"ACGGTA", offs, 1, 7, out, None, err, 512) == fa.FIN_EINVAL                 # strands
    assert L.fin_search_batch_screen(idx.h, b"ACGGTA", offs, 1, fa.FIN_MERGED, 1, 1001, 0, None, None, err, 512) == fa.FIN_EINVAL and b"1000" in err.value
    assert L.fin_records_read_summaries(None, 5, None, 0, 31, out, 1) == fa.FIN_EINVAL
    assert L.fin_records_read_summaries(None, 0, None, 0, 31, None, 1) == fa.FIN_OK


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_summary_entry_points_fail_loudly_without_device():
    """No CPU fallback: without a HIP device the device entry points raise, they do not compute"""
    idx = fa.FinimizerIndex.build(["ACGGT", "CGGTA"], 4)
    with pytest.raises(fa.FinitoError) as e:
        idx.search_reads_summaries(["ACGGTA"])
    assert e.value.code == -3
    with pytest.raises(fa.FinitoError) as e:
        idx.screen_reads(["ACGGTA"])
    assert e.value.code == -3
    with pytest.raises(fa.FinitoError) as e:
        idx.batch(["ACGGTA"]).read_summaries()
    assert e.value.code == -3


def test_cli_usage_rules(tmp_path):
    common = [BIN, "search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq")]
    r = subprocess.run([BIN, "search-fmin", "--help"], capture_output=True, text=True)
    assert all(x in r.stderr for x in ("--read-summary", "--screen", "--min-found", "--min-permille", "--screen-invert"))
    r = subprocess.run(common + ["--no-text", "1"], capture_output=True, text=True)
    assert r.returncode == 1 and "--read-summary" in r.stderr and "--screen" in r.stderr and not r.stdout
    # with either flag --no-text 1 is legal: the run gets as far as the query file / index it cannot find
    for flag in ("--read-summary", "--screen"):
        r = subprocess.run(common + ["--no-text", "1", flag, str(tmp_path / "s.tsv")], capture_output=True, text=True)
        assert r.returncode == 1 and "--no-text" not in r.stderr
    r = subprocess.run(common + ["--min-found", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and "--screen" in r.stderr
    r = subprocess.run(common + ["--screen", str(tmp_path / "p.txt"), "--min-permille", "1001"], capture_output=True, text=True)
    assert r.returncode == 1 and "--min-permille" in r.stderr and "1000" in r.stderr
