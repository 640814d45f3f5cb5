"""Read classification by unitig labels, the parts that need no GPU (include/finito_amd.h: fin_read_class, fin_records_read_classes): the definition written out
in numpy over the pairs a record set means (tests/test_records.py::brute_expand), the rule of assignment, the host function against the definition on the
hand-made records of tests/util.py, what is refused, and the command's usage rules for --classify and --label-report."""
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
NONE = 0xFFFFFFFF


def classes_of(pairs, nks, labels):
    """the definition (include/finito_amd.h), over a read set's pairs back to back, read r has nks[r] of them; labels[u] = unitig u's label or NONE.  A loop over
    the reads, np.bincount over the labels of each read's found slots; np.argmax returns the first maximum: a tie goes to the smaller label"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    nks = np.asarray(nks, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    out = np.zeros(len(nks), dtype=fa.READ_CLASS_DTYPE)
    at = np.concatenate([[0], np.cumsum(nks)])
    for r in range(len(nks)):
        u = pairs[at[r]:at[r + 1], 0]
        lab = labels[u[u != -1]]
        lab = lab[lab != NONE]
        if len(lab) == 0:
            out[r] = (NONE, 0, 0, 0)
            continue
        c = np.bincount(lab)
        best = int(np.argmax(c))
        rest = np.delete(c, best)
        out[r] = (best, c[best], rest.max() if len(rest) else 0, len(lab))
    return out


def assigned(classes, nks, min_found, min_permille, min_margin):
    """the rule of assignment, literally, in Python integers: the tally slot of every read, -1 for an unassigned one"""
    out = np.full(len(classes), -1, dtype=np.int64)
    for r, (c, nk) in enumerate(zip(classes, nks)):
        nb, ns = int(c["n_best"]), int(c["n_second"])
        if nb >= max(min_found, 1) and 1000 * nb >= min_permille * int(nk) and nb >= ns + min_margin:
            out[r] = int(c["label"])
    return out


def tally_of(classes, nks, n_labels, min_found, min_permille, min_margin):
    """uint64[n_labels + 1]: the reads assigned to each label, then the unassigned ones"""
    slot = assigned(classes, nks, min_found, min_permille, min_margin)
    slot[slot < 0] = n_labels
    return np.bincount(slot, minlength=n_labels + 1).astype(np.uint64)


def assert_classes(got, want, what=""):
    assert got.dtype == fa.READ_CLASS_DTYPE and got.shape == want.shape, what
    for f in ("label", "n_best", "n_second", "n_labelled"):
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, "%s: field %s differs in %d reads, first %d: got %s, want %s" % (what, f, len(bad), bad[0], got[bad[0]], want[bad[0]])


def run_labelling(rng, n_unitigs, n_labels=7, none_share=0.1):
    """about n_labels labels over contiguous runs of unitig numbers, none_share of the unitigs without one; every label is used"""
    cuts = np.sort(rng.choice(np.arange(1, n_unitigs), n_labels - 1, replace=False))
    lab = np.searchsorted(cuts, np.arange(n_unitigs), side="right").astype(np.uint32)
    lab[rng.random(n_unitigs) < none_share] = NONE
    assert len(np.unique(lab[lab != NONE])) == n_labels and (lab == NONE).any()
    return lab


def test_the_numpy_definition_on_small_reads():
    labels = [0, 1, 1, NONE, 2]
    tup = lambda a: [tuple(x) for x in a.tolist()]
    # a tie goes to the smaller label, whichever comes first in the read
    assert tup(classes_of([(4, 0), (4, 1), (0, 7), (0, 8)], [4], labels)) == [(0, 2, 2, 4)]
    assert tup(classes_of([(1, 0), (2, 1), (4, 7), (4, 8)], [4], labels)) == [(1, 2, 2, 4)]
    # two unitigs of one label vote together; an unlabelled unitig does not vote, but its slot is a found slot all the same (it is not an absent one)
    assert tup(classes_of([(1, 5), (2, 9), (3, 1), (3, 2), (3, 3), (-1, -1), (0, 0)], [7], labels)) == [(1, 2, 1, 3)]
    # the empty class: nothing found, nothing labelled, no k-mers
    assert tup(classes_of([(-1, -1)] * 3 + [(3, 1), (3, 2)], [3, 2, 0], labels)) == [(NONE, 0, 0, 0)] * 3
    # one label only: no second
    assert tup(classes_of([(4, 1), (-1, -1), (4, 3)], [3], labels)) == [(2, 2, 0, 2)]
    # reversing the slot order changes none of the four
    p = np.array([(-1, -1), (2, 9), (2, 8), (0, 7), (-1, -1), (4, 1), (4, 2), (3, 3), (-1, -1)])
    assert tup(classes_of(p, [9], labels)) == tup(classes_of(p[::-1], [9], labels)) == [(1, 2, 2, 5)]
    # the rule: ties pass a margin of 0 and fail a margin of 1; min_found 0 counts as 1; the share is of nk, not of the found slots
    c = classes_of([(4, 0), (4, 1), (0, 7), (0, 8)] + [(1, 1)] * 3 + [(-1, -1)] * 3 + [(-1, -1)] * 2, [4, 6, 2, 0], labels)
    assert tup(c) == [(0, 2, 2, 4), (1, 3, 0, 3), (NONE, 0, 0, 0), (NONE, 0, 0, 0)]
    assert assigned(c, [4, 6, 2, 0], 1, 0, 0).tolist() == [0, 1, -1, -1] and assigned(c, [4, 6, 2, 0], 0, 0, 0).tolist() == [0, 1, -1, -1]
    assert assigned(c, [4, 6, 2, 0], 1, 0, 1).tolist() == [-1, 1, -1, -1] and assigned(c, [4, 6, 2, 0], 3, 0, 0).tolist() == [-1, 1, -1, -1]
    assert assigned(c, [4, 6, 2, 0], 1, 500, 0).tolist() == [0, 1, -1, -1] and assigned(c, [4, 6, 2, 0], 1, 501, 0).tolist() == [-1, -1, -1, -1]
    assert tally_of(c, [4, 6, 2, 0], 3, 1, 0, 1).tolist() == [0, 1, 0, 3]


@pytest.mark.parametrize("k", [16, 31, 63])
def test_host_classes_of_hand_made_records(k):
    c = hand_made_case(k)
    rng = np.random.default_rng(1600 + k)
    kinds = c.recs["meta"] >> 16
    rev = (c.recs["meta"] >> 8) & 1
    for i, labels in enumerate((run_labelling(rng, len(c.unitigs)), np.arange(len(c.unitigs), dtype=np.uint32), np.full(len(c.unitigs), NONE, dtype=np.uint32))):
        want = classes_of(c.pairs, c.nks, labels)
        if i == 0:
            # conditions on the input: every kind, both strands (meta bit 8), and what the classes must show
            assert all((kinds == x).sum() > 100 for x in (0, 1, 2)) and ((kinds == 1) & (rev == 1)).sum() > 100
            one = want[kinds == 1]
            assert (one["label"] == NONE).any() and (one["label"] != NONE).any() and (one["n_second"] == 0).all()
            assert (want["n_labelled"][kinds == 2] == 0).all() and (want[kinds == 0]["n_second"] > 0).any()
            found = np.add.reduceat((c.pairs[:, 0] != -1).astype(np.int64), np.concatenate([[0], np.cumsum(c.nks)[:-1]]))
            assert ((want["n_labelled"] > 0) & (want["n_labelled"] < found)).any()
        got = fa.records_read_classes(c.recs, c.stream, k, labels)
        assert_classes(got, want, "k=%d" % k)
        one_thread, eight = fa.records_read_classes(c.recs, c.stream, k, labels, n_threads=1), fa.records_read_classes(c.recs, c.stream, k, labels, n_threads=8)
        assert one_thread.tobytes() == eight.tobytes() == got.tobytes()


def test_records_found_on_the_reverse_strand():
    """meta bit 8 reverses the slot order: the class does not change; with eight gaps, nine stretches"""
    k = 4
    labels = np.full(9, NONE, dtype=np.uint32); labels[7] = 3
    for rev in (0, 1):
        recs = np.zeros(2, dtype=fa.RECORD_DTYPE)
        Es = [10 + 12 * e for e in range(8)]
        recs["u"], recs["off0"], recs["nk"], recs["meta"] = (7, 8), 100, 120, 8 | (rev << 8) | (1 << 16)
        recs["Es"] = sum(E << (16 * e) for e, E in enumerate(Es[:4])); recs["Es2"] = sum(E << (16 * e) for e, E in enumerate(Es[4:]))
        none = np.zeros((0, 2), np.int32)
        got = fa.records_read_classes(recs, none, k, labels)
        assert_classes(got, classes_of(brute_expand(recs, none, k), recs["nk"], labels), "rev=%d" % rev)
        assert [tuple(x) for x in got.tolist()] == [(3, 120 - 8 * 4, 0, 120 - 8 * 4), (NONE, 0, 0, 0)]


def test_refusals():
    c = hand_made_case(31)
    labels = np.zeros(len(c.unitigs), dtype=np.uint32)
    for threads in (1, 8):
        for stream in (c.stream[:-1], np.concatenate([c.stream, c.stream[:3]])):   # a truncated stream, a stream with pairs to spare
            with pytest.raises(fa.FinitoError) as e:
                fa.records_read_classes(c.recs, stream, 31, labels, n_threads=threads)
            assert e.value.code == fa.FIN_EINVAL
        bad = np.array(c.stream); bad[len(bad) // 2] = (-2, 5)   # neither found nor (-1,-1)
        with pytest.raises(fa.FinitoError) as e:
            fa.records_read_classes(c.recs, bad, 31, labels, n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
        top = int(max(c.stream[:, 0].max(), c.recs["u"].max()))
        with pytest.raises(fa.FinitoError) as e:   # a unitig number the labelling does not reach: in the stream, in a record
            fa.records_read_classes(c.recs, c.stream, 31, labels[:top], n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
        fa.records_read_classes(c.recs, c.stream, 31, labels[:top + 1], n_threads=threads)
    assert len(fa.records_read_classes(np.zeros(0, fa.RECORD_DTYPE), np.zeros((0, 2), np.int32), 31, labels)) == 0   # nothing is legal


def test_null_and_bad_arguments_are_refused_before_any_device_call():
    L = fa.lib()
    err = C.create_string_buffer(512)
    h = C.c_void_p()
    assert L.fin_labels_create(None, 0, None, 1, C.byref(h), err, 512) == fa.FIN_EINVAL and b"null" in err.value
    assert L.fin_labels_download(None, None, None, err, 512) == fa.FIN_EINVAL and L.fin_labels_reset(None, None) == fa.FIN_EINVAL
    assert L.fin_labels_device_labels(None) is None and L.fin_labels_device_reads(None) is None and L.fin_batch_device_read_classes(None) is None
    L.fin_labels_free(None)
    assert L.fin_batch_classify(None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_batch_download_read_classes(None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_batch_add_classes(None, None, 1, 0, 0, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_search_batch_classify(None, None, None, 0, fa.FIN_MERGED, None, None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_search_batch_add_classes(None, None, None, 0, fa.FIN_MERGED, None, 1, 0, 0, err, 512) == fa.FIN_EINVAL
    assert L.fin_index_unitig_numbers(None, None, None, 0, None, err, 512) == fa.FIN_EINVAL
    out = (C.c_uint32 * 4)()
    assert L.fin_records_read_classes(None, 5, None, 0, 31, out, 1, out, 1) == fa.FIN_EINVAL
    assert L.fin_records_read_classes(None, 0, None, 0, 31, None, 0, None, 1) == fa.FIN_OK
    # what a labelling is checked for comes before the device is asked for: n_labels 0 or above 2^31, a label that is neither below n_labels nor FIN_NO_LABEL
    idx = fa.FinimizerIndex.build(["ACGGT", "CGGTA"], 4)
    for lab, n in (([0, 1], 0), ([0, 1], 0x80000001), ([0, 2], 2), ([5, NONE], 5)):
        with pytest.raises(fa.FinitoError) as e:
            idx.labels(np.array(lab, dtype=np.uint32), n)
        assert e.value.code == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:
        idx.labels(np.array([0], dtype=np.uint32))   # one label per unitig
    assert e.value.code == fa.FIN_EINVAL


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_classification_entry_points_fail_loudly_without_device():
    """No CPU fallback: without a HIP device the device entry points raise, they do not compute"""
    idx = fa.FinimizerIndex.build(["ACGGT", "CGGTA"], 4)
    with pytest.raises(fa.FinitoError) as e:
        idx.labels(np.array([0, 1], dtype=np.uint32))
    assert e.value.code == fa.FIN_ENODEV
    with pytest.raises(fa.FinitoError) as e:
        idx.unitig_numbers(["ACGGT"])
    assert e.value.code == fa.FIN_ENODEV


def test_cli_usage_rules(tmp_path):
    common = [BIN, "search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq")]
    lab = ["--label-unitigs", str(tmp_path / "u.fna"), "--labels", str(tmp_path / "l.txt")]
    r = subprocess.run([BIN, "search-fmin", "--help"], capture_output=True, text=True)
    assert all(x in r.stderr for x in ("--label-unitigs", "--labels", "--classify", "--label-report", "--class-min-found", "--class-min-permille", "--class-min-margin"))
    r = subprocess.run(common + ["--no-text", "1"], capture_output=True, text=True)
    assert r.returncode == 1 and "--classify" in r.stderr and "--label-report" in r.stderr and not r.stdout
    # with either flag --no-text 1 is legal: the run gets as far as the query file / index it cannot find
    for flag in ("--classify", "--label-report"):
        r = subprocess.run(common + lab + ["--no-text", "1", flag, str(tmp_path / "s.tsv")], capture_output=True, text=True)
        assert r.returncode == 1 and "--no-text" not in r.stderr
        r = subprocess.run(common + [flag, str(tmp_path / "s.tsv")], capture_output=True, text=True)   # no labelling
        assert r.returncode == 1 and "--label-unitigs" in r.stderr and "--labels" in r.stderr
    r = subprocess.run(common + lab, capture_output=True, text=True)   # a labelling nobody uses
    assert r.returncode == 1 and "--classify" in r.stderr
    r = subprocess.run(common + lab + ["--classify", str(tmp_path / "c.tsv"), "--class-min-margin", "1"], capture_output=True, text=True)
    assert r.returncode == 1 and "--label-report" in r.stderr
    r = subprocess.run(common + lab + ["--label-report", str(tmp_path / "p.txt"), "--class-min-permille", "1001"], capture_output=True, text=True)
    assert r.returncode == 1 and "--class-min-permille" in r.stderr and "1000" in r.stderr
    # --min-found stays the screen's
    r = subprocess.run(common + lab + ["--label-report", str(tmp_path / "p.txt"), "--min-found", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and "--screen" in r.stderr
