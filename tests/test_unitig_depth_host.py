"""The per-position depth, the parts that need no GPU (include/finito_amd.h: fin_records_depth, fin_depth_*, fin_search_batch_unitig_depth): the host-side depth
against np.bincount over fin_expand_records' pairs, what it refuses, loud failure of the device entry points on a box without a device, and the command's usage
rules for --unitig-depth, --min-depth and --no-text."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from tests.test_unitig_coverage_host import made_up_ends, random_record_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def depth_of(pairs, ends):
    """the definition: np.bincount over the found pairs, mapped through `ends` to text positions"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    p = p[p[:, 0] >= 0]
    starts = np.concatenate([[0], np.asarray(ends, dtype=np.int64)[:-1]])
    return np.bincount(starts[p[:, 0]] + p[:, 1], minlength=int(ends[-1])).astype(np.uint32)


def test_stat_dtype_is_the_headers_struct():
    assert fa.DEPTH_STAT_DTYPE.itemsize == 16 and fa.DEPTH_STAT_DTYPE.names == ("sum", "max", "n_at_least")
    assert [fa.DEPTH_STAT_DTYPE.fields[n][1] for n in fa.DEPTH_STAT_DTYPE.names] == [0, 8, 12]


@pytest.mark.parametrize("k", [16, 31, 63])
def test_host_depth_against_bincount_of_the_expanded_pairs(k):
    rng = np.random.default_rng(180 + k)
    ends = made_up_ends(rng, k)
    recs, stream = random_record_set(rng, k, ends, n=6000)
    pairs, npos = fa.expand_records(recs, stream, k)
    want = depth_of(pairs, ends)
    assert int(want.sum()) == npos and want.max() >= 3 and (want == 0).any() and (recs["meta"] >> 16 == 1).sum() > 500 and len(stream) > 10000
    for threads in (1, 3, 0):
        got = fa.records_depth(recs, stream, k, ends, n_threads=threads)
        assert got.dtype == np.uint32 and got.shape == want.shape
        assert np.array_equal(got, want), "k=%d threads=%d" % (k, threads)
    # twice the record set is twice the depth: nothing saturates, nothing is idempotent
    twice = fa.records_depth(np.concatenate([recs, recs]), np.concatenate([stream, stream]), k, ends)
    assert np.array_equal(twice, 2 * want)


def test_host_depth_on_nothing():
    got = fa.records_depth(np.zeros(0, dtype=fa.RECORD_DTYPE), np.zeros((0, 2), np.int32), 31, [100, 230])
    assert got.dtype == np.uint32 and got.shape == (230,) and not got.any()


def test_host_depth_refuses_a_foreign_stream_and_places_outside_the_index():
    rng = np.random.default_rng(19)
    ends = made_up_ends(rng, 31)
    recs, stream = random_record_set(rng, 31, ends, n=2500)
    for threads in (1, 3):
        with pytest.raises(fa.FinitoError) as e:   # a truncated stream
            fa.records_depth(recs, stream[:-1], 31, ends, n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
        with pytest.raises(fa.FinitoError):        # a stream with pairs to spare
            fa.records_depth(recs, np.concatenate([stream, stream[:3]]), 31, ends, n_threads=threads)
        top_rec = int(recs["u"][(recs["meta"] >> 16 == 1) & (recs["nk"] > 0) & ((recs["meta"] & 0xFF) == 0)].max())
        with pytest.raises(fa.FinitoError):        # a record's unitig is not below n_unitigs
            fa.records_depth(recs, stream, 31, ends[:top_rec], n_threads=threads)
        only0 = recs[recs["meta"] >> 16 == 0]
        top = int(stream[:, 0].max())
        with pytest.raises(fa.FinitoError):        # a stream pair's unitig is not below n_unitigs
            fa.records_depth(only0, stream, 31, ends[:top], n_threads=threads)
        assert np.array_equal(fa.records_depth(only0, stream, 31, ends[:top + 1], n_threads=threads), depth_of(stream, ends[:top + 1]))
        # a k-mer that leaves its own unitig: one that would begin in the unitig's last k - 1 bases, from the stream and from a record
        bad = stream.copy()
        i = int(np.nonzero(bad[:, 0] >= 0)[0][5]); u = int(bad[i, 0])
        bad[i, 1] = int(ends[u] - (ends[u - 1] if u else 0)) - 31 + 1
        with pytest.raises(fa.FinitoError):
            fa.records_depth(only0, bad, 31, ends, n_threads=threads)
        one = np.zeros(1, dtype=fa.RECORD_DTYPE)
        one["u"], one["nk"], one["meta"] = 7, 100, 1 << 16
        length = int(ends[7] - ends[6])
        one["off0"] = length - 31 + 1 - 100
        got = fa.records_depth(one, np.zeros((0, 2), np.int32), 31, ends, n_threads=threads)
        assert int(got.sum()) == 100 and got.max() == 1 and not got[ends[7] - 30:ends[7]].any() and got[ends[7] - 31] == 1
        one["off0"] += 1
        with pytest.raises(fa.FinitoError):
            fa.records_depth(one, np.zeros((0, 2), np.int32), 31, ends, n_threads=threads)
    with pytest.raises(fa.FinitoError):            # ends that descend
        fa.records_depth(np.zeros(0, dtype=fa.RECORD_DTYPE), np.zeros((0, 2), np.int32), 31, [100, 50])


def test_null_arguments_are_refused_before_any_device_call():
    L = fa.lib()
    err = C.create_string_buffer(512)
    h = C.c_void_p()
    assert L.fin_depth_create(None, 0, C.byref(h), err, 512) == fa.FIN_EINVAL and not h.value
    assert L.fin_batch_add_depth(None, None, None, err, 512) == fa.FIN_EINVAL and b"null" in err.value
    assert L.fin_depth_download(None, 1, None, None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_depth_reset(None, None) == fa.FIN_EINVAL
    assert L.fin_depth_device_diff(None) is None
    assert L.fin_search_batch_unitig_depth(None, None, None, 0, fa.FIN_MERGED, 1, None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_search_batch_add_depth(None, None, None, 0, fa.FIN_MERGED, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_records_depth(None, 5, None, 0, 31, None, 10, None, 1) == fa.FIN_EINVAL
    assert L.fin_set_option(b"debug_depth_tile", 4097) != 0 and L.fin_set_option(b"debug_depth_tile", 257) == 0 and L.fin_set_option(b"debug_depth_tile", 0) == 0
    L.fin_depth_free(None)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_depth_entry_points_fail_loudly_without_device():
    """No CPU fallback: without a HIP device the depth's device entry points raise, they do not compute"""
    idx = fa.FinimizerIndex.build(["ACGGT", "CGGTA"], 4)
    with pytest.raises(fa.FinitoError) as e:
        idx.depth(0)
    assert e.value.code == -3
    with pytest.raises(fa.FinitoError) as e:
        idx.unitig_depth(["ACGGTA"])
    assert e.value.code == -3
    with pytest.raises(fa.FinitoError) as e:
        idx.unitig_depth([], min_depth=3)
    assert e.value.code == -3


def test_cli_usage_rules(tmp_path):
    common = [BIN, "search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq")]
    r = subprocess.run(common + ["--no-text", "1"], capture_output=True, text=True)
    assert r.returncode == 1 and "--unitig-depth" in r.stderr and "--unitig-counts" in r.stderr and not r.stdout
    # --min-depth without --unitig-depth is a usage error, with or without another product
    r = subprocess.run(common + ["--min-depth", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and "--min-depth" in r.stderr and "--unitig-depth" in r.stderr and not r.stdout
    r = subprocess.run(common + ["--min-depth", "3", "--unitig-coverage", str(tmp_path / "c.tsv")], capture_output=True, text=True)
    assert r.returncode == 1 and "--min-depth" in r.stderr and not r.stdout
    for bad in ("-1", "x", "4294967296", "3x"):
        r = subprocess.run(common + ["--min-depth", bad, "--unitig-depth", str(tmp_path / "d.tsv")], capture_output=True, text=True)
        assert r.returncode == 1 and "--min-depth" in r.stderr, bad
    # with --unitig-depth, --no-text 1 and --min-depth are legal: the run gets as far as the index it cannot find
    r = subprocess.run(common + ["--no-text", "1", "--unitig-depth", str(tmp_path / "d.tsv"), "--min-depth", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and "--no-text" not in r.stderr and "--min-depth" not in r.stderr
    r = subprocess.run([BIN, "search-fmin", "--help"], capture_output=True, text=True)
    assert "--unitig-depth" in r.stderr and "--min-depth" in r.stderr and "--no-text" in r.stderr
