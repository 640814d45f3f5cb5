"""The coverage bitmap, the parts that need no GPU (include/finito_amd.h: fin_records_cover, fin_cover_*, fin_search_batch_unitig_coverage): the host-side
bitmap against np.unique over fin_expand_records' pairs, what it refuses, loud failure of the device entry points on a box without a device, and the
command's usage rules for --unitig-coverage and --no-text."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")
N_UNITIGS = 300


def made_up_ends(rng, k):
    """unitigs long enough for a record of 259 k-mers: lengths 260 + k .. 1500"""
    return np.cumsum(rng.integers(260 + k, 1500, N_UNITIGS)).astype(np.int64)


def random_record_set(rng, k, ends, n=3000):
    """the generator shape of tests/test_unitig_counts_host.py::random_record_set -- all three kinds, nk 0..259, 0..8 positions that may touch, overlap or lie
    beyond the last slot, both strand bits -- with places that exist: a kind-1 read lies inside its unitig, a kind-0 read's stream pairs are runs of ascending or
    descending offsets inside a unitig, absent slots between them"""
    starts = np.concatenate([[0], ends[:-1]])
    lens = ends - starts
    recs = np.zeros(n, dtype=fa.RECORD_DTYPE)
    stream = []
    for r in recs:
        nk = int(rng.integers(0, 260)); kind = int(rng.integers(0, 3))
        r["nk"] = nk
        if kind == 0:
            i = 0
            while i < nk:
                run = min(nk - i, int(rng.integers(1, 90)))
                if rng.random() < 0.25:
                    stream += [(-1, -1)] * run
                else:
                    u = int(rng.integers(0, N_UNITIGS)); a = int(rng.integers(0, lens[u] - k + 1 - run + 1))
                    offs = range(a, a + run) if rng.random() < 0.5 else range(a + run - 1, a - 1, -1)
                    stream += [(u, o) for o in offs]
                i += run
            continue
        nE = int(rng.integers(0, 9)) if kind == 1 else 0
        Es = sorted(int(x) for x in rng.integers(0, nk + k - 1, nE)) if nk else []
        nE = len(Es)
        u = int(rng.integers(0, N_UNITIGS))
        r["u"], r["off0"] = u, int(rng.integers(0, lens[u] - k + 1 - nk + 1))
        r["meta"] = nE | (int(rng.integers(0, 2)) << 8) | (kind << 16)
        r["Es"] = sum(E << (16 * e) for e, E in enumerate(Es[:4])); r["Es2"] = sum(E << (16 * e) for e, E in enumerate(Es[4:]))
    return recs, np.array(stream, dtype=np.int32).reshape(-1, 2)


def bits_of(pairs, ends):
    """the definition: np.unique over the found pairs, mapped through `ends` to bit positions"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    p = p[p[:, 0] >= 0]
    starts = np.concatenate([[0], np.asarray(ends, dtype=np.int64)[:-1]])
    g = np.unique(starts[p[:, 0]] + p[:, 1])
    flat = np.zeros(64 * ((int(ends[-1]) + 63) // 64), dtype=np.uint8)
    flat[g] = 1
    return np.packbits(flat, bitorder="little").view(np.uint64), len(g)


def test_host_bitmap_against_unique_of_the_expanded_pairs():
    rng = np.random.default_rng(18)
    for k in (4, 21, 31, 63):
        ends = made_up_ends(rng, k)
        recs, stream = random_record_set(rng, k, ends)
        pairs, npos = fa.expand_records(recs, stream, k)
        want, distinct = bits_of(pairs, ends)
        assert 0 < distinct < npos and (recs["meta"] >> 16 == 1).sum() > 500 and len(stream) > 10000
        for threads in (1, 3, 0):
            got = fa.records_cover(recs, stream, k, ends, n_threads=threads)
            assert got.dtype == np.uint64 and got.shape == want.shape
            assert np.array_equal(got, want), "k=%d threads=%d" % (k, threads)


def test_host_bitmap_on_nothing():
    got = fa.records_cover(np.zeros(0, dtype=fa.RECORD_DTYPE), np.zeros((0, 2), np.int32), 31, [100, 230])
    assert got.tolist() == [0] * 4


def test_host_bitmap_refuses_a_foreign_stream_and_places_outside_the_index():
    rng = np.random.default_rng(19)
    ends = made_up_ends(rng, 31)
    recs, stream = random_record_set(rng, 31, ends, n=2500)
    for threads in (1, 3):
        with pytest.raises(fa.FinitoError) as e:   # a truncated stream
            fa.records_cover(recs, stream[:-1], 31, ends, n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
        with pytest.raises(fa.FinitoError):        # a stream with pairs to spare
            fa.records_cover(recs, np.concatenate([stream, stream[:3]]), 31, ends, n_threads=threads)
        top_rec = int(recs["u"][(recs["meta"] >> 16 == 1) & (recs["nk"] > 0) & ((recs["meta"] & 0xFF) == 0)].max())
        with pytest.raises(fa.FinitoError):        # a record's unitig is not below n_unitigs
            fa.records_cover(recs, stream, 31, ends[:top_rec], n_threads=threads)
        only0 = recs[recs["meta"] >> 16 == 0]
        top = int(stream[:, 0].max())
        with pytest.raises(fa.FinitoError):        # a stream pair's unitig is not below n_unitigs
            fa.records_cover(only0, stream, 31, ends[:top], n_threads=threads)
        assert np.array_equal(fa.records_cover(only0, stream, 31, ends[:top + 1], n_threads=threads), bits_of(stream, ends[:top + 1])[0])
        # an offset beyond the unitig: a k-mer that would begin in the unitig's last k - 1 bases, from the stream and from a record
        bad = stream.copy()
        i = int(np.nonzero(bad[:, 0] >= 0)[0][5]); u = int(bad[i, 0])
        bad[i, 1] = int(ends[u] - (ends[u - 1] if u else 0)) - 31 + 1
        with pytest.raises(fa.FinitoError):
            fa.records_cover(only0, bad, 31, ends, n_threads=threads)
        one = np.zeros(1, dtype=fa.RECORD_DTYPE)
        one["u"], one["nk"], one["meta"] = 7, 100, 1 << 16
        length = int(ends[7] - ends[6])
        one["off0"] = length - 31 + 1 - 100
        assert fa.records_cover(one, np.zeros((0, 2), np.int32), 31, ends, n_threads=threads).view(np.uint8).sum() > 0
        one["off0"] += 1
        with pytest.raises(fa.FinitoError):
            fa.records_cover(one, np.zeros((0, 2), np.int32), 31, ends, n_threads=threads)


def test_null_arguments_are_refused_before_any_device_call():
    L = fa.lib()
    err = C.create_string_buffer(512)
    h = C.c_void_p()
    assert L.fin_cover_create(None, 0, C.byref(h), err, 512) == fa.FIN_EINVAL and not h.value
    assert L.fin_batch_add_cover(None, None, None, err, 512) == fa.FIN_EINVAL and b"null" in err.value
    assert L.fin_cover_download(None, None, None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_cover_reset(None, None) == fa.FIN_EINVAL
    assert L.fin_cover_device_bits(None) is None
    assert L.fin_search_batch_unitig_coverage(None, None, None, 0, fa.FIN_MERGED, None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_search_batch_add_cover(None, None, None, 0, fa.FIN_MERGED, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_records_cover(None, 5, None, 0, 31, None, 10, None, 1) == fa.FIN_EINVAL
    L.fin_cover_free(None)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_coverage_entry_points_fail_loudly_without_device():
    """No CPU fallback: without a HIP device the coverage's device entry points raise, they do not compute"""
    idx = fa.FinimizerIndex.build(["ACGGT", "CGGTA"], 4)
    with pytest.raises(fa.FinitoError) as e:
        idx.cover(0)
    assert e.value.code == -3
    with pytest.raises(fa.FinitoError) as e:
        idx.unitig_coverage(["ACGGTA"])
    assert e.value.code == -3
    with pytest.raises(fa.FinitoError) as e:
        idx.unitig_coverage([])
    assert e.value.code == -3


def test_cli_usage_rules(tmp_path):
    common = [BIN, "search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq")]
    r = subprocess.run(common + ["--no-text", "1"], capture_output=True, text=True)
    assert r.returncode == 1 and "--unitig-counts" in r.stderr and "--unitig-coverage" in r.stderr and not r.stdout
    # with --unitig-coverage, --no-text 1 is legal: the run gets as far as the index it cannot find
    r = subprocess.run(common + ["--no-text", "1", "--unitig-coverage", str(tmp_path / "c.tsv")], capture_output=True, text=True)
    assert r.returncode == 1 and "--no-text" not in r.stderr
    r = subprocess.run([BIN, "search-fmin", "--help"], capture_output=True, text=True)
    assert "--unitig-coverage" in r.stderr and "--unitig-counts" in r.stderr and "--no-text" in r.stderr
