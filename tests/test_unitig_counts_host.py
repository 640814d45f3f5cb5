"""The per-unitig profile, the parts that need no GPU (include/finito_amd.h: fin_records_unitig_counts, fin_hits_*, fin_search_batch_unitig_counts):
the host-side counter against np.bincount over fin_expand_records' pairs, what it refuses, loud failure of the device entry points on a box
without a device, and the command's usage rule for --no-text."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")
N_UNITIGS = 1000


def random_record_set(rng, k, n=3000):
    """as tests/test_records.py::test_expander_against_the_records_meaning builds them: all three kinds, nk 0..259, 0..8 positions that may
    touch, overlap or lie beyond the last slot, both strand bits"""
    recs = np.zeros(n, dtype=fa.RECORD_DTYPE)
    stream = []
    for r in recs:
        nk = int(rng.integers(0, 260)); kind = int(rng.integers(0, 3))
        r["nk"] = nk
        if kind == 0:
            # (runs of one unitig, absent slots between them: what a searched read looks like)
            u = int(rng.integers(-1, 50))
            for _ in range(nk):
                if rng.random() < 0.2:
                    u = int(rng.integers(-1, 50))
                stream.append((u, u))
            continue
        nE = int(rng.integers(0, 9)) if kind == 1 else 0
        Es = sorted(int(x) for x in rng.integers(0, nk + k - 1, nE)) if nk else []
        nE = len(Es)
        r["u"], r["off0"], r["meta"] = int(rng.integers(0, N_UNITIGS)), int(rng.integers(0, 5000)), nE | (int(rng.integers(0, 2)) << 8) | (kind << 16)
        r["Es"] = sum(E << (16 * e) for e, E in enumerate(Es[:4])); r["Es2"] = sum(E << (16 * e) for e, E in enumerate(Es[4:]))
    return recs, np.array(stream, dtype=np.int32).reshape(-1, 2)


def test_host_counter_against_bincount_of_the_expanded_pairs():
    rng = np.random.default_rng(8)
    for k in (4, 21, 31, 63):
        recs, stream = random_record_set(rng, k)
        pairs, npos = fa.expand_records(recs, stream, k)
        u = pairs[:, 0].astype(np.int64)
        want = np.bincount(u[u >= 0], minlength=N_UNITIGS).astype(np.uint64)
        assert int(want.sum()) == npos and (recs["meta"] >> 16 == 1).sum() > 500 and len(stream) > 10000
        for threads in (1, 3, 0):
            got = fa.records_unitig_counts(recs, stream, k, N_UNITIGS, n_threads=threads)
            assert got.dtype == np.uint64 and got.shape == (N_UNITIGS,)
            assert np.array_equal(got, want), "k=%d threads=%d" % (k, threads)


def test_host_counter_on_nothing():
    got = fa.records_unitig_counts(np.zeros(0, dtype=fa.RECORD_DTYPE), np.zeros((0, 2), np.int32), 31, 7)
    assert got.tolist() == [0] * 7


def test_host_counter_refuses_a_foreign_stream_and_a_unitig_outside_the_index():
    rng = np.random.default_rng(9)
    recs, stream = random_record_set(rng, 31, n=2500)
    for threads in (1, 3):
        with pytest.raises(fa.FinitoError) as e:   # a truncated stream
            fa.records_unitig_counts(recs, stream[:-1], 31, N_UNITIGS, n_threads=threads)
        assert e.value.code == fa.FIN_EINVAL
        with pytest.raises(fa.FinitoError):        # a stream with pairs to spare
            fa.records_unitig_counts(recs, np.concatenate([stream, stream[:3]]), 31, N_UNITIGS, n_threads=threads)
        top_rec = int(recs["u"][(recs["meta"] >> 16 == 1) & (recs["nk"] > 0) & ((recs["meta"] & 0xFF) == 0)].max())
        with pytest.raises(fa.FinitoError):        # a record's unitig is not below n_unitigs
            fa.records_unitig_counts(recs, stream, 31, top_rec, n_threads=threads)
        only0 = recs[recs["meta"] >> 16 == 0]
        with pytest.raises(fa.FinitoError):        # a stream pair's unitig is not below n_unitigs
            fa.records_unitig_counts(only0, stream, 31, int(stream[:, 0].max()), n_threads=threads)
        assert fa.records_unitig_counts(only0, stream, 31, int(stream[:, 0].max()) + 1, n_threads=threads).sum() == (stream[:, 0] >= 0).sum()


def test_null_arguments_are_refused_before_any_device_call():
    L = fa.lib()
    err = C.create_string_buffer(512)
    h = C.c_void_p()
    assert L.fin_hits_create(None, 0, C.byref(h), err, 512) == fa.FIN_EINVAL and not h.value
    assert L.fin_batch_add_hits(None, None, None, err, 512) == fa.FIN_EINVAL and b"null" in err.value
    assert L.fin_hits_download(None, None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_hits_reset(None, None) == fa.FIN_EINVAL
    assert L.fin_hits_device_counts(None) is None
    assert L.fin_search_batch_unitig_counts(None, None, None, 0, fa.FIN_MERGED, None, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_search_batch_add_hits(None, None, None, 0, fa.FIN_MERGED, None, err, 512) == fa.FIN_EINVAL
    assert L.fin_records_unitig_counts(None, 5, None, 0, 31, 10, None, 1) == fa.FIN_EINVAL
    L.fin_hits_free(None)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_profile_entry_points_fail_loudly_without_device():
    """No CPU fallback: without a HIP device the profile's device entry points raise, they do not compute"""
    idx = fa.FinimizerIndex.build(["ACGGT", "CGGTA"], 4)
    with pytest.raises(fa.FinitoError) as e:
        idx.hits(0)
    assert e.value.code == -3
    with pytest.raises(fa.FinitoError) as e:
        idx.unitig_counts(["ACGGTA"])
    assert e.value.code == -3
    with pytest.raises(fa.FinitoError) as e:
        idx.unitig_counts([])
    assert e.value.code == -3


def test_cli_no_text_needs_unitig_counts(tmp_path):
    r = subprocess.run([BIN, "search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq"), "--no-text", "1"], capture_output=True, text=True)
    assert r.returncode == 1 and "--unitig-counts" in r.stderr and not r.stdout
    r = subprocess.run([BIN, "search-fmin", "--help"], capture_output=True, text=True)
    assert "--unitig-counts" in r.stderr and "--no-text" in r.stderr
