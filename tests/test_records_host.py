"""Hand-made records, the parts that need no GPU (tests/util.py::hand_made_records; include/finito_amd.h: fin_batch_set_records): the conditions the generator
must meet for tests/test_records_device.py to mean anything, asserted on the records and on tests/test_records.py::brute_expand alone; the host functions over
the very record set the device consumers are given, against the same numpy references; and the refusal of null arguments before any device call."""
import ctypes as C

import numpy as np
import pytest

import finito_amd as fa
from tests.test_segments_host import assert_segments, segments_of
from tests.test_unitig_counts import profile_of
from tests.test_unitig_coverage_host import bits_of
from tests.test_unitig_depth import Want as DepthWant
from tests.util import UNIFORM_BLOCKS, hand_made_case


def positions_of(rec):
    return [(int(rec["Es"] if e < 4 else rec["Es2"]) >> (16 * (e & 3))) & 0xFFFF for e in range(int(rec["meta"]) & 0xFF)]


def assert_generator_conditions(case):
    """what the record set must hold (counted on the records and on brute_expand's pairs, never on anything the library computes)"""
    recs, k, pairs = case.recs, case.k, case.pairs
    kind, nE, rev, nks = recs["meta"] >> 16, recs["meta"] & 0xFF, (recs["meta"] >> 8) & 1, recs["nk"].astype(np.int64)
    one = kind == 1
    for e in range(9):
        for s in (0, 1):
            assert (one & (nE == e) & (rev == s)).sum() >= 100, "kind-1 records with %d positions on strand %d" % (e, s)
    at = np.concatenate([[0], np.cumsum(nks)])
    starts = np.concatenate([[0], case.ends[:-1]])
    overlap = clamp0 = clamp_end = nothing = whole_long = cross1 = cross2 = 0
    for r in np.nonzero(one)[0]:
        E, nk = positions_of(recs[r]), int(nks[r])
        overlap += any(max(b - k + 1, 0) <= min(a, nk - 1) for a, b in zip(E, E[1:]))   # two neighbouring gaps share a slot
        clamp0 += any(x < k - 1 for x in E)
        clamp_end += any(x >= nk for x in E)
        whole_long += (not E) and nk >= 200
        p = pairs[at[r]:at[r + 1]].astype(np.int64)
        p = p[p[:, 0] >= 0]
        nothing += len(p) == 0
        if len(p):   # the found stretches as text positions, and how many 64-position word boundaries each crosses
            g = np.sort(starts[p[:, 0]] + p[:, 1])
            cut = np.nonzero(np.diff(g) != 1)[0]
            first, last = g[np.concatenate([[0], cut + 1])], g[np.concatenate([cut, [len(g) - 1]])]
            words = (last >> 6) - (first >> 6)
            cross1 += bool((words >= 1).any()); cross2 += bool((words >= 2).any())
    assert overlap >= 50 and clamp0 >= 50 and clamp_end >= 50 and nothing >= 20 and whole_long >= 20 and cross1 >= 50 and cross2 >= 50, \
        (overlap, clamp0, clamp_end, nothing, whole_long, cross1, cross2)
    uniform = {256 * blk + w: kd for blk, kd in UNIFORM_BLOCKS for w in range(0, 256, 64)}
    for w in range(0, len(recs), 64):
        seen = set(int(x) for x in kind[w:w + 64])
        assert seen == ({uniform[w]} if w in uniform else {0, 1, 2}), "wave at read %d holds kinds %s" % (w, seen)
    blk1 = [blk for blk, kd in UNIFORM_BLOCKS if kd == 1][0]
    assert len(set(recs["u"][256 * blk1:256 * blk1 + 256].tolist())) == 1, "the kind-1 block lies on one unitig"
    # places: inside their unitig, some at its first k-mer, some with the last slot on its last
    kmers = np.diff(np.concatenate([[0], case.ends])) - k + 1
    room = kmers[recs["u"][one]] - nks[one] - recs["off0"][one]
    assert (room >= 0).all() and (room == 0).sum() >= 50 and (recs["off0"][one] == 0).sum() >= 50
    # the searched reads' pairs: both directions, absent slots, repeats
    s = case.stream.astype(np.int64)
    same = (s[1:, 0] == s[:-1, 0]) & (s[1:, 0] >= 0)
    d = s[1:, 1] - s[:-1, 1]
    assert (same & (d == 1)).sum() > 1000 and (same & (d == -1)).sum() > 1000 and (same & (d == 0)).sum() > 100 and (s[:, 0] == -1).sum() > 1000


@pytest.mark.parametrize("k", [16, 31, 63])
def test_the_generator_meets_its_conditions(k):
    assert_generator_conditions(hand_made_case(k))


@pytest.mark.parametrize("k", [16, 31, 63])
def test_host_functions_on_the_hand_made_records(k):
    """expand_records, records_unitig_counts, records_cover, records_depth and records_segments over the record set the device consumers are given"""
    c = hand_made_case(k)
    n_unitigs = len(c.ends)
    for threads in (1, 3):
        got, npos = fa.expand_records(c.recs, c.stream, k, n_threads=threads)
        assert np.array_equal(got, c.pairs) and npos == int((c.pairs[:, 0] != -1).sum())
        assert np.array_equal(fa.records_unitig_counts(c.recs, c.stream, k, n_unitigs, n_threads=threads), profile_of(c.pairs, n_unitigs))
        assert np.array_equal(fa.records_cover(c.recs, c.stream, k, c.ends, n_threads=threads), bits_of(c.pairs, c.ends)[0])
        assert np.array_equal(fa.records_depth(c.recs, c.stream, k, c.ends, n_threads=threads).astype(np.int64), DepthWant(c.pairs, c.ends).depth)
        assert_segments(fa.records_segments(c.recs, c.stream, k, n_threads=threads), segments_of(c.pairs, c.nks), "k=%d threads=%d" % (k, threads))


def test_null_arguments_are_refused_before_any_device_call():
    L = fa.lib()
    err = C.create_string_buffer(512)
    recs = np.zeros(4, dtype=fa.RECORD_DTYPE)
    assert L.fin_batch_set_records(None, None, None, err, 512) == fa.FIN_EINVAL and b"null" in err.value
    err = C.create_string_buffer(512)
    assert L.fin_batch_set_records(None, recs.ctypes.data_as(C.c_void_p), None, err, 512) == fa.FIN_EINVAL and b"null" in err.value
    assert L.fin_batch_set_records(None, None, None, None, 0) == fa.FIN_EINVAL   # no room for a message either
