"""Reference coordinates on the device (include/finito_amd.h: REFERENCE COORDINATES, fin_refpaths_*; fin_refpaths.hip).  The expectation is always
tests/test_refpaths_host.py's model -- plain Python from the header's definitions -- over the ORACLE's pairs segmented by tests/test_segments_host.py's model, or
over hand-made pairs; never a device result or a twin's.  The variants lifted are Pileup.call's (the lift's INPUT).  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.test_refpaths_host import assert_lift, assert_windows, model_lift, model_windows, window_offsets
from tests.test_records_device import inject
from tests.test_segments import nks_of, oracle_pairs
from tests.test_segments_host import assert_segments, segments_of
from tests.test_streams import Delay
from tests.test_unitig_counts import read_families
from tests.test_unitig_depth import Want
from tests.util import cut_unitigs, random_genome, rc, sample_reads

pytestmark = pytest.mark.gpu

WINDOWS = (1, 7, 64, 1000, 50000)   # the last one is larger than every sequence
TILES = (64, 0)
SENT = 0xA5A5A5A5A5A5A5A5


def substituted(rng, s, n):
    r = list(s)
    for p in rng.choice(len(s), n, replace=False):
        r[p] = "ACGT"[("ACGT".index(r[p]) + int(rng.integers(1, 4))) % 4]
    return "".join(r)


class World:
    def __init__(self, k):
        self.k = k
        rng = self.rng = np.random.default_rng(4100 + k)
        g = self.g = random_genome(rng, 40000)
        self.unitigs = cut_unitigs(rng, g, k, max_len=max(700, 4 * k))
        self.p = fa.FinimizerIndex.build(self.unitigs, k).to_device(0)
        self.o = OracleIndex.build(self.unitigs, k)
        self.ends = self.o.ends()
        assert np.array_equal(self.p.export(fa.X_ENDS), self.ends)
        copy = substituted(rng, g, 30)
        copy = copy[:20000] + random_genome(rng, 200) + copy[20200:]
        self.refs = [g, rc(g), copy, g[100:100 + k - 1], g[500:500 + k], random_genome(rng, 300)]
        self.seq_nk = nks_of(self.refs, k).astype(np.uint32)
        self.paths = segments_of(oracle_pairs(self.o, self.refs), self.seq_nk)
        # the sample: read families for the depth; reads of a copy with 60 planted substitutions for the pileup
        self.reads = read_families(rng, g, k, self.unitigs, n=400)
        self.depth = Want(oracle_pairs(self.o, self.reads), self.ends).depth.astype(np.uint32)
        planted = substituted(rng, g, 60)
        self.planted_reads = sample_reads(rng, planted, 3000, k + 120, err=0.0, random_frac=0.0)
        for a in (self.seq_nk, self.depth, *self.paths):
            a.setflags(write=False)

    def model_windows(self, window, md, times=1):
        return model_windows(self.seq_nk, *self.paths, self.ends, self.depth * np.uint32(times), window, md)

    def close(self):
        self.p.close()


@pytest.fixture(scope="module", params=[31, 127], ids=lambda k: "k%d" % k)
def w(request):
    world = World(request.param)
    yield world
    world.close()


def assert_paths(got, w, what=""):
    nk, so, sg = got
    assert nk.dtype == np.uint32 and np.array_equal(nk, w.seq_nk), what
    assert_segments((so, sg), w.paths, what)


def loaded(w):
    rp = w.p.ref_paths()
    b = w.p.batch(w.refs); b.run(fa.FIN_MERGED)
    rp.add(b)
    b.close()
    return rp


def test_the_expectation_shows_everything(w):
    so, sg = w.paths
    n = np.abs(sg["len"].astype(np.int64))
    assert (sg["len"] > 1).sum() >= 40 and (sg["len"] < 0).sum() >= 40, "fewer than 40 forward or 40 reverse segments"
    tiles = -(-n // 64)
    assert (tiles == 1).any() and (tiles == 2).any() and (tiles >= 3).any(), "a tile-count class at tile 64 is missing"
    assert so[4] == so[3] and w.seq_nk[3] == 0 and w.seq_nk[4] == 1 and so[5] == so[4] + 1 and so[6] == so[5], "k - 1 bases, k bases, nowhere"
    assert int(w.depth.max()) >= 3 and (w.depth == 0).any()


def test_paths_in_every_text_mode_and_by_every_route(w):
    p = w.p
    rp = p.ref_paths()
    assert (rp.n_seqs, rp.n_segments, rp.n_slots) == (0, 0, 0) and len(rp.download()[2]) == 0
    for mode in (0, 1, 2):
        b = p.batch(w.refs); b.text_mode(mode); b.run(fa.FIN_MERGED)
        rp.reset().add(b)
        assert_paths(rp.download(), w, "text mode %d" % mode)
        assert (rp.n_seqs, rp.n_segments, rp.n_slots) == (len(w.refs), len(w.paths[1]), int(w.seq_nk.sum()))
        b.close()
    # appended twice: the second copy's offsets go on where the first one's end
    b = p.batch(w.refs); b.run(fa.FIN_MERGED); b.segments(); rp.add(b); b.close()
    nk, so, sg = rp.download()
    n = len(w.paths[1])
    assert np.array_equal(nk, np.tile(w.seq_nk, 2)) and np.array_equal(so, np.concatenate([w.paths[0], w.paths[0][1:] + np.uint64(n)]))
    assert sg[:n].tobytes() == sg[n:].tobytes() == w.paths[1].tobytes()
    # host buffers, cut into sub-batches between sequences only
    p.set_option("pipeline_kmers", int(w.seq_nk.sum()) // 5); p.set_option("pipeline_depth", 3)
    try:
        assert_paths(rp.reset().add_reads(w.refs).download(), w, "host buffers, sub-batches")
    finally:
        p.set_option("pipeline_kmers", None); p.set_option("pipeline_depth", None)
    assert_paths(rp.reset().add_reads(w.refs).download(), w, "host buffers")
    assert rp.reset().add_reads([]).n_seqs == 0
    # upload: the model's paths in, the same bytes out
    assert_paths(rp.upload(w.seq_nk, *w.paths).download(), w, "upload")
    assert all(rp.device_ptrs())
    rp.close()


@pytest.mark.parametrize("route", ["add", "upload"])
def test_depth_windows_against_the_model(w, route):
    p = w.p
    rp = loaded(w) if route == "add" else p.ref_paths().upload(w.seq_nk, *w.paths)
    d = p.depth()
    b = p.batch(w.reads); b.text_mode(2); b.run(fa.FIN_MERGED)
    d.add(b)
    try:
        for tile in TILES:
            p.set_option("refpaths_tile", tile)
            for window in WINDOWS:
                for md in (1, 3):
                    assert_windows(rp.depth_windows(d, window, md), w.model_windows(window, md), "tile %d, window %d, min_depth %d" % (tile, window, md))
        d.add(b)
        p.set_option("refpaths_tile", 64)
        twice = rp.depth_windows(d, 7, 3)
        assert_windows(twice, w.model_windows(7, 3, times=2), "added twice")
        assert np.array_equal(twice.windows["depth_sum"], w.model_windows(7, 1)[1]["depth_sum"] * np.uint64(2))
        r = rp.depth_windows(d, 1000, 1)
        assert np.isnan(r.mean_depth[int(r.win_offs[5])]) and len(r.of(3)) == 0 and r.breadth[0] == r.windows["covered"][0] / r.windows["in_graph"][0]
        assert_paths(rp.download(), w, "the paths are not changed")
    finally:
        p.set_option("refpaths_tile", None)
        b.close(); d.close(); rp.close()


def test_lift_variants_against_the_model_over_the_pileups_candidates(w):
    p = w.p
    pl = p.pileup()
    pl.add_reads(w.planted_reads)
    v = pl.call(min_alt=2, min_permille=200)
    assert len(v) >= 20, "the planted substitutions were not called: %d candidates" % len(v)
    want = model_lift(w.seq_nk, *w.paths, w.ends, w.k, v)
    assert ((want["flags"] & 1) == 1).sum() >= 8 and ((want["flags"] & 1) == 0).sum() >= 8
    assert (np.bincount(want["var"].astype(np.int64), minlength=len(v)) >= 2).sum() >= 4
    for rp, what in ((loaded(w), "add"), (p.ref_paths().upload(w.seq_nk, *w.paths), "upload")):
        assert_lift(rp.lift_variants(v), want, what)
        assert len(rp.lift_variants(v[:0])) == 0
        one = rp.lift_variants(v[7:8])
        assert_lift(one, model_lift(w.seq_nk, *w.paths, w.ends, w.k, v[7:8]), what + ", one variant")
        ref, alt = fa.ref_variant_bases(want, v)
        fwd = (want["flags"] & 1) == 0
        assert np.array_equal(ref[fwd], v["ref"][want["var"][fwd]]) and np.array_equal(ref[~fwd], 3 - v["ref"][want["var"][~fwd]])
        # the lifted base IS the sequence's base wherever the sequence is the genome or its reverse complement
        for s in (0, 1):
            m = want["seq"] == s
            assert [w.refs[s][q] for q in want["pos"][m]] == ["ACGT"[c] for c in ref[m]], "sequence %d" % s
        rp.close()
    pl.close()


def test_one_segment_across_many_tiles_and_windows():
    """ONE unitig of 5 000 bases: a reference is a single segment that crosses many tiles and windows, forward and reverse"""
    k = 31
    rng = np.random.default_rng(77)
    u = random_genome(rng, 5000)
    p = fa.FinimizerIndex.build([u], k).to_device(0)
    o = OracleIndex.build([u], k)
    ends = o.ends()
    refs = [u, rc(u), u[1234:4000], rc(u[17:4999])]
    seq_nk = nks_of(refs, k).astype(np.uint32)
    paths = segments_of(oracle_pairs(o, refs), seq_nk)
    assert np.abs(paths[1]["len"]).tolist() == [4970, 4970, 2736, 4952] and (paths[1]["len"] < 0).sum() == 2
    reads = sample_reads(rng, u, 400, 150, err=0.01, random_frac=0.05)
    depth = Want(oracle_pairs(o, reads), ends).depth.astype(np.uint32)
    rp, d = p.ref_paths().add_reads(refs), p.depth().add_reads(reads)
    assert_segments(rp.download()[1:], paths, "one unitig")
    try:
        for tile in (64, 128, 0):
            p.set_option("refpaths_tile", tile)
            for window in WINDOWS:
                assert_windows(rp.depth_windows(d, window, 2), model_windows(seq_nk, *paths, ends, depth, window, 2), "tile %d, window %d" % (tile, window))
    finally:
        p.set_option("refpaths_tile", None)
    v = p.pileup().add_reads(sample_reads(rng, substituted(rng, u, 25), 1500, 150, err=0.0, random_frac=0.0)).call(2, 200)
    assert len(v) >= 10
    assert_lift(rp.lift_variants(v), model_lift(seq_nk, *paths, ends, k, v), "one unitig")
    rp.close(); d.close(); p.close()


def test_the_download_waits_for_an_add_behind_a_delay(w):
    b = w.p.batch(w.refs); b.run(fa.FIN_MERGED)
    b.segments()   # (the run's overflow verdict is known and the segments are made: the add below has nothing to wait for)
    rp = w.p.ref_paths().add(b)
    rp.reset().download()   # (room for the segments is there)
    delay, S = Delay(), torch.cuda.Stream()
    delay(S, 60.0)
    rp.add(b, stream=S.cuda_stream)
    assert S.query() is False, "the stream is idle where its delay should still run"
    assert_paths(rp.download(), w, "behind a delay")
    rp.close(); b.close()


def raw_depth(L, rp, d, window, md, n_wo, cap):
    """fin_refpaths_depth with sentinel-filled outputs for a path set of n_wo sequences and room for cap windows"""
    wo, out = np.full(n_wo + 2, SENT, dtype=np.uint64), np.full(2 * cap + 2, SENT, dtype=np.uint64)   # (win_offs has n_wo + 1 entries: one sentinel behind them)
    n, err = C.c_uint64(12345), C.create_string_buffer(512)
    rc_ = L.fin_refpaths_depth(rp.h, d.h if d is not None else None, window, md, wo.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), cap, C.byref(n), err, 512)
    return rc_, wo, out, int(n.value), err.value


def raw_lift(L, rp, v, cap):
    out = np.full(2 * cap + 2, SENT, dtype=np.uint64)
    n, err = C.c_uint64(12345), C.create_string_buffer(512)
    rc_ = L.fin_refpaths_lift_variants(rp.h, v.ctypes.data_as(C.c_void_p), len(v), out.ctypes.data_as(C.c_void_p), cap, C.byref(n), err, 512)
    return rc_, out, int(n.value), err.value


def test_refusals_leave_sentinel_filled_outputs_untouched(w):
    p, L = w.p, fa.lib()
    rp = loaded(w)
    d = p.depth().add_reads(w.reads)
    ns = len(w.refs)
    W = int(window_offsets(w.seq_nk, 7)[-1])
    untouched = lambda *a: all((x == SENT).all() for x in a)
    # a good call fills exactly its outputs
    rc_, wo, out, n, _ = raw_depth(L, rp, d, 7, 1, ns, W)
    want = w.model_windows(7, 1)
    assert rc_ == 0 and n == W and np.array_equal(wo[:-1], want[0]) and wo[-1] == SENT and out[:-2].tobytes() == want[1].tobytes() and untouched(out[-2:])
    # room for one window too few; window 0; a null depth; a depth of another index
    rc_, wo, out, n, msg = raw_depth(L, rp, d, 7, 1, ns, W - 1)
    assert rc_ == fa.FIN_ELIMIT and n == W and untouched(wo, out) and b"too small" in msg
    rc_, wo, out, n, msg = raw_depth(L, rp, d, 0, 1, ns, W)
    assert rc_ == fa.FIN_EINVAL and n == 0 and untouched(wo, out) and b"window" in msg
    rc_, wo, out, n, msg = raw_depth(L, rp, None, 7, 1, ns, W)
    assert rc_ == fa.FIN_EINVAL and untouched(wo, out)
    p2 = fa.FinimizerIndex.build(w.unitigs, w.k).to_device(0)
    d2 = p2.depth()
    rc_, wo, out, n, msg = raw_depth(L, rp, d2, 7, 1, ns, W)
    assert rc_ == fa.FIN_EINVAL and untouched(wo, out) and b"different indexes" in msg
    b2 = p2.batch(w.refs[3:]); b2.run(fa.FIN_MERGED)
    with pytest.raises(fa.FinitoError) as e:   # a batch of another index
        rp.add(b2)
    assert e.value.code == fa.FIN_EINVAL and "different indexes" in str(e.value)
    err = C.create_string_buffer(512)
    assert L.fin_search_batch_add_refpaths(p2.h, *fa._reads_args(w.refs[3:]), rp.h, err, 512) == fa.FIN_EINVAL and b"another index" in err.value
    b3 = p.batch(w.refs[3:])
    with pytest.raises(fa.FinitoError) as e:   # a batch that has not run
        rp.add(b3)
    assert e.value.code == fa.FIN_EINVAL
    assert_paths(rp.download(), w, "behind the refused adds")
    b2.close(); b3.close(); d2.close(); p2.close()
    # the lift: variants that do not ascend, variants outside the index, room for one record too few
    v = np.zeros(3, dtype=fa.VARIANT_DTYPE)
    v["u"], v["off"] = [0, 0, 1], [1, 5, 2]
    full = model_lift(w.seq_nk, *w.paths, w.ends, w.k, v)
    assert len(full) >= 3
    rc_, out, n, _ = raw_lift(L, rp, v, len(full))
    assert rc_ == 0 and n == len(full) and out[:-2].tobytes() == full.tobytes() and untouched(out[-2:])
    rc_, out, n, msg = raw_lift(L, rp, v, len(full) - 1)
    assert rc_ == fa.FIN_ELIMIT and n == len(full) and untouched(out)
    for what, edit in ((b"does not ascend", lambda x: x["off"].__setitem__(1, 1)), (b"outside the index", lambda x: x["u"].__setitem__(2, p.n_unitigs)),
                       (b"outside the index", lambda x: x["off"].__setitem__(2, int(w.ends[1] - w.ends[0])))):
        bad = v.copy(); edit(bad)
        rc_, out, n, msg = raw_lift(L, rp, bad, len(full))
        assert rc_ == fa.FIN_EINVAL and n == 0 and untouched(out) and what in msg, msg
    with pytest.raises(fa.FinitoError) as e:   # upload: the first bad segment by name, the object as it was
        bad = w.paths[1].copy(); bad["off"][5] = 1 << 20
        rp.upload(w.seq_nk, w.paths[0], bad)
    assert e.value.code == fa.FIN_EINVAL and "segment 5 " in str(e.value) and "offsets outside" in str(e.value)
    assert_paths(rp.download(), w, "behind the refused upload")
    rp.close(); d.close()


def test_hand_made_pairs_outside_the_index_are_caught_by_the_guard(w):
    """pairs that name no place of the index, put over a run's results (fin_batch_set_pairs): the segments made of them reach the object, the kernels' guard
    refuses them -- FIN_EINVAL "outside the index", nothing written -- and a reset makes the object usable again"""
    p, L, k = w.p, fa.lib(), w.k
    d = p.depth().add_reads(w.reads)
    v = p.pileup().add_reads(w.planted_reads).call(2, 200)
    nk0 = int(w.ends[0]) - k + 1
    reads = [w.g[1000:1000 + k + 9], w.g[3000:3000 + k + 9]]
    good = oracle_pairs(w.o, reads).astype(np.int32)
    cases = {"a unitig number at n_unitigs": (p.n_unitigs, 0, 1), "a forward run past nk(u)": (0, nk0 - 2, 1), "a reverse run from nk(u)": (0, nk0, -1),
             "a huge unitig number": (0x7FFFFFF0, 5, 1)}
    rp = p.ref_paths()
    W = int(window_offsets(nks_of(reads, k), 7)[-1])
    for name, (u, off, step) in cases.items():
        pairs = good.copy()
        pairs[10:15, 0] = u; pairs[10:15, 1] = off + step * np.arange(5)
        b = p.batch(reads); b.run(fa.FIN_MERGED); b.set_pairs(pairs)
        rp.reset().add(b)
        assert rp.n_seqs == 2
        rc_, wo, out, n, msg = raw_depth(L, rp, d, 7, 1, 2, W)
        assert rc_ == fa.FIN_EINVAL and b"outside the index" in msg and (wo == SENT).all() and (out == SENT).all(), name
        rc_, out, n, msg = raw_lift(L, rp, v, 64)
        assert rc_ == fa.FIN_EINVAL and b"outside the index" in msg and (out == SENT).all(), name
        b.close()
        if k <= 63:   # the same pairs under hand-made records (fin_batch_set_records): both reads marked as searched, in text modes 1 and 2
            for mode in (1, 2):
                b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
                assert b.run_info()["fast_path"]
                recs = np.zeros(2, dtype=fa.RECORD_DTYPE)
                recs["nk"] = nks_of(reads, k)
                inject(b, recs, pairs, mode)
                rp.reset().add(b)
                rc_, wo, out, n, msg = raw_depth(L, rp, d, 7, 1, 2, W)
                assert rc_ == fa.FIN_EINVAL and b"outside the index" in msg and (wo == SENT).all() and (out == SENT).all(), "%s, records, mode %d" % (name, mode)
                rc_, out, n, msg = raw_lift(L, rp, v, 64)
                assert rc_ == fa.FIN_EINVAL and b"outside the index" in msg and (out == SENT).all(), "%s, records, mode %d" % (name, mode)
                b.close()
    b = p.batch(w.refs); b.run(fa.FIN_MERGED)
    rp.reset().add(b)
    assert_windows(rp.depth_windows(d, 7, 1), w.model_windows(7, 1), "after the reset")
    b.close(); rp.close(); d.close()


def test_a_withheld_step_answers_with_the_depths_code():
    """tests/test_pileup_records.py's recipe: with the overflow list cut to three entries a step of genome reads overruns; added to the depth, the depth refuses with
    FIN_ELIMIT until its reset, and fin_refpaths_depth answers with that code and message; the paths themselves refuse such a run when it is offered"""
    k = 31
    rng = np.random.default_rng(11)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    reads = sample_reads(rng, g, 500, 150)
    L = fa.lib()
    rp, d = p.ref_paths().add_reads([g[:3000]]), p.depth()
    try:
        assert L.fin_set_option(b"lds_deque_limit", 1) == 0 and L.fin_set_option(b"seed_anchors", 0) == 0 and L.fin_set_option(b"debug_ovf_cap", 3) == 0
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        d.add(b)
        rc_, wo, out, n, msg = raw_depth(L, rp, d, 7, 1, 1, 1000)
        assert rc_ == fa.FIN_ELIMIT and b"overflow list" in msg and (wo == SENT).all() and (out == SENT).all()
        with pytest.raises(fa.FinitoError) as e:
            rp.add(b)
        assert e.value.code == fa.FIN_ELIMIT and rp.n_seqs == 1
        b.close()
        assert L.fin_set_option(b"debug_ovf_cap", 0) == 0
        assert int(rp.depth_windows(d.reset(), 1000, 1).windows["depth_sum"].sum()) == 0
    finally:
        L.fin_set_option(b"lds_deque_limit", 16); L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"debug_ovf_cap", 0)
        rp.close(); d.close(); p.close()
