"""Reads assigned to references on the device (include/finito_amd.h: fin_assign_rows, fin_batch_assign, fin_batch_assign_bin, fin_search_batch_assign; DESIGN.md
4.21) against the host twin fin_rows_assign and the numpy model of tests/test_assign_host.py.  All expectations are exact: rows, heads, assigned, sole and
counters are compared byte for byte.  Option "assign_rpb" is 64 in the row cases, so several blocks flush into the same colours and the last block is partial.
The bins (fin_assign_column_kernel) are held to np.flatnonzero over the unpacked column of the rows Batch.assign returns: at 130 colours (W = 3) for colours in
every word and at bit 63, at 1 .. 1000 reads, and once past 262 144 reads, where the scan of the blocks' counts leaves its first level."""
import numpy as np
import pytest
import torch

import finito_amd as fa
from tests.test_assign_host import (N_COLORS, assert_identities, assert_same, dyadic_weights, model, random_rows, random_weights, unpack_bool)
from tests.test_colors_host import pack_members, words_of
from tests.test_eqclasses import on_device, small   # noqa: F401 (the fixture: the suite's small index)
from tests.test_streams import Delay
from tests.util import cut_unitigs, random_genome, sample_reads

pytestmark = pytest.mark.gpu
N_ROWS = [0, 1, 63, 64, 65, 257, 3000]


def device_assign(asg, rows, want_rows=True, want_heads=True, stream=None):
    """rows through Assign.add_rows: (assigned rows or None, heads or None)"""
    n, W = len(rows), asg.words
    t = on_device(rows) if n else None
    out = torch.zeros((max(n, 1), W), dtype=torch.int64, device="cuda") if want_rows else None
    heads = torch.zeros((max(n, 1), 2), dtype=torch.int32, device="cuda") if want_heads else None
    torch.cuda.synchronize()
    asg.add_rows(t.data_ptr() if n else 0, n, out.data_ptr() if want_rows else 0, heads.data_ptr() if want_heads else 0, stream=stream)
    asg.download()   # waits
    torch.cuda.synchronize()
    r = out.cpu().numpy().view(np.uint64)[:n] if want_rows else None
    h = np.ascontiguousarray(heads.cpu().numpy()).view(fa.READ_ASSIGN_DTYPE).reshape(-1)[:n] if want_heads else None
    return r, h


@pytest.mark.parametrize("n_colors", N_COLORS)
def test_rows_against_twin_and_model(small, n_colors):
    p, g, _ = small
    rng = np.random.default_rng(3600 + n_colors)
    col = p.colors(n_colors)
    p.set_option("assign_rpb", 64)
    try:
        for family, weights, fold in (("dyadic", dyadic_weights, False), ("random", random_weights, True)):
            x = weights(rng, n_colors)
            thr = rng.integers(0, 9, n_colors) / 8.0 if family == "dyadic" else rng.uniform(0, 1, n_colors)
            asg = col.assigner(x, thr)
            for n in N_ROWS:
                what = "%s weights, %d colours, %d rows" % (family, n_colors, n)
                rows = random_rows(rng, n, n_colors, max_set=8 if family == "dyadic" else min(n_colors, 40))
                asg.reset()
                r, h = device_assign(asg, rows)
                got = (r, h) + asg.download()
                twin = fa.rows_assign(rows, n_colors, x, thr)
                assert_same(got, twin, what + ": against the host twin")
                assert_same(got, model(rows, n_colors, x, thr, fold), what + ": against the model")
                assert_identities(rows, got, what)
            asg.close()
    finally:
        p.set_option("assign_rpb", None)
    col.close()


@pytest.mark.parametrize("n_colors", [5, 130])
def test_default_blocks_two_adds_reset_set_and_null_outputs(small, n_colors):
    p, g, _ = small
    rng = np.random.default_rng(3700 + n_colors)
    col = p.colors(n_colors)
    x, x2 = random_weights(rng, n_colors), dyadic_weights(rng, n_colors)
    asg = col.assigner(x)               # thresholds 0.5
    a, b = random_rows(rng, 3000, n_colors), random_rows(rng, 257, n_colors)
    ta, tb = fa.rows_assign(a, n_colors, x, 0.5), fa.rows_assign(b, n_colors, x, 0.5)
    r, h = device_assign(asg, a)        # the automatic rows per block
    assert_same((r, h) + asg.download(), ta, "default blocks")
    r, h = device_assign(asg, b, want_rows=False)   # two adds accumulate; no assigned rows wanted
    assert r is None and h.tobytes() == tb[1].tobytes()
    for got, u, v in zip(asg.download(), ta[2:], tb[2:]):
        assert got.tobytes() == (u + v).tobytes(), "two adds"
    asg.reset()
    r, h = device_assign(asg, b, want_heads=False)  # no heads wanted
    assert h is None and r.tobytes() == tb[0].tobytes()
    assert_same(asg.download(), tb[2:], "after a reset")
    r, h = device_assign(asg, b, want_rows=False, want_heads=False)   # counts alone
    assert [int(v) for v in asg.download()[2]] == [2 * int(v) for v in tb[4]]
    # set: new weights and thresholds for the adds behind it, the counts stay; reset behind it leaves the weights
    asg.set(x2, 0.25)
    t2 = fa.rows_assign(a, n_colors, x2, 0.25)
    r, h = device_assign(asg, a)
    assert r.tobytes() == t2[0].tobytes() and h.tobytes() == t2[1].tobytes()
    assert asg.download()[0].tobytes() == (2 * tb[2] + t2[2]).tobytes()
    asg.reset()
    r, h = device_assign(asg, a)
    assert_same((r, h) + asg.download(), t2, "set, then reset")
    for call, word in ((lambda: asg.set(-x2, 0.5), "weight of colour 0"), (lambda: col.assigner(x, 1.5), "threshold of colour 0")):
        with pytest.raises(fa.FinitoError) as e:
            call()
        assert e.value.code == fa.FIN_EINVAL and word in str(e.value)
    import ctypes as C
    f64p = C.POINTER(C.c_double)
    bad, half, err, h_out = x.copy(), np.full(n_colors, 0.5), C.create_string_buffer(512), C.c_void_p()
    bad[n_colors - 1] = np.nan             # the C entry points by themselves refuse, and name the colour
    assert asg.L.fin_assign_create(col.h, bad.ctypes.data_as(f64p), half.ctypes.data_as(f64p), C.byref(h_out), err, 512) == fa.FIN_EINVAL
    assert ("the weight of colour %d" % (n_colors - 1)) in err.value.decode() and not h_out.value
    half[2] = 1.25
    assert asg.L.fin_assign_set(asg.h, x.ctypes.data_as(f64p), half.ctypes.data_as(f64p), None, err, 512) == fa.FIN_EINVAL
    assert "the threshold of colour 2" in err.value.decode()
    asg.close(); col.close()


def test_stray_bits_are_masked_on_the_device(small):
    p, g, _ = small
    n_colors = 70
    rng = np.random.default_rng(3750)
    col = p.colors(n_colors)
    x = random_weights(rng, n_colors)
    rows = random_rows(rng, 200, n_colors)
    dirty = rows.copy()
    dirty[:, 1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(6)
    asg = col.assigner(x, 0.1)
    r, h = device_assign(asg, dirty)
    assert_same((r, h) + asg.download(), fa.rows_assign(rows, n_colors, x, 0.1), "stray bits")
    asg.close(); col.close()


def test_download_waits_for_an_add_behind_a_delay(small):
    """tests/test_streams.py's download case: the add sits behind a delay on a non-blocking stream when the download is issued, and the result includes it"""
    p, g, _ = small
    n_colors = 70
    rng = np.random.default_rng(3800)
    col = p.colors(n_colors)
    x = random_weights(rng, n_colors)
    asg = col.assigner(x, 0.2)
    rows = random_rows(rng, 500, n_colors)
    t = on_device(rows)
    out = torch.zeros((500, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    delay, S = Delay(), torch.cuda.Stream()
    delay(S, 60.0)
    asg.add_rows(t.data_ptr(), 500, out.data_ptr(), 0, stream=S.cuda_stream)
    assert S.query() is False, "the stream is idle where its delay should still run"
    got = asg.download()
    twin = fa.rows_assign(rows, n_colors, x, 0.2)
    assert_same(got, twin[2:], "behind a delay")
    assert out.cpu().numpy().view(np.uint64).tobytes() == twin[0].tobytes()
    del t, out
    asg.close(); col.close()


# ---- end to end: three references ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three():
    k = 31
    rng = np.random.default_rng(3900)
    shared, priv = random_genome(rng, 6000), [random_genome(rng, 3000) for _ in range(3)]
    unitigs = []
    for piece in [shared] + priv:
        unitigs += cut_unitigs(rng, piece, k, max_len=300)
    refs = [shared + x for x in priv]
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    col = p.colors(3)
    for c in range(3):
        col.add_reads([shared, priv[c]], c)
    reads = []
    for ref, n in zip(refs, (700, 200, 100)):
        reads += sample_reads(rng, ref, n, 100, err=0.0, random_frac=0.05)
    reads = [reads[i] for i in rng.permutation(len(reads))]
    assert len(reads) % 2 == 0
    eq = col.eqclasses(64)
    ab = eq.add_reads(reads).abundance(np.array([len(r) for r in refs], dtype=np.float64), max_iters=200)
    eq.close()
    yield p, col, reads, ab
    col.close(); p.close()


def test_batch_assign_bins_and_pairs(three):
    p, col, reads, ab = three
    x = ab.weights()
    assert x[0] > x[1] > x[2] > 0
    asg = col.assigner(x, ab.theta)      # the mGEMS rule
    b = p.batch(reads)
    b.run(fa.FIN_MERGED)
    prow, phead = b.pseudoalign(col, 1000)
    frow = {both: b.pseudoalign_pairs(col, 1000, both)[0].copy() for both in (False, True)}
    # per read
    rows, heads = b.assign(asg)
    twin = fa.rows_assign(prow, 3, x, ab.theta)
    assert_same((rows, heads) + asg.download(), twin, "Batch.assign")
    assert int(twin[4][1]) > 0 and int(twin[2].sum()) > 0
    assert b.device_assign_ptrs()[0] != 0 and b.device_assign_ptrs()[1] != 0
    M = unpack_bool(rows, 3)
    for c in range(3):
        ids = b.assign_bin(c)
        assert ids.dtype == np.uint32 and ids.tolist() == np.flatnonzero(M[:, c]).tolist(), "bin of colour %d" % c
        assert b.device_bin_ptr() != 0
    with pytest.raises(fa.FinitoError) as e:
        b.assign_bin(3)
    assert e.value.code == fa.FIN_EINVAL and "colour 3" in str(e.value)
    # a colour nobody has: a weight of 0 is never assigned
    x0 = x.copy(); x0[2] = 0.0
    asg.set(x0, 0.0).reset()
    rows0, _ = b.assign(asg)
    assert len(b.assign_bin(2)) == 0 and b.assign_bin(0).tolist() == np.flatnonzero(unpack_bool(rows0, 3)[:, 0]).tolist()
    asg.set(x, ab.theta).reset()
    # per fragment, on a stream of the caller's
    S = torch.cuda.Stream()
    for both in (False, True):
        asg.reset()
        rows, heads = b.assign(asg, pairs=True, both=both, stream=S.cuda_stream)
        twin = fa.rows_assign(frow[both], 3, x, ab.theta)
        assert_same((rows, heads) + asg.download(), twin, "Batch.assign, pairs, both %s" % both)
        Mf = unpack_bool(rows, 3)
        for c in range(3):
            assert b.assign_bin(c).tolist() == np.flatnonzero(Mf[:, c]).tolist()
    # the pseudo rows and the pair rows are unchanged
    r2, h2 = (np.zeros_like(prow), np.zeros_like(phead))
    import ctypes as C
    err = C.create_string_buffer(512)
    assert b.L.fin_batch_download_pseudo(b.h, r2.ctypes.data_as(C.POINTER(C.c_uint64)), h2.ctypes.data_as(C.c_void_p), err, 512) == 0
    assert r2.tobytes() == prow.tobytes() and h2.tobytes() == phead.tobytes()
    f2 = np.zeros_like(frow[True])
    assert b.L.fin_batch_download_pair_pseudo(b.h, f2.ctypes.data_as(C.POINTER(C.c_uint64)), None, err, 512) == 0
    assert f2.tobytes() == frow[True].tobytes()
    # an odd number of reads with pairs
    odd = p.batch(reads[:11]); odd.run(fa.FIN_MERGED)
    with pytest.raises(fa.FinitoError) as e:
        odd.assign(asg, pairs=True)
    assert e.value.code == fa.FIN_EINVAL and "odd" in str(e.value)
    odd.close(); b.close(); asg.close()


def test_add_reads_in_sub_batches(three):
    p, col, reads, ab = three
    x = ab.weights()
    asg = col.assigner(x, 0.3)
    one = {}
    for pairs, both in ((False, False), (True, False), (True, True)):
        asg.reset()
        rows, heads = asg.add_reads(reads, pairs=pairs, both=both)
        one[pairs, both] = (rows, heads) + asg.download()
        assert int(one[pairs, both][4][0]) == (len(reads) // 2 if pairs else len(reads))
    b = p.batch(reads); b.run(fa.FIN_MERGED)
    asg.reset()
    assert_same(b.assign(asg) + asg.download(), one[False, False], "one batch")
    b.close()
    nk = np.array([max(len(r) - p.k + 1, 0) for r in reads])
    limit = int(nk.sum()) // 7
    cuts = np.searchsorted(np.concatenate([[0], np.cumsum(nk)]), np.arange(1, 7) * limit)
    assert (cuts % 2 == 1).any()            # cuts by single reads would fall inside a pair
    p.set_option("pipeline_kmers", limit); p.set_option("pipeline_depth", 3)
    try:
        for key in one:
            asg.reset()
            rows, heads = asg.add_reads(reads, pairs=key[0], both=key[1])
            assert_same((rows, heads) + asg.download(), one[key], "sub-batches, pairs %s both %s" % key)
            none, heads2 = asg.add_reads(reads, pairs=key[0], both=key[1], want_rows=False)
            assert none is None and heads2.tobytes() == heads.tobytes()
    finally:
        p.set_option("pipeline_kmers", None); p.set_option("pipeline_depth", None)
    with pytest.raises(fa.FinitoError) as e:
        asg.add_reads(reads[:11], pairs=True)
    assert e.value.code == fa.FIN_EINVAL and "odd" in str(e.value)
    asg.close()


# ---- bins of a colour in every word, bit 63, partial waves and blocks, more than 1024 blocks of 256 rows ----------------------------------------------------
BIN_COLORS = (0, 63, 64, 127, 128, 129)   # the first and last bit of words 0 and 1, the first bit of word 2 and the top colour
NOBODY = 77                               # a colour no unitig has: an empty bin


@pytest.fixture(scope="module")
def coloured(small):
    """the small index with 130 colours drawn at random over its unitigs -- words 0, 1 and 2 all populated, the colours of BIN_COLORS on many unitigs, NOBODY on
    none --, an assigner that keeps every colour of a row (all weights 1, thresholds 0), and the index's text to cut reads from"""
    p, _, _ = small
    rng = np.random.default_rng(3950)
    n_colors = 130
    member = rng.random((p.n_unitigs, n_colors)) < 0.03
    member[np.arange(p.n_unitigs), np.array(BIN_COLORS)[rng.integers(0, len(BIN_COLORS), p.n_unitigs)]] |= rng.random(p.n_unitigs) < 0.7
    member[:, NOBODY] = False
    bits = pack_members(member)
    assert bits.shape[1] == 3 and bits.any(axis=0).all() and all(member[:, c].sum() >= 10 for c in BIN_COLORS) and not member.any(axis=1).all()
    col = p.colors(n_colors, bits)
    asg = col.assigner(np.ones(n_colors), 0.0)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[p.export(fa.X_CONCAT)]
    yield p, col, asg, text, p.export(fa.X_ENDS).astype(np.int64), n_colors
    asg.close(); col.close()


def cut_reads(rng, text, ends, k, n):
    """n reads of k bases, each cut from inside one unitig (nk = 1), as (bases, offsets)"""
    starts = np.concatenate([[0], ends[:-1]])
    u = rng.integers(0, len(ends), n)
    a = starts[u] + (rng.random(n) * (ends[u] - starts[u] - k + 1)).astype(np.int64)
    bases = np.ascontiguousarray(text[a[:, None] + np.arange(k)[None, :]]).reshape(-1)
    return bases, (np.arange(n + 1, dtype=np.uint64) * np.uint64(k))


def check_bins(b, asg, n_colors, colours, what):
    """Batch.assign_bin against the rows Batch.assign returns: np.flatnonzero over the unpacked column; returns the rows"""
    rows, _ = b.assign(asg.reset())
    M = unpack_bool(rows, n_colors)
    for c in colours:
        ids = b.assign_bin(c)
        want = np.flatnonzero(M[:, c])
        assert ids.dtype == np.uint32 and np.array_equal(ids, want), "%s: bin of colour %d: %d ids, %d rows have the colour" % (what, c, len(ids), len(want))
    return rows, M


@pytest.mark.parametrize("n_reads", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_bins_of_colours_in_every_word(coloured, n_reads):
    """fin_assign_column_kernel at W = 3: the word of the colour (c >> 6), bit 63 of a word, a last wave and a last block that are partial"""
    p, col, asg, text, ends, n_colors = coloured
    rng = np.random.default_rng(3960 + n_reads)
    b = p.batch(cut_reads(rng, text, ends, p.k, n_reads)); b.run(fa.FIN_MERGED)
    rows, M = check_bins(b, asg, n_colors, BIN_COLORS + (NOBODY,), "%d reads" % n_reads)
    assert rows.shape == (n_reads, 3) and len(b.assign_bin(NOBODY)) == 0
    if n_reads == 1000:
        assert all(M[:, c].sum() >= 20 for c in BIN_COLORS) and rows.any(axis=0).all() and not M.any(axis=1).all()
        assert M[-1].any() or M[-2].any() or M[-3].any()   # the partial block's rows are not all empty
    b.close()


def test_bins_past_one_block_a_scan_thread(coloured):
    """more than 262 144 reads, that is more than 1024 blocks of 256 rows: a thread of fin_blk_scan_kernel carries two blocks, and the last block is partial"""
    p, col, asg, text, ends, n_colors = coloured
    n_reads = 262_144 + 256 + 57
    b = p.batch(cut_reads(np.random.default_rng(3970), text, ends, p.k, n_reads)); b.run(fa.FIN_MERGED)
    rows, M = check_bins(b, asg, n_colors, (0, 128), "%d reads" % n_reads)
    for c in (0, 128):   # rows on both sides of the first level's end and in the last, partial block
        have = np.flatnonzero(M[:, c])
        assert (have < 262_144).sum() > 1000 and (have >= 262_144).any() and (have >= 262_144 + 256).any()
    b.close()
