"""Merging equivalence-class accumulators on the device (include/finito_amd.h: fin_eqclasses_add_classes, fin_eqclasses_add_classes_host, fin_eqclasses_merge;
fin_eqclasses.hip: the weighted add; finito_amd/dist.py: replicate_colors, allreduce_eqclasses).  The expectation is the definition in Python integers
(tests/test_eqclasses_merge_host.py::weighted_classes) or in numpy (tests/test_eqclasses_host.py::classes_of_rows), never a device output; the table mirror of
tests/test_eqclasses_table_host.py chooses rows and gives the number of collision-list entries.  Integer comparisons are exact."""
import os
import sys

import numpy as np
import pytest
import torch

import finito_amd as fa
from finito_amd import dist as fdist
from tests.test_abundance_host import rtol1
from tests.test_colors_host import pack, random_matrix, rows_of
from tests.test_dist import _free_port
from tests.test_eqclasses import N_COLORS_OF_W, assert_all, on_device, set31, small   # noqa: F401 (the fixtures: the suite's small index and read set)
from tests.test_eqclasses_host import assert_classes, classes_of_rows, random_rows
from tests.test_eqclasses_merge_host import weighted_classes
from tests.test_eqclasses_table_host import TableModel, chain_rows, draw_rows, ec_home, lg_of, tags_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [1, 2, 1 << 32, (1 << 40) + 3]


def assert_weighted(eq, want, what, serial=None):
    """download and stats against the definition"""
    assert_classes(eq.download(), want, what)
    st = eq.stats()
    assert st[:3] == [sum(int(x) for x in want[1]) + want[2], want[2], len(want[0])], "%s: stats %s" % (what, st)
    if serial is not None:
        assert st[3] == serial, "%s: %d rows through the serial pass, the mirror has %d" % (what, st[3], serial)


def device_list(rows, weights):
    return on_device(rows), on_device(np.asarray(weights, dtype=np.uint64))


# ---- 1. the weighted add against the model -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 64])
def test_weighted_add_against_the_model(small, W):
    p, g, _ = small
    rng = np.random.default_rng(3200 + W)
    n_colors = N_COLORS_OF_W[W]
    col = p.colors(n_colors)
    eq = col.eqclasses(1024)
    lone = pack([[0, n_colors - 1, 7]], n_colors)[0]
    for n in (1, 63, 64, 65, 257):
        rows = random_rows(rng, n, n_colors, max(n // 4, 1), empty_share=0.0)
        assert not (rows == lone).all(axis=1).any()
        weights = np.array([WEIGHTS[i] for i in rng.integers(0, 4, n)], dtype=np.uint64)
        if n > 1:
            rows[n // 2] = 0; weights[n // 2] = (1 << 40) + 3           # an all-zero row with a weight
            rows[n - 1] = 0; weights[n - 1] = 2                         # ... and one in the last lane of the list
            rows[n // 3] = lone; weights[n // 3] = 0                    # a row of weight 0 that occurs nowhere else
            rows[1] = rows[0]                                           # a duplicate, whatever the draw gave
            assert len(np.unique(rows, axis=0)) < n
        want = weighted_classes(rows, [int(x) for x in weights], 3, n_colors)
        assert not (want[0] == lone).all(axis=1).any() and (n == 1 or want[2] > 1 << 40)
        what = "W=%d, %d classes" % (W, n)
        eq.reset().add_classes(rows, weights, 3)
        assert_weighted(eq, want, what + ", host arrays", serial=0)
        tr, tw = device_list(rows, weights)
        assert eq.reset().add_classes_device(tr.data_ptr(), tw.data_ptr(), n, 3) is eq
        assert_weighted(eq, want, what + ", device pointers", serial=0)
        eq.add_classes_device(tr.data_ptr(), tw.data_ptr(), n)       # a second add meets the classes of the first
        twice = weighted_classes(np.concatenate([rows, rows]), [int(x) for x in weights] * 2, 3, n_colors)
        assert_weighted(eq, twice, what + ", added twice", serial=0)
    # no classes, seven unaligned reads
    none = (np.zeros((0, W), dtype=np.uint64), np.zeros(0, dtype=np.uint64), 7)
    eq.reset().add_classes(none[0], none[1], 7)
    assert_weighted(eq, none, "W=%d, nothing but unaligned reads, host arrays" % W)
    eq.reset().add_classes_device(0, 0, 0, 7)
    assert_weighted(eq, none, "W=%d, nothing but unaligned reads, device pointers" % W)
    eq.add_classes_device(0, 0, 0, 0).add_classes(none[0], none[1])
    assert_weighted(eq, none, "W=%d, empty adds" % W)
    eq.close(); col.close()


# ---- 2. merge ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 64])
def test_merge(small, W):
    p, g, _ = small
    rng = np.random.default_rng(3300 + W)
    n_colors = N_COLORS_OF_W[W]
    col = p.colors(n_colors)
    rows = random_rows(rng, 1001, n_colors, 50)
    cut = 433
    ta, tb = on_device(rows[:cut]), on_device(rows[cut:])
    A, B = col.eqclasses(1024), col.eqclasses(256)
    A.add_rows(ta.data_ptr(), cut)
    B.add_rows(tb.data_ptr(), len(rows) - cut)
    want_b = classes_of_rows(rows[cut:], n_colors)
    assert want_b[2] > 0 and len(classes_of_rows(rows[:cut], n_colors)[0]) != len(classes_of_rows(rows, n_colors)[0])
    assert A.merge(B) is A
    assert_all(A, classes_of_rows(rows, n_colors), n_colors, "W=%d, merged" % W, n_rows=len(rows))
    assert_all(B, want_b, n_colors, "W=%d, the source afterwards" % W, n_rows=len(rows) - cut)
    A.merge(B)                                    # a second time: counted twice
    assert_all(A, classes_of_rows(np.concatenate([rows, rows[cut:]]), n_colors), n_colors, "W=%d, merged twice" % W)
    E = col.eqclasses(16)
    A.merge(E)                                    # an empty source
    assert_all(A, classes_of_rows(np.concatenate([rows, rows[cut:]]), n_colors), n_colors, "W=%d, an empty source" % W)
    E.close()
    E = col.eqclasses(64)
    E.merge(B)                                    # into an empty destination
    assert_all(E, want_b, n_colors, "W=%d, into an empty accumulator" % W)
    U = col.eqclasses(8)                          # a source that holds only unaligned rows
    tz = on_device(np.zeros((70, W), dtype=np.uint64))
    U.add_rows(tz.data_ptr(), 70)
    E.merge(U)
    assert_all(E, (want_b[0], want_b[1], want_b[2] + 70), n_colors, "W=%d, a source of unaligned rows" % W)
    for x in (A, B, E, U):
        x.close()
    col.close()


# ---- 3. the serial pass with weights -----------------------------------------------------------------------------------------------------------
def serial_case(rng, tag_bits, max_classes, W):
    """under one tag: the owner, the chain rows A holds behind it, and a list of rows that are in A (serial match) and rows that are new (serial claim),
    long enough for the chain to cross the table's end; weights; the mirror's count of collision-list entries for A's adds and for the list"""
    lg = lg_of(max_classes)
    main_tag = max(range(1, 1 << tag_bits), key=lambda t: ec_home(t, lg))
    owner, chain, _ = chain_rows(rng, max_classes, tag_bits, W, main_tag, max_classes - 1, False)
    held = chain[: len(chain) // 2]
    listed = np.concatenate([owner, chain[len(held) // 2:], chain[-1:]])   # the owner, rows in A, new rows, and the last new row twice
    listed = listed[rng.permutation(len(listed))]
    weights = np.array([WEIGHTS[i] for i in rng.integers(0, 4, len(listed))], dtype=np.uint64)
    assert (tags_of(np.concatenate([owner, chain]), tag_bits) == main_tag).all()
    m = TableModel(max_classes, tag_bits, W)
    before = m.add(owner).serial + m.add(held).serial
    rep = m.add(listed)
    assert before == len(held) and rep.serial == len(listed) - 1 and (rep.window_wrapped or rep.start_wrapped) and not rep.limit_claim and not rep.limit_serial
    return owner, held, listed, weights, before, rep.serial


@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("tag_bits,max_classes", [(4, 16), (1, 16), (4, 4)])
def test_the_serial_pass_with_weights(small, W, tag_bits, max_classes):
    p, g, _ = small
    rng = np.random.default_rng(3400 + 10 * tag_bits + max_classes + W)
    n_colors = 64 * W
    assert 2 <= 1 << lg_of(max_classes) <= 32
    owner, held, listed, weights, before, serial = serial_case(rng, tag_bits, max_classes, W)
    col = p.colors(n_colors)
    t_owner, t_held = on_device(owner), on_device(held)
    what = "W=%d, %d tag bits, %d slots" % (W, tag_bits, 1 << lg_of(max_classes))
    in_a = np.concatenate([owner, held])
    want = weighted_classes(np.concatenate([in_a, listed]), [1] * len(in_a) + [int(x) for x in weights], 0, n_colors)
    assert len(want[0]) == max_classes
    p.set_option("ec_tag_bits", tag_bits)
    try:
        A = col.eqclasses(max_classes)
        A.add_rows(t_owner.data_ptr(), 1).add_rows(t_held.data_ptr(), len(held))
        assert A.stats()[3] == before
        tr, tw = device_list(listed, weights)
        A.add_classes_device(tr.data_ptr(), tw.data_ptr(), len(listed))
        assert_weighted(A, want, what + ", a list", serial=before + serial)
        # the same through a merge: the source's dense list holds every listed row once, in its own slot order
        B = col.eqclasses(max_classes)
        B.add_classes(listed, weights)
        A.reset().add_rows(t_owner.data_ptr(), 1).add_rows(t_held.data_ptr(), len(held))
        A.merge(B)
        assert_weighted(A, want, what + ", a merge", serial=before + serial - 1)   # (the row listed twice is one class of the source)
        A.close(); B.close()
    finally:
        p.set_option("ec_tag_bits", None)
    col.close()


# ---- 4. capacity and flags ---------------------------------------------------------------------------------------------------------------------
def test_capacity_and_flags(small):
    p, g, rng = small
    n_colors, W = 128, 2
    col = p.colors(n_colors)
    pool = np.unique(rng.integers(1, 1 << 63, size=(130, W), dtype=np.uint64), axis=0)
    assert len(pool) == 130
    t60, t_other = on_device(pool[:60]), on_device(pool[60:120])
    A, B = col.eqclasses(100), col.eqclasses(1000)
    A.add_rows(t60.data_ptr(), 60)
    B.add_rows(t_other.data_ptr(), 60)
    A.merge(B)                                    # 120 distinct rows, full-width tags: the claim pass meets the limit
    for _ in range(2):
        with pytest.raises(fa.FinitoError) as e:
            A.download()
        assert e.value.code == fa.FIN_ELIMIT and "max_classes" in str(e.value)
    assert A.stats()[3] == 0
    with pytest.raises(fa.FinitoError) as e:      # a flagged source is refused, the destination is unchanged
        B.merge(A)
    assert e.value.code == fa.FIN_ELIMIT
    assert_all(B, classes_of_rows(pool[60:120], n_colors), n_colors, "the destination of a refused merge", n_rows=60)
    A.reset().add_rows(t60.data_ptr(), 60)
    t40 = on_device(pool[60:100])
    B.reset().add_rows(t40.data_ptr(), 40)
    A.merge(B)                                    # exactly max_classes
    assert_all(A, classes_of_rows(pool[:100], n_colors), n_colors, "after the reset, exactly max_classes", n_rows=100)
    A.close(); B.close()
    # the limit met only in the serial pass: one tag, the owner in the table, max_classes new rows in the list
    rows = draw_rows(rng, W, 6, 1, lg_of(4))
    t_owner = on_device(rows[:1])
    p.set_option("ec_tag_bits", 1)
    try:
        A = col.eqclasses(4)
        A.add_rows(t_owner.data_ptr(), 1)
        A.add_classes(rows[1:5], [5, 1 << 32, 1, 2])
        with pytest.raises(fa.FinitoError) as e:
            A.download()
        assert e.value.code == fa.FIN_ELIMIT and A.stats()[3] == 4
        A.reset().add_rows(t_owner.data_ptr(), 1)
        A.add_classes(rows[1:4], [5, 1 << 32, 1])
        assert_weighted(A, weighted_classes(rows[:4], [1, 5, 1 << 32, 1], 0, n_colors), "after the reset, the serial pass below the limit", serial=3)
        A.close()
    finally:
        p.set_option("ec_tag_bits", None)
    # stray bits: n_colors 70, bit 6 of word 1 and above belong to no colour
    col70 = p.colors(70)
    A = col70.eqclasses(64)
    good = pack([[0, 69], [3], [5, 64]], 70)
    A.add_classes(good, [4, 1, 1 << 33], 2)
    want = weighted_classes(good, [4, 1, 1 << 33], 2, 70)
    bad = good.copy(); bad[1, 1] |= np.uint64(1) << np.uint64(6)
    for w in ([1, 1, 1], [1, 0, 1]):              # refused at the call, whatever the class's reads
        with pytest.raises(fa.FinitoError) as e:
            A.add_classes(bad, w)
        assert e.value.code == fa.FIN_EINVAL and "n_colors" in str(e.value)
    assert_weighted(A, want, "after the refused host add")
    tr, tw = device_list(bad, [1, 1, 1])
    A.add_classes_device(tr.data_ptr(), tw.data_ptr(), 3)
    for _ in range(2):
        with pytest.raises(fa.FinitoError) as e:
            A.download()
        assert e.value.code == fa.FIN_EINVAL and "n_colors" in str(e.value)
    D = col70.eqclasses(64)
    with pytest.raises(fa.FinitoError) as e:
        D.merge(A)
    assert e.value.code == fa.FIN_EINVAL and D.stats()[:3] == [0, 0, 0]
    A.reset().add_classes(good, [4, 1, 1 << 33], 2)
    assert_weighted(A, want, "after the reset")
    # refusals of merge
    with pytest.raises(fa.FinitoError) as e:
        A.merge(None)
    assert e.value.code == fa.FIN_EINVAL
    err = fa.C.create_string_buffer(512)
    assert fa.lib().fin_eqclasses_merge(A.h, None, None, err, 512) == fa.FIN_EINVAL and fa.lib().fin_eqclasses_merge(None, A.h, None, err, 512) == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:
        A.merge(A)
    assert e.value.code == fa.FIN_EINVAL
    other = col.eqclasses(64)                     # 128 colours against 70
    with pytest.raises(fa.FinitoError) as e:
        A.merge(other)
    assert e.value.code == fa.FIN_EINVAL and "n_colors" in str(e.value)
    assert_weighted(A, want, "after the refused merges")
    same = p.colors(70)                           # another colour object with the same n_colors: legal
    S = same.eqclasses(64)
    S.merge(A)
    assert_weighted(S, want, "colours of another object, equal n_colors")
    for x in (A, D, S, other):
        x.close()
    same.close(); col70.close(); col.close()


# ---- 5. order ----------------------------------------------------------------------------------------------------------------------------------
def test_merges_adds_and_a_reset_on_several_streams(small):
    p, g, _ = small
    rng = np.random.default_rng(3500)
    n_colors = 100
    col = p.colors(n_colors)
    r1, r2, rb = (random_rows(rng, n, n_colors, 30) for n in (300, 517, 411))
    t1, t2, tb = on_device(r1), on_device(r2), on_device(rb)
    s1, s2, s3 = (torch.cuda.Stream() for _ in range(3))
    A, B = col.eqclasses(256), col.eqclasses(256)
    B.add_rows(tb.data_ptr(), len(rb), stream=s3.cuda_stream)          # (the merge waits for it)
    A.add_rows(t1.data_ptr(), len(r1), stream=s1.cuda_stream)
    A.merge(B, stream=s1.cuda_stream)
    A.add_rows(t2.data_ptr(), len(r2), stream=s1.cuda_stream)
    assert_all(A, classes_of_rows(np.concatenate([r1, rb, r2]), n_colors), n_colors, "add, merge, add on one stream", n_rows=len(r1) + len(rb) + len(r2))
    A.add_rows(t1.data_ptr(), len(r1), stream=s1.cuda_stream)
    A.merge(B, stream=s2.cuda_stream)
    A.reset(stream=s3.cuda_stream)                                      # on another stream: behind everything issued so far
    A.merge(B, stream=s1.cuda_stream)
    A.add_rows(t2.data_ptr(), len(r2), stream=s2.cuda_stream)
    B.reset(stream=s2.cuda_stream)                                      # the source emptied right behind the merge: the gather came first
    assert_all(A, classes_of_rows(np.concatenate([rb, r2]), n_colors), n_colors, "what was issued behind the reset", n_rows=len(rb) + len(r2))
    assert B.stats()[:3] == [0, 0, 0]
    A.close(); B.close(); col.close()


# ---- 6. real reads and what comes after ----------------------------------------------------------------------------------------------------------
def test_real_reads_in_two_shards_and_the_estimates(set31):
    p, o, g, unitigs, reads, bits, n_colors, rng = set31
    bases, offsets = fa.flatten(reads)
    col = p.colors(n_colors, bits)
    whole = col.eqclasses(4096).add_reads(reads)
    parts = [col.eqclasses(4096) for _ in range(2)]
    for rank, e in enumerate(parts):
        my_bases, my_offs, (lo, hi) = fdist.shard_reads(bases, offsets, rank, 2)
        assert 0 < hi - lo < len(reads)
        e.add_reads((my_bases, my_offs))
    merged = parts[0].merge(parts[1])
    want = whole.download()
    assert len(want[0]) > 5 and want[2] > 0
    assert_classes(merged.download(), want, "two shards merged")
    assert merged.stats()[:3] == whole.stats()[:3]
    # downstream: the estimates take the merged accumulator as they take any
    crows, creads, un = merged.download()
    r = rtol1(len(crows), n_colors)
    got, twin = merged.abundance(max_iters=1, tol=0.0), fa.classes_abundance(crows, creads, n_colors, max_iters=1, tol=0.0)
    assert got.n_unaligned == un and np.array_equal(got.alpha == 0, twin.alpha == 0) and (np.abs(got.alpha - twin.alpha) <= r * np.abs(twin.alpha)).all()
    bm, bw = merged.bootstrap(n_boot=3, seed=5, max_iters=1, tol=0.0), whole.bootstrap(n_boot=3, seed=5, max_iters=1, tol=0.0)
    assert np.array_equal(bm.n_reads, bw.n_reads) and int(bm.n_reads.min()) > 0
    bt = fa.classes_bootstrap(crows, creads, n_colors, 3, seed=5, max_iters=1, tol=0.0)
    assert np.array_equal(bm.n_reads, bt.n_reads)
    assert np.array_equal(bm.alpha == 0, bt.alpha == 0) and (np.abs(bm.alpha - bt.alpha) <= r * np.abs(bt.alpha)).all()
    # fragments, cut after an even number of reads
    cut = 2 * (len(reads) // 4) + 2
    n_even = len(reads) - len(reads) % 2
    whole.reset().add_read_pairs(reads[:n_even])
    parts[0].reset().add_read_pairs(reads[:cut])
    parts[1].reset().add_read_pairs(reads[cut:n_even])
    assert_classes(parts[0].merge(parts[1]).download(), whole.download(), "fragments in two parts merged")
    for e in parts + [whole]:
        e.close()
    col.close()


# ---- 7. two ranks --------------------------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, tmp, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    from finito_amd import synth
    from oracle.oracle import OracleIndex
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        k, n_colors = 21, 70
        g = synth.genome(60_000)
        u = synth.unitigs(g, k, max_len=300)
        bases, offsets = synth.reads(g, 900, read_len=120).as_tuple()
        idx = fdist.replicate_index(lambda: fa.FinimizerIndex.build(u.as_tuple(), k, n_threads=2), os.path.join(tmp, "idx"), rank, dist)
        idx.to_device(0)
        bits = random_matrix(np.random.default_rng(3600), idx.n_unitigs, n_colors)
        col = fdist.replicate_colors(idx.colors(n_colors, bits) if rank == 0 else None, idx, n_colors, rank, dist)
        assert np.array_equal(col.download()[0], bits)
        my_bases, my_offs, _ = fdist.shard_reads(bases, offsets, rank, world)
        eq = col.eqclasses(4096).add_reads((my_bases, my_offs))
        assert fdist.allreduce_eqclasses(eq, dist) is eq
        o = OracleIndex.from_components(k, idx.components())
        pairs, _, _ = o.search_batch((bases, offsets))
        nks = np.maximum(np.diff(np.asarray(offsets).astype(np.int64)) - k + 1, 0)
        want = classes_of_rows(rows_of(pairs, nks, bits, n_colors, 1000)[0], n_colors)
        assert len(want[0]) > 3
        assert_classes(eq.download(), want, "rank %d" % rank)
        verdicts = [None] * world
        dist.all_gather_object(verdicts, True)
        if rank == 0:
            q.put(all(verdicts))
        eq.close(); col.close(); idx.close()
    finally:
        dist.destroy_process_group()


def test_two_ranks_gloo_allreduce(tmp_path):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(300)
        assert pr.exitcode == 0
    assert q.get(timeout=5) is True
