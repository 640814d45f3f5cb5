"""Merging equivalence classes, the parts that need no GPU (include/finito_amd.h: fin_classes_merge; finito_amd/dist.py: gather_other_classes): the host twin
of the weighted add against a brute-force model -- both lists expanded to rows, np.unique(axis=0, return_counts=True) --, weights above 2^32 against Python
integers, what is refused, and the gather-and-merge arithmetic of allreduce_eqclasses on two gloo ranks.  Every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import finito_amd as fa
from tests.test_colors_host import words_of
from tests.test_dist import _free_port
from tests.test_eqclasses_host import assert_classes, classes_of_rows, random_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64P = C.POINTER(C.c_uint64)


def weighted_classes(rows, weights, n_unaligned, n_colors):
    """the definition of the weighted add in Python integers: (class rows in canonical order, reads, n_unaligned) of rows[r] counted weights[r] times and
    n_unaligned empty rows besides; a class of 0 reads is none"""
    W = words_of(n_colors)
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, W)
    total, un = {}, int(n_unaligned)
    for row, w in zip(rows, weights):
        if not row.any():
            un += int(w)
        elif int(w):
            total[row.tobytes()] = total.get(row.tobytes(), 0) + int(w)
    if not total:
        return np.zeros((0, W), dtype=np.uint64), np.zeros(0, dtype=np.uint64), un
    distinct = np.unique(np.array([np.frombuffer(b, dtype=np.uint64) for b in total]).reshape(-1, W), axis=0)
    return distinct, np.array([total[r.tobytes()] for r in distinct], dtype=np.uint64), un


def a_class_list(rng, n_colors, n, max_weight=5):
    """an unsorted class list with duplicate rows and one class of 0 reads: (rows, reads)"""
    rows = random_rows(rng, n, n_colors, max(n // 3, 2), empty_share=0.0)
    reads = rng.integers(1, max_weight + 1, n).astype(np.uint64)
    reads[n // 2] = 0
    return rows, reads


@pytest.mark.parametrize("n_colors", [5, 130, 4096])
def test_classes_merge_against_the_expanded_rows(n_colors):
    rng = np.random.default_rng(3100 + n_colors)
    W = words_of(n_colors)
    ra, wa = a_class_list(rng, n_colors, 60)
    rb, wb = a_class_list(rng, n_colors, 45)
    rb[:7] = ra[:7]                       # rows in both lists
    ra[20] = ra[3]; wa[20] = 2; wa[3] = 4   # ... and twice in one
    lone = np.zeros(W, dtype=np.uint64); lone[W - 1] = np.uint64(1) << np.uint64((n_colors - 1) & 63); lone[0] |= np.uint64(1)
    assert not (ra == lone).all(axis=1).any() and not (rb == lone).all(axis=1).any()
    rb[10] = lone; wb[10] = 0             # a class of 0 reads whose row occurs nowhere else
    assert len(np.unique(np.concatenate([ra, rb]), axis=0)) < len(ra) + len(rb) - 7
    expanded = np.concatenate([np.repeat(ra, wa.astype(np.int64), axis=0), np.repeat(rb, wb.astype(np.int64), axis=0)])
    want = classes_of_rows(expanded, n_colors)
    assert want[2] == 0 and not (want[0] == lone).all(axis=1).any()
    got = fa.classes_merge(ra, wa, rb, wb, n_colors)
    assert_classes(got + (0,), want, "%d colours" % n_colors)
    assert_classes(fa.classes_merge(rb, wb, ra, wa, n_colors) + (0,), want, "%d colours, the other way round" % n_colors)
    assert_classes(weighted_classes(np.concatenate([ra, rb]), np.concatenate([wa, wb]), 0, n_colors), want, "the integer model")
    # one side empty, both sides empty
    none_r, none_w = np.zeros((0, W), dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    alone = classes_of_rows(np.repeat(ra, wa.astype(np.int64), axis=0), n_colors)
    assert_classes(fa.classes_merge(ra, wa, none_r, none_w, n_colors) + (0,), alone, "b empty")
    assert_classes(fa.classes_merge(none_r, none_w, ra, wa, n_colors) + (0,), alone, "a empty")
    rows, reads = fa.classes_merge(none_r, none_w, none_r, none_w, n_colors)
    assert rows.shape == (0, W) and len(reads) == 0
    # merging the merged list with nothing changes nothing: the output is a class list
    assert_classes(fa.classes_merge(got[0], got[1], none_r, none_w, n_colors) + (0,), want, "idempotent")


def test_weights_above_two_to_the_32():
    n_colors = 70
    rng = np.random.default_rng(3170)
    big = [1, 2, 1 << 32, (1 << 40) + 3, (1 << 58) + 5]
    ra = random_rows(rng, 30, n_colors, 8, empty_share=0.0)
    rb = ra[rng.permutation(30)][:20]
    wa = np.array([big[i % 5] for i in range(30)], dtype=np.uint64)
    wb = np.array([big[(3 * i + 1) % 5] for i in range(20)], dtype=np.uint64)
    want = weighted_classes(np.concatenate([ra, rb]), [int(x) for x in wa] + [int(x) for x in wb], 0, n_colors)
    assert int(want[1].max()) > 1 << 58 and len(want[0]) <= 8
    sums = {}
    for row, w in list(zip(ra, wa)) + list(zip(rb, wb)):
        sums[row.tobytes()] = sums.get(row.tobytes(), 0) + int(w)
    assert max(sums.values()) < 1 << 64
    got = fa.classes_merge(ra, wa, rb, wb, n_colors)
    assert_classes(got + (0,), want, "big weights")
    assert [int(x) for x in got[1]] == [sums[r.tobytes()] for r in got[0]]


def test_refusals():
    L = fa.lib()
    n = C.c_uint64(99)
    out, reads = np.zeros((4, 1), dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    p = lambda a: np.ascontiguousarray(a, dtype=np.uint64).ctypes.data_as(U64P)

    def ask(ra, wa, rb, wb, n_colors, cap):
        ra, wa, rb, wb = (np.ascontiguousarray(x, dtype=np.uint64) for x in (ra, wa, rb, wb))
        return L.fin_classes_merge(p(ra), p(wa), len(wa), p(rb), p(wb), len(wb), n_colors, out.ctypes.data_as(U64P), reads.ctypes.data_as(U64P), cap, C.byref(n))
    a, wa, b, wb = [[3], [1]], [2, 5], [[2], [3]], [7, 1]
    assert ask(a, wa, b, wb, 5, 3) == fa.FIN_OK and n.value == 3 and out[:3, 0].tolist() == [1, 2, 3] and reads[:3].tolist() == [5, 7, 3]
    n.value = 99
    assert ask(a, wa, b, wb, 5, 2) == fa.FIN_ELIMIT and n.value == 3           # cap one too small: the number of classes is still reported
    stray = [[1], [1 << 5]]
    assert ask(stray, [1, 1], b, wb, 5, 4) == fa.FIN_EINVAL and ask(b, wb, stray, [1, 1], 5, 4) == fa.FIN_EINVAL and ask(stray, [1, 1], b, wb, 6, 4) == fa.FIN_OK
    assert ask(stray, [1, 0], b, wb, 5, 4) == fa.FIN_EINVAL                    # ... in a class of 0 reads too
    for bad in (0, 4097):
        assert ask(a, wa, b, wb, bad, 4) == fa.FIN_ELIMIT
        with pytest.raises(fa.FinitoError) as e:
            fa.classes_merge(a, wa, b, wb, bad)
        assert e.value.code == fa.FIN_ELIMIT
    with pytest.raises(fa.FinitoError) as e:
        fa.classes_merge(stray, [1, 1], b, wb, 5)
    assert e.value.code == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:
        fa.classes_merge(a, [1], b, wb, 5)                                     # two rows, one count
    assert e.value.code == fa.FIN_EINVAL


# ---- two gloo ranks: the gather allreduce_eqclasses uses, without an accumulator -------------------------------------------------------------------
def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    from finito_amd import dist as fdist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        n_colors = 130
        rows = random_rows(np.random.default_rng(3190), 900, n_colors, 25)   # the same set on every rank
        cut = [0, 431, 900]
        mine = fa.rows_eqclasses(rows[cut[rank]:cut[rank + 1]], n_colors)
        others = fdist.gather_other_classes(*mine, rank, dist)
        assert len(others) == world - 1
        got_rows, got_reads, got_un = mine
        for o_rows, o_reads, o_un in others:
            got_rows, got_reads = fa.classes_merge(got_rows, got_reads, o_rows, o_reads, n_colors)
            got_un += o_un
        assert_classes((got_rows, got_reads, got_un), classes_of_rows(rows, n_colors), "rank %d" % rank)
        verdicts = [None] * world
        dist.all_gather_object(verdicts, True)
        if rank == 0:
            q.put(all(verdicts))
    finally:
        dist.destroy_process_group()


def test_two_ranks_gather_and_merge_cpu():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    assert q.get(timeout=5) is True
