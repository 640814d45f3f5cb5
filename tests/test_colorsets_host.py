"""Deduplicated colour sets on the host (fin_unitig_color_sets, fin_color_sets_expand): the canonical form against np.unique.  No device."""
import ctypes as C

import numpy as np
import pytest

import finito_amd as fa
from tests.test_colors_host import random_matrix, words_of

N_COLORS = (1, 5, 64, 65, 130, 4096)


def top_bit(n_colors):
    """(the last word's index, its top valid bit)"""
    return words_of(n_colors) - 1, np.uint64(1) << np.uint64((n_colors - 1) & 63)


def matrices(rng, n, n_colors):
    """{name: uint64[n, W]}: all rows empty, all equal, all distinct, rows that differ only in the last word's top valid bit, rows that differ only in word 0"""
    W = words_of(n_colors)
    lw, tb = top_bit(n_colors)
    out = {"empty": np.zeros((n, W), dtype=np.uint64)}
    one = random_matrix(rng, 40, n_colors)
    one = one[one.any(axis=1)][:1]
    out["equal"] = np.repeat(one, n, axis=0)
    if n_colors >= 9:       # (2^9 > 300 rows: a counter in the low bits of word 0 makes every row another one, none empty)
        d = np.repeat(one, n, axis=0)
        d[:, 0] = (d[:, 0] & ~np.uint64(0x1FF)) | (np.arange(n, dtype=np.uint64) + np.uint64(1))
        out["distinct"] = d
        w0 = np.array(d)
        w0[:, 1:] = one[0, 1:]
        out["word 0 only"] = w0
    base = np.repeat(one, n, axis=0)
    base[:, lw] &= ~tb
    if n_colors > 1:
        base[:, 0] |= np.uint64(1)          # (never empty without the top bit)
    base[::2, lw] |= tb
    out["top bit only"] = base
    out["random with duplicates"] = random_matrix(rng, max(n, 40), n_colors)[np.r_[np.arange(n), rng.integers(0, max(n, 1), n // 2)].astype(np.int64)]
    return out


def canonical_of(bits):
    """numpy's statement: (set_of, sets) with sets[1:] = np.unique(axis=0) of the non-empty rows"""
    bits = np.asarray(bits, dtype=np.uint64)
    ne = bits.any(axis=1) if len(bits) else np.zeros(0, dtype=bool)
    sets = np.zeros((1, bits.shape[1]), dtype=np.uint64)
    set_of = np.zeros(len(bits), dtype=np.uint32)
    if ne.any():
        uniq, inv = np.unique(bits[ne], axis=0, return_inverse=True)
        sets = np.concatenate([sets, uniq])
        set_of[ne] = inv.reshape(-1).astype(np.uint32) + 1
    return set_of, sets


@pytest.mark.parametrize("n_colors", N_COLORS)
@pytest.mark.parametrize("n", [0, 1, 300])
def test_the_twin_is_np_unique(n, n_colors):
    rng = np.random.default_rng(3800 + n_colors + n)
    for name, bits in matrices(rng, n, n_colors).items():
        what = "%s, %d rows, %d colours" % (name, len(bits), n_colors)
        want_of, want_sets = canonical_of(bits)
        for threads in (1, 8):
            set_of, sets = fa.unitig_color_sets(bits, n_colors, n_threads=threads)
            assert set_of.dtype == np.uint32 and sets.dtype == np.uint64 and sets.shape == want_sets.shape, what
            assert np.array_equal(sets, want_sets) and np.array_equal(set_of, want_of), what
        assert not sets[0].any() and (len(sets) == 1 or sets[1:].any(axis=1).all()), what
        # the canonical order: ascending by word 0, then word 1, ...
        for a, b in zip(sets[1:-1].tolist(), sets[2:].tolist()):
            assert a < b, what
        assert np.array_equal(sets[set_of], bits) if len(bits) else len(set_of) == 0, what
        assert np.array_equal(fa.color_sets_expand(set_of, sets, n_colors), bits), what
    if n == 300:
        lw, tb = top_bit(n_colors)
        # (one colour: the row without its top bit is the empty one)
        assert len(canonical_of(matrices(rng, n, n_colors)["top bit only"])[1]) == (3 if n_colors > 1 else 2)
        assert len(canonical_of(matrices(rng, n, n_colors)["equal"])[1]) == 2


def raw_sets(bits, n_colors, cap):
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    set_of = np.zeros(max(len(bits), 1), dtype=np.uint32)
    sets = np.zeros((max(cap, 1), bits.shape[1]), dtype=np.uint64)
    n = C.c_uint64(99)
    rc = fa.lib().fin_unitig_color_sets(bits.ctypes.data_as(C.POINTER(C.c_uint64)), len(bits), n_colors, set_of.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        sets.ctypes.data_as(C.POINTER(C.c_uint64)), cap, C.byref(n), 2)
    return rc, int(n.value)


def test_refusals():
    rng = np.random.default_rng(3838)
    bits = random_matrix(rng, 200, 70)
    n_sets = len(canonical_of(bits)[1]) - 1
    assert raw_sets(bits, 70, n_sets + 1) == (0, n_sets)
    assert raw_sets(bits, 70, n_sets) == (fa.FIN_ELIMIT, n_sets)      # one row too few; the count is still reported
    assert raw_sets(bits, 0, n_sets + 1)[0] == fa.FIN_ELIMIT and raw_sets(np.zeros((2, 65), np.uint64), 4097, 3)[0] == fa.FIN_ELIMIT
    bad = np.array(bits); bad[17, 1] |= np.uint64(1) << np.uint64(6)   # colour 70 of 70
    assert raw_sets(bad, 70, n_sets + 2)[0] == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:
        fa.unitig_color_sets(bad, 70)
    assert e.value.code == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:
        fa.unitig_color_sets(bits, 4097)
    assert e.value.code == fa.FIN_ELIMIT
    set_of, sets = fa.unitig_color_sets(bits, 70)
    for so, st in ((np.where(np.arange(200) == 5, n_sets + 1, set_of), sets), (set_of, np.where(np.arange(len(sets))[:, None] == 0, 1, sets)), (set_of, sets | (np.uint64(1) << np.uint64(63)))):
        with pytest.raises(fa.FinitoError) as e:
            fa.color_sets_expand(so.astype(np.uint32), st.astype(np.uint64), 70)
        assert e.value.code == fa.FIN_EINVAL


def test_duplicate_and_unused_sets_expand_to_the_same_rows():
    rng = np.random.default_rng(3839)
    bits = random_matrix(rng, 100, 130)
    set_of, sets = fa.unitig_color_sets(bits, 130)
    more = np.concatenate([sets, sets[1:], np.full((2, 3), 1, dtype=np.uint64)])   # every set twice, two that nobody uses
    moved = np.where((np.arange(100) % 2 == 0) & (set_of > 0), set_of + (len(sets) - 1), set_of).astype(np.uint32)
    assert np.array_equal(fa.color_sets_expand(moved, more, 130), bits)
