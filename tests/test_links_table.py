"""The link table where probes wrap and tables are small (include/finito_amd.h: LINKS -- cap = max(4, the smallest power of two >= 2 * max_links), home slot
fin_link_hash(key) & (cap - 1), linear probing; fin_links.hip).  Keys are aimed with fa.link_hash; the expectation is tests/test_links_host.py's Model over the
hand-made pairs; every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import finito_amd as fa
from tests.test_links import batch_of, table_in_hbm
from tests.test_links_host import Model, assert_table
from tests.util import cut_unitigs, random_genome

pytestmark = pytest.mark.gpu

K = 31


@pytest.fixture(scope="module")
def wide():
    rng = np.random.default_rng(4295)
    g = random_genome(rng, 12000)
    p = fa.FinimizerIndex.build(cut_unitigs(rng, g, K, max_len=80), K).to_device(0)
    yield p, rng, p.export(fa.X_ENDS)
    p.close()


def keys_at(ends, cap, home, n, skip=0):
    """n keys (g_a, g_b), g_a + 1 < g_b, whose home slot in a table of cap slots is `home`"""
    total, out = int(ends[-1]), []
    for ga in range(skip, total):
        for gb in range(ga + 2, min(ga + 40, total)):
            if fa.link_hash((ga << 32) | gb) & (cap - 1) == home:
                out.append((ga, gb))
                if len(out) == n:
                    return out
                break
    raise AssertionError("not enough keys")


def reads_of(m0, keys, times=1):
    """one read of two slots per key and time: the slot before at the key's lower place, the slot at its higher place (named as the model names a place)"""
    return [("scan", [m0.end_of(ga), m0.end_of(gb)]) for ga, gb in keys for _ in range(times)]


def run_case(p, rng, ends, a, reads, what, expect_keys=None):
    b, pairs, nks = batch_of(p, rng, reads, K, 1)
    m = Model(pairs, nks, ends)
    if expect_keys is not None:
        assert sorted(m.counts) == sorted(expect_keys), what
    a.add(b)
    b.close()
    return m


@pytest.mark.parametrize("max_links,cap", [(1, 4), (2, 4), (3, 8), (8, 16)])
def test_small_tables_wrap_fill_and_refuse(wide, max_links, cap):
    p, rng, ends = wide
    m0 = Model([], [], ends)
    a = p.links(max_links)
    assert a.capacity == cap
    # keys whose home slot is the last one: the probe wraps
    keys = keys_at(ends, cap, cap - 1, max_links)
    m = run_case(p, rng, ends, a, reads_of(m0, keys, 3), "home slot cap - 1", keys)
    assert_table(a.download(), m, "max_links %d: %d keys at home slot %d" % (max_links, max_links, cap - 1))
    assert all(c == 3 for c in m.counts.values())
    # keys that all share one home slot, exactly max_links of them: downloads
    keys = keys_at(ends, cap, 1, max_links, skip=100)
    m = run_case(p, rng, ends, a.reset(), reads_of(m0, keys, 2), "one home slot", keys)
    assert_table(a.download(), m, "max_links %d: one home slot" % max_links)
    # one more key: FIN_ELIMIT from every download until the reset
    extra = keys_at(ends, cap, 2, 1, skip=300)
    run_case(p, rng, ends, a, reads_of(m0, extra), "one key too many", extra)
    for _ in range(2):
        with pytest.raises(fa.FinitoError) as e:
            a.download()
        assert e.value.code == fa.FIN_ELIMIT and "max_links" in str(e.value)
    assert table_in_hbm(a)[1] == max_links + 1
    # ... and more keys than the table has slots: no probe finds room, nothing hangs
    many = [key for h in range(cap) for key in keys_at(ends, cap, h, 1, skip=500)] + keys_at(ends, cap, 0, 2, skip=700)
    run_case(p, rng, ends, a.reset(), reads_of(m0, many), "more keys than slots")
    with pytest.raises(fa.FinitoError) as e:
        a.download()
    assert e.value.code == fa.FIN_ELIMIT
    assert len(table_in_hbm(a)[0]) == cap
    # the object works again after the reset
    m = run_case(p, rng, ends, a.reset(), reads_of(m0, keys), "after the reset", keys)
    assert_table(a.download(), m, "max_links %d: after the reset" % max_links)
    a.close()


def test_one_hot_key_counts_every_transition(wide):
    """300 reads of 129 slots that alternate between two places: one key, 300 * 128 adds to one slot from many waves"""
    p, rng, ends = wide
    m0 = Model([], [], ends)
    P, Q = m0.end_of(1000), m0.end_of(5000)
    a = p.links(1)
    m = run_case(p, rng, ends, a, [("scan", [P if i % 2 == 0 else Q for i in range(129)])] * 300, "one hot key", [(1000, 5000)])
    assert m.counts == {(1000, 5000): 300 * 128}
    assert_table(a.download(), m, "one hot key")
    assert a.download().links["count"].tolist() == [300 * 128]
    a.close()


def test_min_count_two_adds_and_merged_downloads(wide):
    p, rng, ends = wide
    m0 = Model([], [], ends)
    keys = keys_at(ends, 64, 63, 6) + keys_at(ends, 64, 0, 6, skip=200) + keys_at(ends, 64, 17, 6, skip=400)
    first = [r for i, key in enumerate(keys[:12]) for r in reads_of(m0, [key], 1 + i % 4)]
    second = [r for i, key in enumerate(keys[6:]) for r in reads_of(m0, [key], 1 + i % 3)]
    a, a1, a2 = p.links(32), p.links(32), p.links(32)
    assert a.capacity == 64
    m_both = run_case(p, rng, ends, a, first + second, "both in one add")
    m1, m2 = run_case(p, rng, ends, a1, first, "the first"), run_case(p, rng, ends, a2, second, "the second")
    assert m_both.n_distinct == 18 and m1.n_distinct == 12 and m2.n_distinct == 12 and max(m_both.counts.values()) >= 6
    for mc in (1, 2, 3, 5, 100):
        assert_table(a.download(mc), m_both, "min_count %d" % mc, mc)
    assert len(m_both.table(3)) not in (0, 18)
    # cap_out one too small under a min_count: FIN_ELIMIT with the true number
    L, err, n = fa.lib(), C.create_string_buffer(512), C.c_uint64(0)
    kept = len(m_both.table(3))
    out = np.zeros(3 * kept, dtype=np.uint64)
    assert L.fin_links_download(a.h, 3, out.ctypes.data_as(C.c_void_p), kept - 1, C.byref(n), None, err, 512) == fa.FIN_ELIMIT and n.value == kept
    assert not out.any()
    # two adds equal one add of the concatenated reads
    run_case(p, rng, ends, a1, second, "the second behind the first")
    assert_table(a1.download(), m_both, "two adds")
    # the downloads of two accumulators, merged
    run_case(p, rng, ends, a1.reset(), first, "the first again")
    assert_table(fa.links_merge(a1.download(), a2.download()), m_both, "links_merge")
    for x in (a, a1, a2):
        x.close()
