"""The equivalence-class table (fin_eqclasses.hip) where probes wrap and tables are small, on the device.  The cases are
tests/test_eqclasses_table_host.py::all_cases(), chosen with a Python mirror of the table's hash arithmetic and proven there to have their properties: claim
probes and serial windows that cross the table's end, tables smaller than the serial pass's window, the limit met in the serial pass, collision lists of 1 to
n_rows entries.  Every download is compared with np.unique's classes (classes_of_rows), exact; the mirror's model is never an expectation of a download.  It is
the expectation of stats()[3], the rows through the serial pass, wherever a case's first add holds one row per tag -- which also proves that the guards hold
for the device's table and not only for the model's."""
import numpy as np
import pytest

import finito_amd as fa
from tests.test_eqclasses import assert_all, on_device
from tests.test_eqclasses_host import assert_classes, classes_of_rows
from tests.test_eqclasses_table_host import M64, all_cases, cases_of, tags_of
from tests.util import cut_unitigs, random_genome

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(2390)
    k = 31
    p = fa.FinimizerIndex.build(cut_unitigs(rng, random_genome(rng, 12000), k, max_len=80), k).to_device(0)
    yield p
    p.close()


def run_adds(p, max_classes, tag_bits, W, adds, combine, what, serial_after=None):
    """the adds in turn in a fresh accumulator, each followed by the comparison with np.unique over everything added so far (and, with serial_after, of
    stats()[3] with the model's figure).  What every step downloaded and counted comes back"""
    n_colors = 64 * W
    col = p.colors(n_colors)
    seen = []
    p.set_option("ec_tag_bits", tag_bits); p.set_option("ec_combine", combine)
    try:
        eq = col.eqclasses(max_classes)
        kept = [on_device(a) for a in adds]           # alive until the last download has waited for the adds
        for i, (a, t) in enumerate(zip(adds, kept)):
            eq.add_rows(t.data_ptr(), len(a))
            sofar = np.concatenate(adds[: i + 1])
            step = "%s, ec_combine %d, add %d of %d" % (what, combine, i + 1, len(adds))
            assert_all(eq, classes_of_rows(sofar, n_colors), n_colors, step, n_rows=len(sofar))
            st = eq.stats()
            if serial_after is not None:
                assert st[3] == serial_after[i], "%s: %d rows through the serial pass, the model has %d" % (step, st[3], serial_after[i])
            seen.append((eq.download(), st if serial_after is not None else st[:3]))
        eq.close()
    finally:
        p.set_option("ec_tag_bits", None); p.set_option("ec_combine", None)
        col.close()
    return seen


def assert_same(a, b, what):
    """two runs of the same adds: the downloads and stats of every step"""
    assert len(a) == len(b)
    for (da, sa), (db, sb) in zip(a, b):
        assert_classes(da, db, what)
        assert sa == sb, "%s: stats %s and %s" % (what, sa, sb)


def run_case(p, case):
    """under ec_combine 1 and 0: the same downloads and stats (case 5)"""
    serial = case.serial_after() if case.owners_fixed else None
    both = [run_adds(p, case.max_classes, case.tag_bits, case.W, case.adds, combine, case.name, serial) for combine in (1, 0)]
    assert_same(both[0], both[1], case.name + ", ec_combine 1 against 0")
    return both[0]


# ---- 1. the claim pass across the table's end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases_of("claim_wrap"), ids=repr)
def test_claims_across_the_end_of_the_table(small, case):
    seen = run_case(small, case)
    assert all(st[3] == 0 for _, st in seen)


# ---- 2. the serial pass across the table's end -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases_of("serial_wrap"), ids=repr)
def test_serial_windows_across_the_end_of_the_table(small, case):
    run_case(small, case)


# ---- 3. tables smaller than a window ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases_of("small"), ids=repr)
def test_tables_smaller_than_the_serial_window(small, case):
    run_case(small, case)


# ---- 4. the serial pass's own limit ----------------------------------------------------------------------------------------------------------
def refuses(eq, max_classes):
    for _ in range(2):
        with pytest.raises(fa.FinitoError) as e:
            eq.download()
        assert e.value.code == fa.FIN_ELIMIT and "max_classes = %d;" % max_classes in str(e.value)


@pytest.mark.parametrize("lc", all_cases()[1], ids=lambda lc: lc["name"])
def test_the_limit_met_in_the_serial_pass(small, lc):
    p, mc, W = small, lc["max_classes"], lc["W"]
    n_colors = 64 * W
    col = p.colors(n_colors)
    owner, good, over, extra = (on_device(lc[x]) for x in ("owner", "good", "over", "extra"))
    both = np.concatenate([lc["owner"], lc["good"]])
    want = classes_of_rows(both, n_colors)
    assert len(want[0]) == mc
    p.set_option("ec_tag_bits", 1)
    try:
        eq = col.eqclasses(mc)
        eq.add_rows(owner.data_ptr(), 1).add_rows(good.data_ptr(), len(good))
        assert_all(eq, want, n_colors, lc["name"] + ": exactly max_classes distinct rows", n_rows=len(both))
        serial = eq.stats()[3]
        assert serial == sum(1 for r in lc["good"] if r.tobytes() != lc["owner"][0].tobytes())
        eq.add_rows(extra.data_ptr(), 1)                 # one more class under the same tag, in a later add: the serial pass finds it
        assert eq.stats()[2:] == [mc + 1, serial + 1]
        refuses(eq, mc)
        eq.reset().add_rows(owner.data_ptr(), 1).add_rows(over.data_ptr(), len(over))   # ... and in the same add
        assert eq.stats()[2:] == [mc + 1, serial + 1]
        refuses(eq, mc)
        eq.reset().add_rows(owner.data_ptr(), 1).add_rows(good.data_ptr(), len(good))
        assert_all(eq, want, n_colors, lc["name"] + ": a good add after the reset", n_rows=len(both))
        assert eq.stats()[3] == serial
        eq.close()
    finally:
        p.set_option("ec_tag_bits", None)
        col.close()


# ---- 5. ec_combine = 0: cases 1 to 3 run under both settings (run_case), and these waves -------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2])
def test_waves_with_and_without_combined_adds(small, W):
    rng = np.random.default_rng(2350 + W)
    pool = np.unique(rng.integers(1, M64, size=(66, W), dtype=np.uint64, endpoint=True), axis=0)
    assert len(pool) == 66 and len(np.unique(tags_of(pool, 63))) == 66
    zero = np.zeros(W, dtype=np.uint64)
    waves = {"64 equal rows": pool[[0] * 64], "63 equal rows and one other": pool[[1] * 37 + [2] + [1] * 26], "64 distinct rows": pool[2:66],
             "rows alternating with empty rows": np.array([zero if i % 2 else pool[i % 6] for i in range(192)])}
    for name, rows in waves.items():
        both = [run_adds(small, 1024, 63, W, [rows], combine, "W=%d, %s" % (W, name), [0]) for combine in (1, 0)]
        assert_same(both[0], both[1], name)
    both = [run_adds(small, 1024, 63, W, list(waves.values()), combine, "W=%d, the waves one after the other" % W, [0] * 4) for combine in (1, 0)]
    assert_same(both[0], both[1], "the waves one after the other")


# ---- 6. the collision list at its bounds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases_of("list"), ids=repr)
def test_collision_lists_of_one_row_to_every_row(small, case):
    seen = run_adds(small, case.max_classes, case.tag_bits, case.W, case.adds, 1, case.name, case.serial_after())
    assert seen[-1][1][3] == case.n


# ---- 7. the download's compaction past one block per scan thread -------------------------------------------------------------------------------
@pytest.mark.parametrize("W, n_classes, n_rows", [(1, 3000, 9000), (1, 150000, 300000), (2, 3000, 9000)])
def test_compaction_of_a_table_of_2048_blocks(small, W, n_classes, n_rows):
    rng = np.random.default_rng(2370 + W + n_classes)
    pool = np.unique(rng.integers(1, M64, size=(n_classes, W), dtype=np.uint64, endpoint=True), axis=0)
    assert len(pool) == n_classes and len(np.unique(tags_of(pool, 63))) == n_classes   # no two rows share a full-width tag: nothing for the serial pass
    rows = pool[np.concatenate([np.arange(n_classes), rng.integers(0, n_classes, n_rows - n_classes)])][rng.permutation(n_rows)]
    seen = run_adds(small, 1 << 18, 63, W, [rows], 1, "2^19 slots, W=%d, %d classes" % (W, n_classes), [0])
    assert len(seen[0][0][0]) == n_classes
