"""Shared tags in the compact k-mer table (fin_format.h: FinDevIndex::kt3), fed to the search on purpose.

A slot of the table is {answer g, 30-bit tag}: a tag match is a claim that the text at g must prove, and when two different k-mers share bucket chain and tag the
comparison fails and kernel 3 decides.  By chance that happens once in 2^30 slots looked at, so no other test reaches the branches that implement the rule:
kt3_find_h / pp_claim_holds / the fast path's whole-read comparison / the probe item that meets the claim again (fin_prepass.hip), W_KF1 -> W_RES4 | W_KFV ->
give_up, the wide keys' kt_claim, the lean second look-up of an epoch, W_KFX (fin_kernel_w.hip).  fin_mix64 has an inverse, so colliders are COMPUTED here
(tests/util.py: colliders_of; tests/test_kmer_table_collisions_host.py holds the restatement against the header and asserts what every case presupposes):
for a k-mer y of the index, the k-mers x whose hash differs from y's in bits 30 and 31 only -- same bucket for any table size, same tag.

Scenarios (tests/util.py: collision_case), at k = 31, 32, 63, 64, at k = 100 and 127 (also with lean_tables 3 + fast_path 2), and 1-3 at k = 200:
  1  an absent collider of a verified victim as a read's first, last and middle k-mer (the three the pre-pass looks at), spliced between two matching stretches,
     as the whole read, twice in one read; each also reverse-complemented
  2  the same for victims at the first and the last k-mer of the text, a unitig's first and last k-mer, and (k = 31) a place inside one 64-base text window and
     one across two
  3  the collider is in the index too (one; from k = 32 on also all three: four entries of one tag in one chain): reads along, from and up to every member
  4  (k = 31) the collider inside a run of absent k-mers all of whose strings occur, 0 .. 3 absent k-mers in front of it; lean_walk 1 and 0
  5  an unverified victim (a set with duplicated stretches): an absent collider (a miss in the exact side table) and a present one
Every expectation is the faithful oracle's (merged and forward-only), compared exactly; for k <= 64 the table is asked first (kmer_table_query) whether the
inputs are what they claim.  Not covered: a collider a base or two from its victim (inverting the hash gives no control over the distance), k < 31,
partitioned indexes.

That the branches ran is shown by what a run gives up to the kernel behind the walk kernel (kernel_3_list below): every batch has a CONTROL batch -- the same reads
with every member of a tag group replaced by control_of (same bucket, another tag) --, and under kernel 4 with the table on the collider batch must leave strictly
more.  give_up, where every failed claim ends, fills the walk kernel's read list: for k <= 128 that is kernel 3's list, counted by fin_batch_pipeline_counts [2]
(fin_batch_overflow_reads, the deque-overflow list, was 0 in every such batch); for k > 128 it is the overflow list itself, which the plain kernel works off, so
there fin_batch_overflow_reads carries the figure and [2] is 0 (measured at k = 200).  Either way a wave takes its slots 64 at a time: the figure moves in steps
of 64 and says nothing per read.  The per-read bound of scenario 1 -- every read that BEGINS with an absent collider is given up -- is therefore checked with each such
read as a batch of its own (reads_given_up).

A look-up comes behind probes that passed, and a constructed k-mer is a random one: with bare colliders the list stayed EMPTY in scenario 1 at k = 31, 32 and 100 and
in scenario 2 at k = 31, 32, 64 and 100 -- the string filters settled them absent.  So every absent collider and every control k-mer has all its strings of k - 1
bases in the index (tests/util.py: _support; asserted on the CPU): both reach the same bucket and differ by the tag alone.  This makes the indexes larger than the
few kb of a bare genome (up to 28.6 kb at k = 200), and a read that splices a k-mer between two matching stretches has more than 3 k bases (644 at k = 200).

Measured on an MI355X, slots collider batch / control batch, defaults (fast_path 0 where it differs in brackets):

  k      scenario 1   scenario 2   scenario 3        scenario 4   scenario 5
  31     512 / 0      192 / 0      64 / 0 (128 / 0)  256 / 0      192 / 0
  32     576 / 0      320 / 0      64 / 0 (128 / 0)  -            192 / 0
  63     576 / 0      320 / 0      64 / 0 (128 / 0)  -            128 / 0 (192 / 0)
  64     576 / 0      320 / 0      128 / 0           -            192 / 0
  100    576 / 0      320 / 0      128 / 0           -            192 / 64
  127    576 / 0      320 / 0      128 / 0           -            192 / 64
  200    576 / 0      320 / 0      128 / 0           -            -
  scenario 4 with lean_walk 0: 256 / 0, fast path on and off.  lean_tables 3 + fast_path 2 at k = 100 and 127: 576 / 0, 320 / 0, 64 / 0, and scenario 5 128 / 64 (k = 100)
  and 192 / 64 (k = 127).  Scenario 1's reads that begin with an absent collider, one batch each, given up collider / control: 20 / 0 of 20 at k = 31, 24 / 0 of 24 at
  every other k.  (Scenario 5's control leaves 64 at k = 100 and 127 only: supposedly the unverified k-mers beside the victims in a set with duplicated stretches --
  a wide key's unverified claim is given up whoever makes it, W_KF1 verdict 2; not traced further.)
"""
import contextlib

import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import format_pairs
from tests.util import COLLISION_KS, collision_case, collision_scenarios

pytestmark = pytest.mark.gpu

CASES = [(k, s) for k in COLLISION_KS for s in collision_scenarios(k)]
_INDEXES = {}


@pytest.fixture(scope="module", autouse=True)
def uploaded_indexes():
    """a case's index is uploaded once per setting of the upload-time options and shared by the tests of this module"""
    yield
    for p in _INDEXES.values():
        p.close()
    _INDEXES.clear()


def index_of(c, **at_upload):
    key = (c.k, c.scenario) + tuple(sorted(at_upload.items()))
    if key not in _INDEXES:
        p = fa.FinimizerIndex.build(list(c.unitigs), c.k)
        for name, value in at_upload.items():
            p.set_option(name, value)
        _INDEXES[key] = p.to_device(0)
    return _INDEXES[key]


@contextlib.contextmanager
def options(p, **kv):
    """this handle's own values of run-time options; afterwards the handle follows the process-wide values again, whatever they are (the library has no getter for
    those, so they are not touched)"""
    try:
        for name, value in kv.items():
            p.set_option(name, value)
        yield
    finally:
        for name in kv:
            p.set_option(name, None)


def expected_text(c, name):
    if ("text", name) not in c.expected:
        merged = c.expected[name][0]
        rd = c.reads if name == "reads" else c.control_reads
        at = np.concatenate([[0], np.cumsum([len(r) - c.k + 1 for r in rd])])
        c.expected[("text", name)] = "".join(format_pairs(merged[at[i]:at[i + 1]]) for i in range(len(rd))).encode()
    return c.expected[("text", name)]


def kernel_3_list(b):
    """what the last run of the batch gave up to the kernel behind the walk kernel, where every failed claim ends (fin_kernel_w.hip: give_up).  k <= 128: the slots of
    kernel 3's read list (fin_batch_pipeline_counts [2]: a wave takes them 64 at a time, some stay empty; fin_batch_overflow_reads, the deque-overflow list, stays 0).
    k > 128: the walk kernel's list IS the overflow list, which the plain kernel works off: fin_batch_overflow_reads counts its entries one by one, and [2] stays 0.
    The sum serves both"""
    return b.pipeline_counts(48)[2] + b.overflow_reads()


def reads_given_up(p, reads):
    """how many of these reads, each run as a batch of its own, leave anything to the kernel behind the walk kernel: a count per read, which the slots of a whole batch
    (64 per wave) cannot give"""
    n = 0
    for r in reads:
        b = p.batch([r])
        try:
            b.run(fa.FIN_MERGED)
            n += kernel_3_list(b) > 0
        finally:
            b.close()
    return n


def run_and_compare(c, p, name="reads", mode=0, what=""):
    """the batch `name` of the case, merged, in text mode `mode`, against the oracle: the pairs (modes 0 and 1), the text (modes 1 and 2).  Returns what the run left
    to kernel 3 (kernel_3_list) and what it decided"""
    rd = c.reads if name == "reads" else c.control_reads
    merged = c.expected[name][0]
    b = p.batch(rd)
    try:
        b.text_mode(mode)
        b.run(fa.FIN_MERGED)
        if mode < 2:
            got, npos = b.download()
            bad = np.nonzero((got.astype(np.int64) != merged).any(axis=1))[0]
            assert len(bad) == 0, "k=%d scenario %d %s %s: %d pairs differ from the oracle's, the first at %d: %s, oracle %s" % (
                c.k, c.scenario, name, what, len(bad), bad[0], got[bad[0]].tolist(), merged[bad[0]].tolist())
            assert npos == int((merged[:, 0] >= 0).sum())
        if mode > 0:
            assert b.text() == expected_text(c, name), "k=%d scenario %d %s %s: the text of mode %d differs from the oracle's" % (c.k, c.scenario, name, what, mode)
        return kernel_3_list(b), b.run_info()
    finally:
        b.close()


def compare_forward(c, p, what=""):
    for name, rd in (("reads", c.reads), ("control", c.control_reads)):
        got, _ = p.search_reads(rd, fa.FIN_FWD)
        assert np.array_equal(got.astype(np.int64), c.expected[name][1]), "k=%d scenario %d %s %s: forward-only pairs differ from the oracle's" % (c.k, c.scenario, name, what)


def assert_inputs_are_what_they_claim(c, p):
    """k <= 64, the table asked directly: every collider is claimed with its victim's g; an absent collider's claim has no proof (flag 4 clear), of the members of a
    group that are in the index exactly one is borne out (a verified claim whose text spells it, or an unverified one the exact side table holds); no control k-mer
    is claimed"""
    for v, cs in c.groups:
        g, fl = p.kmer_table_query([v] + cs)
        assert (fl & 3).all(), "a member of a tag group the table does not claim: %s %s" % (v, fl.tolist())
        assert (g == g[0]).all(), "a collider claimed at another place than its victim: %s %s" % (v, g.tolist())
        inside = [i for i, m in enumerate([v] + cs) if i == 0 or m in c.present]
        borne_out = [i for i in inside if (fl[i] & 1 and fl[i] & 4) or (fl[i] & 2 and fl[i] & 8)]
        assert len(borne_out) == 1, (v, fl.tolist())
        assert int(g[0]) == c.answers[([v] + cs)[borne_out[0]]][0]
        if len(inside) == 1:
            assert bool(fl[0] & 2) == (c.scenario == 5) and bool(fl[0] & 1) == (c.scenario != 5)
        for i, m in enumerate([v] + cs):
            if i not in inside:
                assert not fl[i] & 4 and not fl[i] & 8, "an absent collider, proven present: %s" % m
    for name, e in c.where.items():
        assert int(p.kmer_table_query([c.text[e - c.k + 1:e + 1]])[0][0]) == e, name
    if c.control:
        _, fl = p.kmer_table_query(list(c.control.values()))
        assert not (fl & 3).any(), "a control k-mer is claimed"


@pytest.mark.parametrize("k,scenario", CASES)
def test_scenario(k, scenario):
    """the scenario under the defaults and with the fast path off (k = 100, 127: also lean tables + the fast path above 63; scenario 4: also lean_walk 0), merged and
    forward-only, collider and control batch; and the proof that the shared tags were met: kernel 3's list grows against the control batch"""
    c = collision_case(k, scenario)
    p = index_of(c)
    assert p.kmer_table_bytes() > 0
    if k <= 64:
        assert_inputs_are_what_they_claim(c, p)
    n_col, info = run_and_compare(c, p, "reads", what="defaults")
    n_ctl, _ = run_and_compare(c, p, "control", what="defaults")
    assert info["kernel"] == 4
    print("COUNTS k=%d scenario %d: %d / %d" % (k, scenario, n_col, n_ctl))
    compare_forward(c, p, "defaults")
    with options(p, fast_path=0):
        n_col0, _ = run_and_compare(c, p, "reads", what="fast_path 0")
        n_ctl0, _ = run_and_compare(c, p, "control", what="fast_path 0")
        print("COUNTS k=%d scenario %d fast_path 0: %d / %d" % (k, scenario, n_col0, n_ctl0))
        compare_forward(c, p, "fast_path 0")
    if scenario == 4:
        with options(p, lean_walk=0):
            for fast in (1, 0):
                with options(p, fast_path=fast):
                    n2, _ = run_and_compare(c, p, "reads", what="lean_walk 0 fast_path %d" % fast)
                    m2, _ = run_and_compare(c, p, "control", what="lean_walk 0 fast_path %d" % fast)
                    print("COUNTS k=%d scenario %d lean_walk 0 fast_path %d: %d / %d" % (k, scenario, fast, n2, m2))
                    assert n2 > m2
    if k in (100, 127):
        pl = index_of(c, lean_tables=3)
        assert pl.lean_tables()
        with options(pl, fast_path=2):
            nl, infl = run_and_compare(c, pl, "reads", what="lean_tables 3 fast_path 2")
            ml, _ = run_and_compare(c, pl, "control", what="lean_tables 3 fast_path 2")
            assert infl["fast_path"]
            print("COUNTS k=%d scenario %d lean_tables 3 fast_path 2: %d / %d" % (k, scenario, nl, ml))
            compare_forward(c, pl, "lean_tables 3 fast_path 2")
            assert nl > ml
    assert n_col > n_ctl, "the collider batch sends no more reads to kernel 3 than its control: the shared tags were not met (%d / %d)" % (n_col, n_ctl)
    assert n_col0 > n_ctl0, "fast_path 0: the shared tags were not met (%d / %d)" % (n_col0, n_ctl0)
    if scenario == 1:   # a read that BEGINS with an absent collider: the pre-pass's look claims it, the walk kernel's look-up meets the claim again and gives the read up
        first_col = reads_given_up(p, [c.reads[i] for i in c.first_reads]); first_ctl = reads_given_up(p, [c.control_reads[i] for i in c.first_reads])
        print("COUNTS k=%d scenario 1, reads that begin with a collider, one batch each: %d / %d of %d" % (k, first_col, first_ctl, len(c.first_reads)))
        assert first_col >= len(c.first_reads) - first_ctl, (first_col, first_ctl, len(c.first_reads))


@pytest.mark.parametrize("lean_tables", (None, 0), ids=("lean_default", "lean_tables_0"))
@pytest.mark.parametrize("kmer_table", (1, 0), ids=("table", "no_table"))
@pytest.mark.parametrize("k", (31, 63))
def test_scenario_1_under_every_option(k, kmer_table, lean_tables):
    """scenario 1 with fast_path {0, 1} x defer_strand {0, 1} x the three text modes, on replicas uploaded with lean_tables {default, 0} x kmer_table {1, 0} (0: the
    answer no table has a part in).  In text modes 1 and 2 the text is made from the fast path's records: a read that carries an absent collider where the pre-pass
    looks must not come back as a finished record whose expansion differs from the oracle's line"""
    c = collision_case(k, 1)
    at_upload = {}
    if lean_tables is not None:
        at_upload["lean_tables"] = lean_tables
    if not kmer_table:
        at_upload["kmer_table"] = 0
    p = index_of(c, **at_upload)
    assert (p.kmer_table_bytes() > 0) == bool(kmer_table)
    for fast in (1, 0):
        for defer in (1, 0):
            with options(p, fast_path=fast, defer_strand=defer):
                for mode in (0, 1, 2):
                    for name in ("reads", "control"):
                        run_and_compare(c, p, name, mode=mode, what="fast_path %d defer_strand %d lean_tables %s kmer_table %d" % (fast, defer, lean_tables, kmer_table))


@pytest.mark.parametrize("kernel", (3, 2, 0), ids=("v3", "v2", "plain"))
@pytest.mark.parametrize("k", COLLISION_KS)
def test_scenarios_on_the_other_kernels(k, kernel):
    """every scenario once on the lazy-streaming, the streaming and the plain kernel (k = 200: kernels 3 and 2 cannot run, the option falls back to the plain one)"""
    for scenario in collision_scenarios(k):
        c = collision_case(k, scenario)
        p = index_of(c)
        with options(p, kernel=kernel):
            _, info = run_and_compare(c, p, "reads", what="kernel %d" % kernel)
            assert info["kernel"] == (kernel if k <= 128 else 0)
            compare_forward(c, p, "kernel %d" % kernel)
