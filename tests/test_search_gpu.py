"""Parity tests proper: the HIP path, called through the C ABI, against the CPU oracle and the reference's vectors."""
import os

import numpy as np
import pytest

import finito_amd as fa
from finito_amd import synth
from oracle.oracle import Counters, OracleIndex
from tests.util import DEFER_KAT, cut_unitigs, defer_family_case, mosaic_read, random_genome, rc, sample_reads

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=[4, 3, 2, 0], ids=["v4", "v3", "v2", "plain"])
def kernel(request):
    """every test runs on the kernel pipeline (4, the default), the lazy-streaming kernel (3), the streaming kernel (2) and the
    plain lane-per-read kernel (0)"""
    assert fa.lib().fin_set_option(b"kernel", request.param) == 0
    yield request.param
    fa.lib().fin_set_option(b"kernel", 4)


def both(unitigs, k):
    return fa.FinimizerIndex.build(unitigs, k).to_device(0), OracleIndex.build(unitigs, k)


def assert_reads_equal(p, o, reads):
    """merged (search_fmin.hh:47-60) and forward-only (FinimizerIndex::search) results, bit-exact"""
    got, npos = p.search_reads(reads, fa.FIN_MERGED)
    exp, _, _ = o.search_batch(reads)
    assert got.shape == exp.shape
    assert np.array_equal(got.astype(np.int64), exp), "merged results differ"
    assert npos == int((exp[:, 0] != -1).sum())
    gotf, _ = p.search_reads(reads, fa.FIN_FWD)
    strs = reads if isinstance(reads, list) else None
    if strs is not None:
        expf = [x for r in strs for x in o.search(r)[0]]
        assert gotf.tolist() == [list(x) for x in expf], "forward-only results differ"


@pytest.mark.parametrize("name", ["test_shortest_unique_queries", "test_finimizer_branch", "test_reverse_complement_branch",
                                  "test_leftmost", "test_incoming_rc_branch", "test_reverse_complement_query", "test_walk",
                                  "example_fna_k4"])
def test_reference_vectors_on_gpu(kat, name):
    c = next(x for x in kat if x["name"] == name)
    p = fa.FinimizerIndex.build(c["unitigs"], c["k"]).to_device(0)
    for q in c.get("queries", []):
        res = p.search(q["q"])
        if q.get("pairs_rank_of_query_unitig"):
            order = sorted(c["unitigs"], key=lambda s: s[:c["k"]][::-1])
            assert res.local_offsets == [(order.index(q["q"]), 0)]
        else:
            assert res.local_offsets == [tuple(x) for x in q["pairs"]]
        if "n_found" in q:
            assert res.n_found == q["n_found"]
    for q in c.get("merged_queries", []):
        got, _ = p.search_reads([q["q"]], fa.FIN_MERGED)
        assert got.tolist() == q["pairs"]


@pytest.mark.parametrize("k", [4, 7, 12, 21, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255])
def test_random_reads_vs_oracle(k):
    """(k > 128: LCS values no longer fit the node byte's 7 bits -- kernels 2 and 3 cannot run, the option falls back to the plain
    kernel; kernel 4 runs its pre-pass and walk kernel, which need no LCS, and sends what they cannot finish to the plain kernel)"""
    rng = np.random.default_rng(1000 + k)
    g = random_genome(rng, 20000)
    unitigs = cut_unitigs(rng, g, k, max_len=max(3 * k, 150))
    p, o = both(unitigs, k)
    reads = sample_reads(rng, g, 400, 150 if k < 60 else 250 if k < 129 else 600)
    if k > 128:
        reads += [mosaic_read(rng, g, k, 900) for _ in range(60)] + [g[:3000], rc(g[5000:6500])]
    assert_reads_equal(p, o, reads)


def test_edge_cases():
    k = 9
    rng = np.random.default_rng(3)
    g = random_genome(rng, 6000)
    unitigs = cut_unitigs(rng, g, k, max_len=90)
    p, o = both(unitigs, k)
    reads = ["", "A", g[10:10 + k - 1], g[100:100 + k], rc(g[200:200 + k]), g[300:420], g[500:560] + "N" + g[561:640],
             g[700:800].lower(), "N" * 30, "ACGT" * 20, g[:5000], "T" * 300, g[900:960] + "n" + g[1000:1050],
             rc(g[2000:2300]), g[1500:1500 + k] + "X"]
    assert_reads_equal(p, o, reads)
    # every read of the batch is ragged on purpose; also all-miss reads
    miss = [random_genome(rng, int(rng.integers(1, 200))) for _ in range(300)]
    assert_reads_equal(p, o, miss)


def test_reads_crossing_unitig_boundaries_and_queries_equal_unitigs():
    k = 15
    rng = np.random.default_rng(8)
    g = random_genome(rng, 30000)
    unitigs = cut_unitigs(rng, g, k, max_len=60)        # many short unitigs: every read crosses several
    p, o = both(unitigs, k)
    assert_reads_equal(p, o, sample_reads(rng, g, 300, 200, err=0.0, random_frac=0.0))
    assert_reads_equal(p, o, unitigs)                    # BASELINE config 1: queries = unitigs


@pytest.mark.parametrize("k", [6, 12, 20])
def test_repetitive_non_disjoint(k):
    """duplicate k-mers (walk semantics, tests.cpp:290-317), low complexity, long runs of growing candidates"""
    rng = np.random.default_rng(70 + k)
    base = random_genome(rng, 80)
    unitigs = []
    for _ in range(40):
        a = int(rng.integers(0, 60)); L = int(rng.integers(k, 70))
        unitigs.append((base + base)[a:a + L])
    unitigs += ["A" * (k + 9), "AC" * k, "ACG" * k, "T" * (k + 1)]
    p, o = both(unitigs, k)
    reads = [(base * 3)[int(rng.integers(0, 80)):][:int(rng.integers(k, 160))] for _ in range(200)]
    reads += ["A" * 100, "AC" * 60, "ACG" * 50, "T" * 40 + "A" * 40, rc(base * 2)]
    reads += sample_reads(rng, base * 3, 100, 90, err=0.05, random_frac=0.1)
    assert_reads_equal(p, o, reads)


def test_deque_overflow_path(monkeypatch):
    """Force the LDS-deque overflow re-run (global-memory deque) on every read and require identical output."""
    k = 31
    rng = np.random.default_rng(11)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    p, o = both(unitigs, k)
    reads = sample_reads(rng, g, 500, 150)
    L = fa.lib()
    assert L.fin_set_option(b"lds_deque_limit", 1) == 0
    try:
        assert_reads_equal(p, o, reads)
        # without seeds every strand goes through the streaming kernels and overflows there: under kernel 4 a read is pushed once per
        # strand item (and again by kernel 3's redo) -- the list has room for that and the count stays within its bound
        assert L.fin_set_option(b"seed_anchors", 0) == 0
        b = p.batch(reads)
        b.run(fa.FIN_MERGED)
        got, _ = b.download()
        n_ovf = b.overflow_reads()
        b.close()
        exp, _, _ = o.search_batch(reads)
        assert np.array_equal(got.astype(np.int64), exp)
        assert 0 < n_ovf <= 4 * len(reads) + 64
        # if the list ever overran (a push beyond its capacity is dropped on the device) the results are withheld, loudly
        assert L.fin_set_option(b"debug_ovf_cap", 3) == 0
        b = p.batch(reads)
        b.run(fa.FIN_MERGED)
        with pytest.raises(fa.FinitoError) as ei:
            b.download()
        assert ei.value.code == fa.FIN_ELIMIT and "overflow list" in str(ei.value)
        # ... by EVERY entry point that delivers results -- a range of pairs, the text
        with pytest.raises(fa.FinitoError) as ei:
            b.download_range(0, 10)
        assert ei.value.code == fa.FIN_ELIMIT and "overflow list" in str(ei.value)
        with pytest.raises(fa.FinitoError) as ei:
            b.text()
        assert ei.value.code == fa.FIN_ELIMIT and "overflow list" in str(ei.value)
        b.close()
        with pytest.raises(fa.FinitoError) as ei:
            p.search_reads_text([r for r in reads if len(r) >= k])
        assert ei.value.code == fa.FIN_ELIMIT
    finally:
        L.fin_set_option(b"lds_deque_limit", 16); L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"debug_ovf_cap", 0)


@pytest.mark.parametrize("k", [23, 150])
def test_epoch_budget_fallback(kernel, k):
    """The per-read epoch budget is what bounds any livelock of the tuned kernels: a read that runs out of it drops its requests
    in flight (cache tags of data that will never arrive must not survive) and is redone by the overflow kernel.  With the budget
    shrunk to about one epoch per base most reads take that way; results must not change.  (k = 150: beyond the streaming kernels'
    range -- kernel 4's walk kernel hands what it gives up straight to the plain kernel's list.)"""
    rng = np.random.default_rng(99)
    g = random_genome(rng, 30000)
    unitigs = cut_unitigs(rng, g, k, max_len=400 + 2 * k)
    p, o = both(unitigs, k)
    reads = [mosaic_read(rng, g, k, 400 + 3 * k) for _ in range(600)] + sample_reads(rng, g, 300, 150 + 2 * k)
    L = fa.lib()
    assert L.fin_set_option(b"epoch_budget_mult", 1) == 0 and L.fin_set_option(b"epoch_budget_add", 8) == 0
    try:
        b = p.batch(reads)
        b.run(fa.FIN_MERGED)
        got, npos = b.download()
        n_ovf = b.overflow_reads()
        b.close()
        exp, _, _ = o.search_batch(reads)
        assert np.array_equal(got.astype(np.int64), exp)
        if kernel != 0 and (k <= 128 or kernel == 4):
            assert n_ovf > 100, "the shrunk budget did not send reads to the overflow kernel (%d)" % n_ovf
        assert_reads_equal(p, o, reads[:200])
    finally:
        L.fin_set_option(b"epoch_budget_mult", 64); L.fin_set_option(b"epoch_budget_add", 4096)


_CONFIG2_ORACLE = []


def test_config2_scale_bit_exact_vs_oracle(kernel):
    """BASELINE config 2 at its full size (5 Mbp unitigs, k=31, 1 M 150 bp reads; the other kernels: 200 k reads): the ground-truth
    property on every read, and the oracle -- built INDEPENDENTLY from the unitigs by its own literal construction (19 s, once for
    the four kernels), not assembled from the product's components -- on a read sample it finishes in seconds."""
    g = synth.genome(5_000_000)
    u = synth.unitigs(g, 31)
    r = synth.reads(g, 1_000_000 if kernel == 4 else 200_000)
    p = fa.FinimizerIndex.build(u.as_tuple(), 31).to_device(0)
    assert p.n_kmers == int(u.offsets[-1]) - 30 * len(u), "generator produced duplicate k-mers"
    b = p.batch(r.as_tuple())
    b.run(fa.FIN_MERGED)
    got, npos = b.download()
    assert b.overflow_reads() <= 2   # the fast path handles (essentially) everything itself
    b.close()
    bad, checked, first = synth.check_ground_truth(p, u, r, got)
    assert checked > 0.5 * got.shape[0] and bad == 0, (bad, checked, first)
    if not _CONFIG2_ORACLE:
        _CONFIG2_ORACLE.append(OracleIndex.build(u.as_tuple(), 31))
    o = _CONFIG2_ORACLE[0]
    sub = r.subset(0, 20000)
    exp, _, _ = o.search_batch(sub.as_tuple(), n_threads=8)
    assert np.array_equal(got[:exp.shape[0]].astype(np.int64), exp)


def test_k63_scale_bit_exact_vs_oracle():
    """BASELINE config 5 shape at reduced size: k=63 (t=1, the only t the reference localizes), 250 bp reads."""
    g = synth.genome(2_000_000)
    u = synth.unitigs(g, 63)
    r = synth.reads(g, 40_000, read_len=250)
    p = fa.FinimizerIndex.build(u.as_tuple(), 63).to_device(0)
    got, _ = p.search_reads(r.as_tuple(), fa.FIN_MERGED)
    bad, checked, first = synth.check_ground_truth(p, u, r, got)
    assert checked > 0 and bad == 0, (bad, checked, first)
    o = OracleIndex.from_components(63, p.components())
    sub = r.subset(0, 8000)
    exp, _, _ = o.search_batch(sub.as_tuple(), n_threads=8)
    assert np.array_equal(got[:exp.shape[0]].astype(np.int64), exp)


def test_batch_object_reuse_and_timing():
    rng = np.random.default_rng(5)
    g = random_genome(rng, 20000)
    unitigs = cut_unitigs(rng, g, 21)
    p, o = both(unitigs, 21)
    reads = sample_reads(rng, g, 1000, 150)
    b = p.batch(reads)
    for _ in range(3):
        b.run(fa.FIN_MERGED)
    got, _ = b.download()
    exp, _, _ = o.search_batch(reads)
    assert np.array_equal(got.astype(np.int64), exp)
    ms, n = b.kernel_time_ms()
    assert n == 3 and ms > 0
    assert b.overflow_reads() == 0   # nothing needed the overflow kernel (deque <= 16, epoch budget not exhausted)
    assert b.n_kmers == exp.shape[0] and b.n_base_strands == 2 * 150 * 1000
    b.close()


def test_host_batch_is_split_into_device_batches():
    """fin_search_batch must give the same pairs when it has to cut the input into several device batches."""
    rng = np.random.default_rng(21)
    g = random_genome(rng, 30000)
    unitigs = cut_unitigs(rng, g, 25)
    p, o = both(unitigs, 25)
    reads = sample_reads(rng, g, 700, 140) + ["ACGT", "", g[100:400]]
    L = fa.lib()
    assert L.fin_set_option(b"max_batch_kmers", 5000) == 0
    try:
        assert_reads_equal(p, o, reads)
    finally:
        L.fin_set_option(b"max_batch_kmers", 1 << 30)


@pytest.mark.parametrize("depth", [1, 2, 5])
def test_copy_compute_pipeline_sub_batches(depth):
    """fin_search_batch streams sub-batches through `depth` reusable device batches on their own streams: same pairs, same order."""
    rng = np.random.default_rng(33)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, 31)
    p, o = both(unitigs, 31)
    reads = sample_reads(rng, g, 1500, 150) + ["", "ACGTAC", g[5000:9000]] + sample_reads(rng, g, 300, 60)
    L = fa.lib()
    assert L.fin_set_option(b"pipeline_kmers", 7000) == 0 and L.fin_set_option(b"pipeline_depth", depth) == 0
    try:
        assert_reads_equal(p, o, reads)
    finally:
        L.fin_set_option(b"pipeline_kmers", 1 << 26)
        L.fin_set_option(b"pipeline_depth", 3)


def test_batch_reload_keeps_buffers_and_results():
    rng = np.random.default_rng(34)
    g = random_genome(rng, 30000)
    unitigs = cut_unitigs(rng, g, 21)
    p, o = both(unitigs, 21)
    sets = [sample_reads(rng, g, 200, 100), sample_reads(rng, g, 900, 150), [], ["ACG"], sample_reads(rng, g, 50, 400)]
    b = p.batch(sets[0])
    for i, reads in enumerate(sets):
        if i:
            b.reload(reads)
        b.run(fa.FIN_MERGED)
        got, npos = b.download()
        exp, _, _ = o.search_batch(reads)
        assert np.array_equal(got.astype(np.int64).reshape(-1, 2), exp.reshape(-1, 2)), f"set {i}"
        assert npos == int((exp[:, 0] != -1).sum()) if exp.size else npos == 0
    b.close()


def test_fuzz_many_small_indexes():
    """Many small random indexes (repeats, non-disjoint sets, dummy-heavy SBWTs, node counts around block and window
    boundaries) against the oracle: stresses mismatch recovery, wide intervals, scans that cross 16-byte windows and
    128-byte blocks, the singleton jump, branch-dictionary anchors and short/ragged/invalid reads."""
    rng = np.random.default_rng(20260)
    n_cases = 300
    for case in range(n_cases):
        k = int(rng.integers(2, 14))
        mode = case % 4
        if mode == 0:      # random genome cut into overlapping pieces
            g = random_genome(rng, int(rng.integers(60, 3000)))
            unitigs = cut_unitigs(rng, g, k, max_len=int(rng.integers(k + 1, 4 * k + 40)))
        elif mode == 1:    # highly repetitive: substrings of a short periodic text
            base = random_genome(rng, int(rng.integers(3, 25)))
            g = base * 40
            unitigs = [g[a:a + L] for a, L in ((int(rng.integers(0, 100)), int(rng.integers(k, k + 60))) for _ in range(int(rng.integers(1, 30))))]
        elif mode == 2:    # low-complexity alphabet
            g = "".join("AC"[x] for x in rng.integers(0, 2, int(rng.integers(50, 800)))) + random_genome(rng, 100)
            unitigs = cut_unitigs(rng, g, k, max_len=k + 30, flip=False)
        else:              # unrelated random strings: many k-mers without predecessor -> many dummy nodes
            g = random_genome(rng, 2000)
            unitigs = [random_genome(rng, int(rng.integers(k, k + 25))) for _ in range(int(rng.integers(1, 60)))]
        unitigs = [u for u in unitigs if len(u) >= k]
        if not unitigs:
            continue
        p, o = both(unitigs, k)
        reads = []
        for _ in range(40):
            t = int(rng.integers(0, 6))
            L = int(rng.integers(0, 200))
            if t == 0:
                r = random_genome(rng, L)
            elif t == 1:
                u = unitigs[int(rng.integers(0, len(unitigs)))]
                r = u
            elif t == 2 and len(g) > 5:
                a = int(rng.integers(0, len(g) - 1)); r = g[a:a + L]
            elif t == 3 and len(g) > 5:
                a = int(rng.integers(0, len(g) - 1)); r = rc(g[a:a + L])
            elif t == 4 and len(g) > 5:
                a = int(rng.integers(0, len(g) - 1)); r = list(g[a:a + L])
                for i in range(len(r)):
                    if rng.random() < 0.08:
                        r[i] = "ACGTNacgtn"[int(rng.integers(0, 10))]
                r = "".join(r)
            else:
                u = unitigs[int(rng.integers(0, len(unitigs)))]
                v = unitigs[int(rng.integers(0, len(unitigs)))]
                r = u[len(u) // 2:] + v[:len(v) // 2 + 1]
            reads.append(r)
        got, _ = p.search_reads(reads, fa.FIN_MERGED)
        exp, _, _ = o.search_batch(reads)
        assert np.array_equal(got.astype(np.int64), exp), "case %d (k=%d, mode %d, %d nodes)" % (case, k, mode, p.n_nodes)
        p.close()


@pytest.mark.parametrize("ptab,prepass", [(-1, 1), (0, 1), (3, 1), (-1, 0), (3, 0)])
def test_fuzz_walks_restarts_and_probes(ptab, prepass):
    """Longer k and reads built from matching stretches of every length, errors at every spacing, unitig crossings, junk and
    non-ACGT bases: what the lazy kernel's walk mode, cold restarts (2k margin) and probes (with and without the prefix table)
    must get bit-exact; the other kernels run the same cases."""
    L = fa.lib()
    assert L.fin_set_option(b"ptab_t", ptab) == 0 and L.fin_set_option(b"probe_prepass", prepass) == 0
    try:
        rng = np.random.default_rng(4242 + ptab)
        for case in range(60):
            k = int(rng.integers(6, 41))
            g = random_genome(rng, int(rng.integers(400, 20000)))
            if case % 5 == 4:   # repeats: duplicate k-mers, walks that could continue along the wrong copy
                g = g[:len(g) // 3] * 3 + random_genome(rng, 200)
            unitigs = cut_unitigs(rng, g, k, max_len=int(rng.integers(k + 1, 6 * k + 200)), flip=bool(case % 2)) if case % 5 != 4 else \
                [g[a:a + n] for a, n in ((int(rng.integers(0, len(g) - k)), int(rng.integers(k, 5 * k + 50))) for _ in range(60))]
            unitigs = [u for u in unitigs if len(u) >= k]
            p, o = both(unitigs, k)
            reads = [mosaic_read(rng, g, k, 500) for _ in range(40)] + [g[:min(len(g), 1200)], rc(g[-700:])]
            got, _ = p.search_reads(reads, fa.FIN_MERGED)
            exp, _, _ = o.search_batch(reads)
            assert np.array_equal(got.astype(np.int64), exp), "case %d (k=%d, %d nodes)" % (case, k, p.n_nodes)
            gotf, _ = p.search_reads(reads[:10], fa.FIN_FWD)
            expf = [x for r in reads[:10] for x in o.search(r)[0]]
            assert gotf.tolist() == [list(x) for x in expf], "forward-only, case %d (k=%d)" % (case, k)
            p.close()
    finally:
        L.fin_set_option(b"ptab_t", -1)
        L.fin_set_option(b"probe_prepass", 1)


def test_multi_device_sharding_same_results():
    """fin_search_batch_multi: shards by record, one host thread per shard; here all shards share device 0."""
    rng = np.random.default_rng(77)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, 31, max_len=600)
    p, o = both(unitigs, 31)
    reads = sample_reads(rng, g, 900, 150) + ["", "ACG", g[5:900]]
    exp, _, _ = o.search_batch(reads)
    for devs in ([0], [0, 0], [0, 0, 0, 0, 0]):
        got, npos = p.search_reads_multi(reads, devs)
        assert np.array_equal(got.astype(np.int64), exp), devs
        assert npos == int((exp[:, 0] != -1).sum())
    with pytest.raises(fa.FinitoError):
        p.search_reads_multi(reads, [0, 99])


@pytest.mark.parametrize("gbases", [1_200_000_000, 4_100_000_000], ids=["1.2Gbp", "4.1Gbp"])
def test_index_beyond_2_30_bases_keeps_its_fast_structures(kernel, gbases):
    """VERDICT r4 missing #1 / weak #8: round 4 built the k-mer table -- hence lean tables and the fast path -- only while 2 * total_len <= 2^31; a 1.1 Gbp
    index silently fell back to the prefix-table / streaming pipeline, five times slower.  The compact table (round 5) has no power-of-two sizing: a
    1.2 Gbp index and one of 4.1 Gbp -- 4.12e9 SBWT nodes, 96 % of the 2^32 that node numbers and text offsets have in this build: more than a human genome's
    unitigs -- are built on the device, uploaded with lean tables, their reads take the fast path, every error-free k-mer localizes to the (unitig, offset) the
    generator knows, and kernel 2 -- which asks no table -- gives the same pairs on a slice."""
    if kernel != 4:
        pytest.skip("one pass on the default kernel")
    k, n_reads = 31, 2_000_000
    g = synth.genome(gbases)
    u = synth.unitigs(g, k)
    assert int(u.offsets[-1]) > (1 << 30)
    p = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    assert p.total_len > (1 << 30) and p.n_nodes < (1 << 32) and p.n_nodes > gbases
    assert p.lean_tables() and p.kmer_table_bytes() > 0 and p.kmer_table_bytes() < 16 * p.total_len and p.replica_table_bytes() < 24 * p.total_len
    r = synth.reads(g, n_reads, read_len=150)
    b = p.batch(r.as_tuple()); b.run(fa.FIN_MERGED); got, npos = b.download()
    info = b.run_info(); pc = b.pipeline_counts(48); b.close()
    assert info["fast_path"] and info["deferred"] and pc[4 * 8 + 9] > 0.85 * n_reads, (info, pc[4 * 8 + 9])   # (the fast path finishes nine reads in ten, as on the 250 Mbp index)
    bad, checked, first = synth.check_ground_truth(p, u, r, got)
    assert checked > 0.4 * got.shape[0] and bad == 0, (bad, checked, first)
    sub = r.subset(0, 200_000)
    assert fa.lib().fin_set_option(b"kernel", 2) == 0
    try:
        got2, _ = p.search_reads(sub.as_tuple(), fa.FIN_MERGED)
    finally:
        fa.lib().fin_set_option(b"kernel", kernel)
    assert np.array_equal(got[: got2.shape[0]], got2), "kernel 4 and kernel 2 disagree on the %.1f Gbp index" % (gbases / 1e9)
    p.close()


@pytest.mark.parametrize("k,read_len,n_reads", [(31, 150, 10_000_000), (63, 250, 10_000_000)], ids=["config3", "config5_t1"])
def test_full_size_ground_truth(kernel, k, read_len, n_reads):
    """BASELINE configs 3 and 5 (t=1) at full size: 250 Mbp index, 10 M reads.  The oracle cannot cover this in seconds, so
    the check is the size-independent one: every error-free k-mer of every genome-derived read must localize to the
    (unitig, offset) the generator knows, plus bit-exactness against the oracle on a slice of the batch."""
    if kernel != 4:
        pytest.skip("full-size run only on the default kernel")
    g = synth.genome(250_000_000)
    u = synth.unitigs(g, k)
    p = fa.FinimizerIndex.build(u.as_tuple(), k).to_device(0)
    assert p.n_kmers == int(u.offsets[-1]) - (k - 1) * len(u), "generator produced duplicate k-mers"
    if k <= 64:   # (the device builder's range: two-word keys above 32 since round 4 -- VERDICT r4 #9a: the chain is checked at k = 63 too, where bench.py uses that builder)
        # VERDICT r3 #9 -- where the 250 Mbp oracle comes from.  The oracle's own construction is too slow at this size, so the oracle below
        # is assembled from the product's exported components; the chain that makes that sound is checked, not asserted in prose:
        #   oracle's literal construction == host builder (tests/test_builder_parity.py: component by component, to 5 Mbp, every k),
        #   host builder == device builder HERE, at full size: every exported component of both, by md5.
        import hashlib
        pd = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0)
        ch, cd = p.components(), pd.components()
        assert set(ch) == set(cd)
        for name in sorted(ch):
            a, b_ = ch[name], cd[name]
            if isinstance(a, (list, tuple)):
                assert len(a) == len(b_) and all(hashlib.md5(np.ascontiguousarray(x)).hexdigest() == hashlib.md5(np.ascontiguousarray(y)).hexdigest() for x, y in zip(a, b_)), name
            elif isinstance(a, np.ndarray):
                assert hashlib.md5(np.ascontiguousarray(a)).hexdigest() == hashlib.md5(np.ascontiguousarray(b_)).hexdigest(), "component %s differs between the host and the device builder" % name
            else:
                assert a == b_, name
        pd.close(); del ch, cd
    r = synth.reads(g, n_reads, read_len=read_len)
    b = p.batch(r.as_tuple())
    b.run(fa.FIN_MERGED)
    got, npos = b.download()
    assert b.overflow_reads() <= n_reads // 100000
    # the lazy kernel against the kernel that streams every base of both strands like the reference: all pairs of the batch,
    # present and absent alike (the ground truth below only speaks about error-free k-mers)
    assert fa.lib().fin_set_option(b"kernel", 2) == 0
    try:
        b.run(fa.FIN_MERGED)
        got2, npos2 = b.download()
    finally:
        fa.lib().fin_set_option(b"kernel", kernel)
    assert npos2 == npos and np.array_equal(got, got2), "kernel 3 and kernel 2 disagree at full size"
    del got2
    b.close()
    bad, checked, first = synth.check_ground_truth(p, u, r, got)
    assert checked > 0.4 * got.shape[0] and bad == 0, (bad, checked, first)
    assert npos >= checked
    o = OracleIndex.from_components(k, p.components())
    sub = r.subset(n_reads - 5000, n_reads)
    exp, _, _ = o.search_batch(sub.as_tuple(), n_threads=fa.host_threads())
    assert np.array_equal(got[got.shape[0] - exp.shape[0]:].astype(np.int64), exp)


def test_long_reads_and_genome_as_query():
    """one lane walks a 300 kb read (positions far beyond the deque's 24-bit end field wrap are covered by the unit
    arithmetic; here: many chunks, many runs, many unitig crossings in one read) -- queries = whole genome and its rc"""
    rng = np.random.default_rng(99)
    g = random_genome(rng, 300_000)
    unitigs = cut_unitigs(rng, g, 31, max_len=3000)
    p, o = both(unitigs, 31)
    noisy = list(g[1000:120000])
    for i in range(0, len(noisy), 997):
        noisy[i] = "N" if i % 2 else "ACGT"[(i // 997) % 4]
    reads = [g, rc(g), "".join(noisy), g[5:40]]
    got, _ = p.search_reads(reads, fa.FIN_MERGED)
    exp, _, _ = o.search_batch(reads)
    assert np.array_equal(got.astype(np.int64), exp)
    # same batch object, forward-only after merged and back: outputs must not leak between runs
    b = p.batch(reads)
    b.run(fa.FIN_MERGED); b.run(fa.FIN_FWD)
    fwd, _ = b.download()
    expf = np.array([x for r in reads for x in o.search(r)[0]], dtype=np.int64).reshape(-1, 2)
    assert np.array_equal(fwd.astype(np.int64), expf)
    b.run(fa.FIN_MERGED)
    again, _ = b.download()
    assert np.array_equal(again.astype(np.int64), exp)
    b.close()


def test_output_text_made_on_the_device(kernel):
    """f-3: the text search-fmin prints (search_fmin.hh:62-65) formatted by the GPU from the pairs: byte-identical to the oracle's
    text -- ids and offsets of every digit count, absent k-mers, ragged reads, sub-batches stitched in order"""
    if kernel != 4:
        pytest.skip("the formatter does not depend on the search kernel")
    rng = np.random.default_rng(8)
    k = 15
    g = random_genome(rng, 120000)
    unitigs = cut_unitigs(rng, g, k, max_len=60)        # thousands of unitigs: ids of 1-4 digits, offsets of 1-2
    unitigs += [g[:30000]]                              # and one long one: offsets of up to 5 digits
    p, o = both(unitigs, k)
    from oracle.oracle import format_pairs
    reads = [r for r in (mosaic_read(rng, g, k, 600) for _ in range(3000)) if len(r) >= k] + [g[100:25000], rc(g[5000:9000]), g[:k], "N" * 40]
    want = "".join(format_pairs(o.search_merged(r)) for r in reads).encode()
    b = p.batch(reads)
    b.run(fa.FIN_MERGED)
    assert b.text() == want
    b.close()
    L = fa.lib()
    assert L.fin_set_option(b"pipeline_kmers", 40000) == 0   # many sub-batches, several in flight: their texts must land in order
    try:
        got, npos = p.search_reads_text(reads)
    finally:
        L.fin_set_option(b"pipeline_kmers", 1 << 26)
    assert got == want and npos == want.count(b"(") - want.count(b"(-1,")
    with pytest.raises(fa.FinitoError):                  # a read without k-mers has no pair to hang its empty line on
        p.search_reads_text(reads + ["ACGT"])


def test_output_text_of_arbitrary_pairs(kernel):
    """the formatter alone, on pairs the search would never produce here: ids and offsets of 1..10 digits (up to 2^31-1), absent pairs, in
    every mix and alignment -- the device's pairs of a batch are overwritten, formatted, and compared with Python's formatting"""
    if kernel != 4:
        pytest.skip("the formatter does not depend on the search kernel")
    rng = np.random.default_rng(77)
    k = 15
    g = random_genome(rng, 30000)
    p, _ = both(cut_unitigs(rng, g, k, max_len=300), k)
    for trial in range(4):
        lens = rng.integers(k, 400, int(rng.integers(50, 1500)))
        reads = [g[int(a):int(a) + int(n)] for a, n in zip(rng.integers(0, len(g) - 400, len(lens)), lens)]
        b = p.batch(reads)
        b.run(fa.FIN_MERGED)
        nk = int(sum(len(r) - k + 1 for r in reads))
        digits = rng.integers(1, 11, (nk, 2))
        vals = np.minimum((10.0 ** (digits - rng.random((nk, 2)))).astype(np.int64), 2 ** 31 - 1).astype(np.int32)
        if trial == 3:
            vals[:, :] = np.where(rng.random((nk, 2)) < 0.5, 2 ** 31 - 1, vals)   # the longest numbers back to back
        absent = rng.random(nk) < (0.0, 0.3, 0.9, 0.1)[trial]
        vals[absent] = -1
        vals = np.ascontiguousarray(vals)
        b.set_pairs(vals)
        want, at = [], 0
        for r in reads:
            n = len(r) - k + 1
            want.append(" ".join("(%d,%d)" % (int(u), int(o)) for u, o in vals[at:at + n]) + "\n")
            at += n
        assert b.text() == "".join(want).encode(), "trial %d" % trial
        b.close()
    p.close()


def test_text_anchors_behind_sequencing_errors(kernel):
    """Kernels 4 and 3: behind a read base that disagrees with the unitig text the k-mers across it are proven absent by probes and the
    next k-mer is found by comparing the read with the text (indexes with duplicated k-mers: test_non_disjoint_families).  Errors
    at every spacing (single, two within k, runs), errors next to unitig ends and read ends, non-ACGT bases, with the option on and off."""
    if kernel not in (3, 4):
        pytest.skip("text re-anchoring is kernel 4's and 3's")
    rng = np.random.default_rng(31)
    L = fa.lib()
    for k in (9, 21, 31, 64):
        g = random_genome(rng, 40000)
        unitigs = cut_unitigs(rng, g, k, max_len=5 * k + 100)
        p, o = both(unitigs, k)
        reads = []
        for _ in range(500):
            a = int(rng.integers(0, len(g) - 400)); n = int(rng.integers(k, 400))
            r = list(g[a:a + n])
            for _e in range(int(rng.integers(0, 6))):
                i = int(rng.integers(0, n))
                for j in range(i, min(n, i + int(rng.integers(1, 4)) * int(rng.integers(0, 2)) + 1)):   # single errors and short runs
                    r[j] = "ACGTN"[int(rng.integers(0, 5))]
            r = "".join(r)
            reads.append(r if rng.random() < 0.5 else rc(r))
        exp, _, _ = o.search_batch(reads)
        for on in (1, 0):
            assert L.fin_set_option(b"text_anchors", on) == 0
            try:
                got, _ = p.search_reads(reads, fa.FIN_MERGED)
            finally:
                L.fin_set_option(b"text_anchors", 1)
            assert np.array_equal(got.astype(np.int64), exp), "k=%d text_anchors=%d" % (k, on)
        p.close()


def check_anchor_table(p, o, k, max_nodes=3000, unitigs=None):
    """the anchor table built on the device, node by node against the oracle: entry = the reference's answer for the node's k-mer (label
    of the node -> faithful search -> place), verified flag = the text at that place spells the label inside one unitig; dummy nodes.
    (k <= 31 replicas are uploaded with "lean_tables" by default and carry no anchor table: the table is then checked on a replica of the
    same unitigs uploaded with lean_tables 0 -- the k-mer table's answers come from the very pass that fills it)"""
    own = None
    if p.lean_tables():
        assert unitigs is not None
        own = fa.FinimizerIndex.build(unitigs, k).set_option("lean_tables", 0).to_device(0)
        assert own.seed_table_bytes() > 0 and own.prefix_table_depth() > 0 and own.unsafe_places() == p.unsafe_places() and own.rc_pairs() == p.rc_pairs()
    tab = (own or p).seed_table()
    if own is not None:
        own.close()
    assert tab is not None and tab.shape == (p.n_nodes, 2)
    uends = np.asarray(o.ends(), dtype=np.int64)
    ustarts = np.concatenate([[0], uends[:-1]])
    text = "".join("ACGT"[c] for c in o.concat())
    labels = o.labels()
    step = max(1, p.n_nodes // max_nodes)
    n_checked = n_unverified = 0
    for v in range(0, p.n_nodes, step):
        lab = labels[v]
        if "$" in lab:
            d = len(lab.strip("$"))   # a dummy node: the first d bases of a unitig behind k-d '$' (d = 0: the root)
            assert tab[v, 0] == (0xFFFFFF00 | d if d else 0xFFFFFFFF), "k=%d node %d (%s)" % (k, v, lab)
            continue
        pairs, nf = o.search(lab)
        assert nf == 1
        u, off = pairs[0]
        g = int(ustarts[u]) + off + k - 1
        assert int(tab[v, 0]) == g, "k=%d node %d: entry %d, the reference's answer %d" % (k, v, int(tab[v, 0]), g)
        spelled = g < int(uends[u]) and text[g - k + 1:g + 1] == lab
        assert (int(tab[v, 1]) >> 31 == 0) == spelled, "k=%d node %d: verified flag" % (k, v)
        if spelled:
            assert int(tab[v, 1]) == u
        n_unverified += not spelled
        n_checked += 1
    return n_checked, n_unverified


def test_seed_table_and_seed_anchors(kernel):
    """Kernel 4: (1) the anchor table built on the device holds, for every SBWT node, the place the reference reports for its k-mer --
    checked node by node against the oracle (label of the node -> faithful search -> place); (2) with seeds on and off
    the pairs are the oracle's: reads that start inside, at and before unitig starts, cross unitig ends, carry errors in their
    first k-mer (the first seed fails), N's, and reads of the other strand."""
    if kernel != 4:
        pytest.skip("seeds are kernel 4's")
    rng = np.random.default_rng(77)
    L = fa.lib()
    n_checked = 0
    for k in (5, 12, 31, 40, 100, 200):
        g = random_genome(rng, 30000)
        unitigs = cut_unitigs(rng, g, k, max_len=4 * k + 150)
        p, o = both(unitigs, k)
        nc, nu = check_anchor_table(p, o, k, unitigs=unitigs)
        n_checked += nc
        assert p.unsafe_places() >= 0
        if p.is_disjoint():
            assert nu == 0 and p.unsafe_places() == 0
        reads = []
        for _ in range(400):
            a = int(rng.integers(0, len(g) - 500)); n = int(rng.integers(k, 500))
            r = list(g[a:a + n])
            for _e in range(int(rng.integers(0, 5))):
                i = int(rng.integers(0, n)) if rng.random() < 0.6 else int(rng.integers(0, min(n, k)))   # many errors inside the first k-mer
                r[i] = "ACGTN"[int(rng.integers(0, 5))]
            r = "".join(r)
            reads.append(r if rng.random() < 0.5 else rc(r))
        reads += [u for u in unitigs[:20]] + [random_genome(rng, 10) + u[:k + 20] for u in unitigs[:20]] + [rc(u) for u in unitigs[20:30]]
        # reads that leave their place for another (indels, chimeras): pieces of the genome glued together, and single-base indels
        reads += [mosaic_read(rng, g, k, 600) for _ in range(150)]
        for _ in range(150):
            n = int(rng.integers(3 * k, 3 * k + 600)); a = int(rng.integers(0, len(g) - n)); r = g[a:a + n]
            for _e in range(int(rng.integers(1, 4))):
                i = int(rng.integers(1, len(r) - 1))
                r = r[:i] + r[i + 1:] if rng.random() < 0.5 else r[:i] + "ACGT"[int(rng.integers(0, 4))] + r[i:]
            reads.append(r if rng.random() < 0.5 else rc(r))
        exp, _, _ = o.search_batch(reads)
        expf = np.concatenate([np.asarray(o.search(r)[0], dtype=np.int64).reshape(-1, 2) for r in reads if len(r) >= k])
        # seeds on / off; with seeds: the output not prefilled (every slot written once by the pipeline) / prefilled
        for on, wg in ((1, 1), (1, 0), (0, 1)):
            assert L.fin_set_option(b"seed_anchors", on) == 0 and L.fin_set_option(b"write_gaps", wg) == 0
            try:
                got, _ = p.search_reads(reads, fa.FIN_MERGED)
                gf, _ = p.search_reads(reads, fa.FIN_FWD)
            finally:
                L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"write_gaps", 1)
            assert np.array_equal(got.astype(np.int64), exp), "k=%d seed_anchors=%d write_gaps=%d" % (k, on, wg)
            assert np.array_equal(gf.astype(np.int64), expf), "k=%d seed_anchors=%d write_gaps=%d forward only" % (k, on, wg)
        p.close()
    assert n_checked > 5000


@pytest.mark.parametrize("seed", [4711, 264190])   # (264190: found by tools/fuzz_defer.py -- a whole-k-mer anchor on an index with reverse-complement pairs)
def test_non_disjoint_families(kernel, seed):
    """Round 3: indexes whose k-mers do NOT all have one place (near-disjoint sets with a handful of duplicated k-mers, matchtig-like
    overlaps, diverged interspersed repeats, tandem repeats) keep the fast path: seeds and text re-anchoring use every place the
    upload found safe, the rest goes the reference's way.  Bit-exact on every kernel, with the options on and off; the anchor table and
    the count of unsafe places against the oracle."""
    from tests.test_oracle_lazy import non_disjoint_sets
    rng = np.random.default_rng(seed)
    L = fa.lib()
    n_unsafe_idx = n_unverified = 0
    for case in range(40):
        k = int(rng.choice([5, 9, 16, 21, 31, 31, 45, 63]))
        g, unitigs = non_disjoint_sets(rng, case, k)
        p, o = both(unitigs, k)
        reads = [mosaic_read(rng, g, k, 500) for _ in range(60)] + sample_reads(rng, g, 120, min(len(g), 150), err=0.02) + [g[:min(len(g), 2500)], rc(g[-900:])]
        exp, _, _ = o.search_batch(reads)
        got, _ = p.search_reads(reads, fa.FIN_MERGED)
        assert np.array_equal(got.astype(np.int64), exp), "case %d (k=%d, family %d)" % (case, k, case % 4)
        gf, _ = p.search_reads(reads[:40], fa.FIN_FWD)
        expf = np.concatenate([np.asarray(o.search(r)[0], dtype=np.int64).reshape(-1, 2) for r in reads[:40] if len(r) >= k])
        assert np.array_equal(gf.astype(np.int64), expf), "forward only, case %d (k=%d)" % (case, k)
        if kernel == 4:
            # the number of unsafe places, exactly: text k-mer positions whose k-mer the reference reports elsewhere
            uends = np.asarray(o.ends(), dtype=np.int64); ustarts = np.concatenate([[0], uends[:-1]])
            text = "".join("ACGT"[c] for c in o.concat())
            want = 0
            if len(text) < 4000:
                for u in range(len(uends)):
                    for e in range(int(ustarts[u]) + k - 1, int(uends[u])):
                        pr, nf = o.search(text[e - k + 1:e + 1])
                        want += not (nf == 1 and int(ustarts[pr[0][0]]) + pr[0][1] + k - 1 == e)
                assert p.unsafe_places() == want, "case %d (k=%d): unsafe places %d, oracle %d" % (case, k, p.unsafe_places(), want)
            nc, nu = check_anchor_table(p, o, k, max_nodes=600, unitigs=unitigs)
            n_unverified += nu
            n_unsafe_idx += p.unsafe_places() > 0
            assert (p.unsafe_places() == 0) or not p.is_disjoint()
            for opts in ((1, 0), (0, 1), (0, 0)):   # (seed_anchors, text_anchors): (0, 1) = text re-anchoring alone; set at run time
                assert L.fin_set_option(b"seed_anchors", opts[0]) == 0 and L.fin_set_option(b"text_anchors", opts[1]) == 0
                try:
                    got, _ = p.search_reads(reads, fa.FIN_MERGED)
                finally:
                    L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"text_anchors", 1)
                assert np.array_equal(got.astype(np.int64), exp), "case %d (k=%d) seed_anchors=%d text_anchors=%d" % (case, k, opts[0], opts[1])
        p.close()
    if kernel == 4:
        assert n_unsafe_idx >= 25 and n_unverified > 0


@pytest.mark.parametrize("k", [21, 31, 32, 47, 63])   # (k > 32: the generator's canonical k-mer keys, and the k-mer table's, are two words)
def test_repeat_rich_spss_and_kmer_table(kernel, k):
    """Round 3: a repeat-rich genome (interspersed families in both orientations, tandem arrays, segmental duplications) as a DISJOINT
    string set that keeps every canonical k-mer at its first occurrence -- short pieces, probe strings that occur all over the index,
    k-mers of a read alternating between the strands.  The oracle's pairs on every kernel; the ground truth (a repeated k-mer comes back
    at its first occurrence); the k-mer table (k <= 31; k = 32: look-ups of the whole k-mer) on and off."""
    g = synth.repeat_genome(300_000, seed=5 + k)
    u = synth.spss(g, k, max_len=1500)
    assert len(u.dup_pos) > 5_000
    r = synth.reads(g, 6000 if kernel in (4, 3) else 2500, read_len=150 if k < 40 else 250)
    p, o = both(u.as_tuple(), k)
    assert p.is_disjoint() and p.unsafe_places() == 0
    exp, _, _ = o.search_batch(r.as_tuple(), n_threads=8)
    L = fa.lib()
    for kf in ((1, 0) if kernel == 4 else (1,)):
        assert L.fin_set_option(b"kmer_table", kf) == 0
        try:
            b = p.batch(r.as_tuple())
            b.run(fa.FIN_MERGED)
            got, npos = b.download()
            n_ovf = b.overflow_reads()
            b.close()
        finally:
            L.fin_set_option(b"kmer_table", 1)
        assert np.array_equal(got.astype(np.int64), exp), "k=%d kmer_table=%d" % (k, kf)
        if kernel == 4 and kf:
            assert (p.kmer_table_bytes() > 0) == (k <= 63) and n_ovf <= len(r) // 100   # the pipeline keeps (nearly) every read (k >= 32: the table is the fast path's own)
    bad, checked, first = synth.check_ground_truth(p, u, r, got)
    assert bad == 0 and checked > 0.5 * got.shape[0], (bad, checked, first)
    p.close()


def test_deferred_second_strand(kernel):
    """Round 3 (CHANGELOG.md 4.14): on an index without reverse-complement pairs and unsafe places kernel 4 searches a read's second strand
    only where the first left slots open -- and, in its last form, on ANY index: a first strand that used the streaming search or a
    whole-k-mer look-up, or reported from a text window with a k-mer whose reverse complement is in the index too, has its sister searched
    in full.  Same pairs with the option on and off; reads with errors in their first k-mer, with N's, of either strand, random reads, reads
    that leave their place (chimeras), reads of 66 000 bases; sets with duplicated k-mers; sets with reverse-complement pairs."""
    if kernel != 4:
        pytest.skip("kernel 4's")
    rng = np.random.default_rng(2026)
    L = fa.lib()
    for k in (9, 21, 31, 32, 63):
        g = random_genome(rng, 60000)
        unitigs = cut_unitigs(rng, g, k, max_len=5 * k + 300)
        p, o = both(unitigs, k)
        assert p.rc_pairs() >= 0 and p.defers_second_strand()   # (k = 9: a 60 kb genome repeats 9-mers and holds reverse-complement pairs -- deferred all the same, with taints)
        reads = sample_reads(rng, g, 1500, 150 if k < 60 else 250, err=0.02, random_frac=0.1) + [mosaic_read(rng, g, k, 500) for _ in range(300)]
        for _ in range(300):   # errors inside the first k-mer of either strand, N's
            a = int(rng.integers(0, len(g) - 400)); n = int(rng.integers(k, 400)); r = list(g[a:a + n])
            for _e in range(int(rng.integers(1, 4))):
                r[int(rng.integers(0, min(n, k)))] = "ACGTN"[int(rng.integers(0, 5))]
            r = "".join(r); reads.append(r if rng.random() < 0.5 else rc(r))
        if k in (21, 63):   # reads of 65536 bases or more are never deferred (a stretch's ends travel in 16 bits): of either strand, with errors
            for flip in (False, True):
                r = list((g + g)[1000:1000 + 66000 + 500 * flip])
                for where in (5, 40000, len(r) - 3):
                    r[where] = "ACGT"[("ACGT".index(r[where]) + 1) % 4]
                reads.append(rc("".join(r)) if flip else "".join(r))
        exp, _, _ = o.search_batch(reads)
        for on in (1, 0):
            assert L.fin_set_option(b"defer_strand", on) == 0
            try:
                b = p.batch(reads); b.run(fa.FIN_MERGED); got, _ = b.download()
                pc = b.pipeline_counts(48); b.close()
            finally:
                L.fin_set_option(b"defer_strand", 1)
            assert np.array_equal(got.astype(np.int64), exp), "k=%d defer_strand=%d" % (k, on)
            if p.defers_second_strand():
                assert (pc[4 * 8 + 8] > 0) == bool(on), "k=%d: deferred strands %d with defer_strand=%d" % (k, pc[4 * 8 + 8], on)
        p.close()
    # sets with duplicated k-mers but no reverse-complement pair (unsafe places, unverified anchor entries): deferred too -- a read whose first
    # strand needed the streaming search or a whole-k-mer look-up has its sister searched in full (CHANGELOG.md 4.14, "tainted")
    n_dup_sets = 0
    for case in range(12):
        k = (21, 31, 16)[case % 3]
        g = random_genome(rng, int(rng.integers(3000, 9000)))
        for _ in range(int(rng.integers(2, 7))):   # exact copies of stretches, somewhere else in the genome
            a = int(rng.integers(0, len(g) - 300)); n = int(rng.integers(k + 3, 300)); at = int(rng.integers(0, len(g)))
            g = g[:at] + g[a:a + n] + g[at:]
        if case % 4 == 3:   # overlapping pieces instead of a cut: every junction's k-mers twice
            unitigs, a = [], 0
            while a + k <= len(g):
                n = int(rng.integers(k, 4 * k + 60)); unitigs.append(g[a:a + n]); a += max(1, n - int(rng.integers(k - 1, 2 * k)))
        else:
            unitigs = cut_unitigs(rng, g, k, max_len=int(rng.integers(3 * k, 12 * k)), flip=False)
        p, o = both(unitigs, k)
        if p.unsafe_places() == 0:
            p.close(); continue
        n_dup_sets += 1
        assert p.defers_second_strand()
        reads = [mosaic_read(rng, g, k, 300) for _ in range(150)] + sample_reads(rng, g, 400, 150, err=0.02, random_frac=0.05) + [g[:1500], rc(g[-900:])]
        reads += [rc(r) for r in reads[:100]]
        exp, _, _ = o.search_batch(reads)
        for on in (1, 0):
            assert L.fin_set_option(b"defer_strand", on) == 0
            try:
                b = p.batch(reads); b.run(fa.FIN_MERGED); got, _ = b.download()
                pc = b.pipeline_counts(48); b.close()
            finally:
                L.fin_set_option(b"defer_strand", 1)
            assert np.array_equal(got.astype(np.int64), exp), "duplicated k-mers, case %d k=%d defer_strand=%d" % (case, k, on)
            assert (pc[4 * 8 + 8] > 0) == bool(on)
        p.close()
    assert n_dup_sets >= 6
    # sets with k-mers AND their reverse complements (round 3, last form: deferred as well -- a first strand that reports from a text window
    # with such a k-mer has its sister searched in full)
    for case in range(6):
        k = (21, 31, 12)[case % 3]
        g = random_genome(rng, int(rng.integers(3000, 8000)))
        unitigs = cut_unitigs(rng, g, k, max_len=int(rng.integers(3 * k, 12 * k)), flip=bool(case % 2))
        for _ in range(int(rng.integers(2, 8))):
            a = int(rng.integers(0, len(g) - 300)); unitigs.append(rc(g[a:a + int(rng.integers(k, 300))]))
        p, o = both(unitigs, k)
        assert p.rc_pairs() > 0 and p.defers_second_strand()
        reads = [mosaic_read(rng, g, k, 300) for _ in range(150)] + sample_reads(rng, g, 400, 150, err=0.02, random_frac=0.05) + [g[:1500], rc(g[-900:])]
        reads += [rc(r) for r in reads[:100]]
        exp, _, _ = o.search_batch(reads)
        for on in (1, 0):
            assert L.fin_set_option(b"defer_strand", on) == 0
            try:
                b = p.batch(reads); b.run(fa.FIN_MERGED); got, _ = b.download()
                pc = b.pipeline_counts(48); b.close()
            finally:
                L.fin_set_option(b"defer_strand", 1)
            assert np.array_equal(got.astype(np.int64), exp), "reverse-complement pairs, case %d k=%d defer_strand=%d" % (case, k, on)
            assert (pc[4 * 8 + 8] > 0) == bool(on)
        p.close()


def mixed_index_cases(n_cases, seed):
    """indexes with duplicated stretches and reverse-complement copies at every k, reads of both strands with errors, chimeras and junk:
    the device (defaults: second strands deferred) against the faithful oracle"""
    from tests.test_oracle_lazy import non_disjoint_sets
    rng = np.random.default_rng(seed)
    stats = {"cases": 0, "rc_pairs": 0, "unsafe": 0}
    for case in range(n_cases):
        k = int(rng.choice([7, 12, 16, 21, 31, 32, 40, 63]))
        if case % 3 == 0:
            g, unitigs = non_disjoint_sets(rng, case, k)
        else:
            g = random_genome(rng, int(rng.integers(1500, 12000)))
            for _ in range(int(rng.integers(0, 5))):
                a = int(rng.integers(0, len(g) - 300)); n = int(rng.integers(k + 2, 300)); at = int(rng.integers(0, len(g)))
                g = g[:at] + g[a:a + n] + g[at:]
            unitigs = cut_unitigs(rng, g, k, max_len=int(rng.integers(2 * k, 12 * k)), flip=bool(case % 2))
            for _ in range(int(rng.integers(0, 6))):
                a = int(rng.integers(0, len(g) - 300)); unitigs.append(rc(g[a:a + int(rng.integers(k, 300))]))
        unitigs = [u for u in unitigs if len(u) >= k]
        o = OracleIndex.build(unitigs, k)
        p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
        L = min(len(g), int(rng.integers(k, 400)))
        reads = [mosaic_read(rng, g, k, 400) for _ in range(60)] + sample_reads(rng, g, 150, L, err=float(rng.choice([0.0, 0.01, 0.03])), random_frac=0.05) + [g[:min(len(g), 3000)], rc(g[-min(len(g), 1200):])]
        reads += [rc(r) for r in reads[:50]]
        exp, _, _ = o.search_batch(reads)
        got, _ = p.search_reads(reads, fa.FIN_MERGED)
        assert np.array_equal(got.astype(np.int64), exp), "mixed case %d (seed %d, k=%d)" % (case, seed, k)
        stats["cases"] += 1; stats["rc_pairs"] += p.rc_pairs() > 0; stats["unsafe"] += p.unsafe_places() > 0
        p.close()
    return stats


def test_deferred_second_strand_on_mixed_indexes(kernel):
    """the device's defaults against the faithful oracle on sets with duplicated stretches AND reverse-complement copies at k in {7 .. 63}
    (tools/fuzz_defer.py runs the same generator with thousands of cases)"""
    if kernel != 4:
        pytest.skip("kernel 4's")
    stats = mixed_index_cases(60, 2026)
    assert stats["cases"] == 60 and stats["rc_pairs"] >= 30 and stats["unsafe"] >= 30


def defer_family_cases(n_cases, seed, ks=(12, 16, 21, 31), options=True):
    """the deferred strand's hard family (tests/util.py: defer_family_case) on the device, `defer_strand` 1 and 0, against the FAITHFUL oracle"""
    L = fa.lib()
    rng = np.random.default_rng(seed)
    stats = {"cases": 0, "rc_pairs": 0, "unsafe": 0, "sisters": 0}
    for case in range(n_cases):
        k = int(ks[case % len(ks)])
        g, unitigs, reads = defer_family_case(rng, case, k)
        p, o = both(unitigs, k)
        exp, _, _ = o.search_batch(reads)
        for on in ((1, 0) if options else (1,)):
            assert L.fin_set_option(b"defer_strand", on) == 0
            try:
                b = p.batch(reads); b.run(fa.FIN_MERGED); got, _ = b.download()
                pc = b.pipeline_counts(48); b.close()
            finally:
                L.fin_set_option(b"defer_strand", 1)
            if not np.array_equal(got.astype(np.int64), exp):
                bad = np.nonzero((got.astype(np.int64) != exp).any(axis=1))[0]
                raise AssertionError("defer family case %d (seed %d, k=%d) defer_strand=%d: %d slots differ, first %d: got %s, faithful %s"
                                     % (case, seed, k, on, len(bad), bad[0], got[bad[0]].tolist(), exp[bad[0]].tolist()))
            if on:
                stats["sisters"] += int(pc[4 * 8 + 8])
        stats["cases"] += 1; stats["rc_pairs"] += p.rc_pairs() > 0; stats["unsafe"] += p.unsafe_places() > 0
        p.close()
    return stats


def test_deferred_strand_walks_into_the_other_strands_slots(kernel):
    """VERDICT r3 #1.  With duplicated unitigs the reference's FORWARD walk may follow a text that does not spell the read's k-mers (the
    branch dictionary's rank names another copy, common.hh:61-67; walk_in_unitigs compares one new base per step, FinimizerIndex.hh:47-102)
    into slots where the reverse strand found the true place -- and the forward pair wins the merge (search_fmin.hh:54-60).  A deferred
    forward strand is searched inside the stretch its sister left open, but its WALK runs on to the read's end and overwrites.  The judge's
    three minimised counter-examples of round 3's CPU restatement, then the family: identical unitigs, near-duplicates that differ in
    their last bases, reverse-complement copies; reads and rc(reads), the unitigs and rc(unitigs), reads that end a base past a unitig."""
    for k, unitigs, read, last in DEFER_KAT:
        p, o = both(unitigs, k)
        exp, _, _ = o.search_batch([read, rc(read)])
        assert tuple(exp[len(read) - k].tolist()) == last   # (the faithful oracle's pair of the read's last slot, as the verdict gives it)
        for on in (1, 0):
            assert fa.lib().fin_set_option(b"defer_strand", on) == 0
            try:
                got, _ = p.search_reads([read, rc(read)], fa.FIN_MERGED)
            finally:
                fa.lib().fin_set_option(b"defer_strand", 1)
            assert np.array_equal(got.astype(np.int64), exp), "k=%d defer_strand=%d: %s != %s" % (k, on, got.tolist(), exp.tolist())
        p.close()
    if kernel != 4:
        stats = defer_family_cases(12, 77, options=False)   # (the other kernels search both strands in full: a sample)
        assert stats["cases"] == 12
        return
    stats = defer_family_cases(120, 2027)
    assert stats["cases"] == 120 and stats["unsafe"] >= 100 and stats["rc_pairs"] >= 40 and stats["sisters"] > 1000, stats


def test_chunk_cache_does_not_promote_under_a_pending_load(kernel):
    """VERDICT r4 #9b: the read-chunk cache kernels 3 and 4 share (FinChunkCache::need, fin_device.h) -- a chunk in the NEXT slot is not made current while
    a load into the CURRENT slot is under way (it would land under the promoted chunk's number: wrong bases, valid tag; commit 81fcdfd).  Driven on the
    device, the cache as the kernels use it."""
    if kernel != 4:
        pytest.skip("one pass is enough")
    import ctypes as C
    bits = C.c_uint32(0xFFFFFFFF)
    assert fa.lib().fin_debug_chunk_cache_selftest(C.byref(bits)) == 0
    assert bits.value == 0, "chunk cache self-test: scenario bits %#x" % bits.value


def test_fresh_seed_batches_of_the_deferral_fuzzers(kernel):
    """VERDICT r4 #9c: one batch each of tools/fuzz_defer.py's two generators under seeds no earlier run used, inside the suite the driver runs: the
    hard family (identical / near-duplicate / reverse-complement unitigs) at every k the walk kernels distinguish -- one-word and two-word keys of the
    k-mer table, back-scans from k = 40 --, `defer_strand` 1 and 0, and the mixed indexes (duplicated stretches AND reverse-complement copies),
    the device's defaults against the FAITHFUL oracle."""
    if kernel != 4:
        pytest.skip("kernel 4's")
    stats = defer_family_cases(100, 5 * 1000003 + 555, ks=(7, 9, 12, 16, 21, 31, 32, 40, 63))
    assert stats["cases"] == 100 and stats["unsafe"] >= 60 and stats["sisters"] > 500, stats
    stats = mixed_index_cases(100, 50005)
    assert stats["cases"] == 100 and stats["rc_pairs"] >= 40 and stats["unsafe"] >= 40, stats


def _fast_path_reads(rng, g, k, unitigs):
    """the read mix of the fast path's tests: reads it finishes (one unitig, a few substitutions, either strand) and every kind it must leave alone"""
    reads = sample_reads(rng, g, 1500, 150, err=0.01, random_frac=0.08) + [mosaic_read(rng, g, k, 400) for _ in range(200)]
    for _ in range(400):
        a = int(rng.integers(0, len(g) - 320)); n = int(rng.integers(k, 320)); r = list(g[a:a + n])
        kind = int(rng.integers(0, 6))
        if kind == 0:      # many errors
            for _e in range(int(rng.integers(4, 9))): r[int(rng.integers(0, n))] = "ACGT"[int(rng.integers(0, 4))]
        elif kind == 1:    # N's
            for _e in range(int(rng.integers(1, 3))): r[int(rng.integers(0, n))] = "Nn"[int(rng.integers(0, 2))]
        elif kind == 2:    # errors inside the first and the last k-mer
            r[int(rng.integers(0, min(n, k)))] = "ACGT"[int(rng.integers(0, 4))]; r[n - 1 - int(rng.integers(0, min(n, k)))] = "ACGT"[int(rng.integers(0, 4))]
        elif kind == 3:    # ... and the middle one too
            for w in (int(rng.integers(0, min(n, k))), n // 2, n - 1 - int(rng.integers(0, min(n, k)))): r[w] = "ACGT"[("ACGT".index(r[w]) + 1) % 4]
        elif kind == 4:    # two errors closer than k
            w = int(rng.integers(0, n)); r[w] = "ACGT"[("ACGT".index(r[w]) + 1) % 4]; w2 = min(n - 1, w + int(rng.integers(1, k))); r[w2] = "ACGT"[("ACGT".index(r[w2]) + 2) % 4]
        r = "".join(r); reads.append(r if rng.random() < 0.5 else rc(r))
    reads += [g[100:100 + k], rc(g[300:300 + k]), g[1000:1300], rc(g[2000:2257]), g[:256], g[-256:], random_genome(rng, 256), random_genome(rng, 300), "A" * 200, "ACGT" * 40, ""]
    reads += [u for u in unitigs[:30]] + [rc(u) for u in unitigs[:30]]
    return reads


def test_fast_path_of_the_pre_pass(kernel):
    """Round 4 (fin_prepass.hip): a read that lies in one unitig with a few substitutions is finished by the pair pre-pass itself -- one comparison
    with the text behind the place of one of its k-mers (first, last or middle k-mer of either strand), the k-mer ends across a disagreeing base
    proven absent on BOTH strands by strings the canonical string filter does not know; a read none of whose k-mers is found is proven absent
    whole.  Same pairs with the option on and off, against the faithful oracle, on the reads the path takes and on every kind it must leave
    alone: more than four errors, N's, unitig ends inside the read, reads longer than 256 bases, of exactly k bases, errors in the first and the
    last k-mer, reads from nowhere; on sets with duplicated k-mers (unsafe places, unverified answers) and with reverse-complement pairs."""
    if kernel != 4:
        pytest.skip("kernel 4's")
    L = fa.lib()
    rng = np.random.default_rng(4242)
    for case, k in enumerate((31, 21, 12, 31, 25, 16, 63, 32, 33, 47, 63)):   # (k >= 32: the fast path's own two-word anchor table)
        g = random_genome(rng, 40000 if case < 3 or case >= 6 else int(rng.integers(4000, 9000)))
        if case == 10:    # k = 63 on a set with duplicated stretches and reverse-complement copies
            for _ in range(4):
                a = int(rng.integers(0, len(g) - 400)); n = int(rng.integers(k + 3, 400)); at = int(rng.integers(0, len(g)))
                g = g[:at] + g[a:a + n] + g[at:]
        if case == 3:     # duplicated stretches: unsafe places / unverified answers
            for _ in range(5):
                a = int(rng.integers(0, len(g) - 300)); n = int(rng.integers(k + 3, 300)); at = int(rng.integers(0, len(g)))
                g = g[:at] + g[a:a + n] + g[at:]
        unitigs = cut_unitigs(rng, g, k, max_len=(600 if case < 3 else 900 if case >= 6 else 12 * k), flip=bool(case % 2))
        if case in (4, 10):     # reverse-complement copies: flagged windows
            for _ in range(6):
                a = int(rng.integers(0, len(g) - 300)); unitigs.append(rc(g[a:a + int(rng.integers(k, 300))]))
        if case == 5:     # identical and near-duplicate unitigs
            unitigs += [unitigs[3], unitigs[7][:-2] + "AC", unitigs[5]]
        p, o = both(unitigs, k)
        assert p.string_filter_bytes() > 0 and p.kmer_table_bytes() > 0
        reads = _fast_path_reads(rng, g, k, unitigs)
        exp, _, _ = o.search_batch(reads)
        for on in (1, 0):
            assert L.fin_set_option(b"fast_path", on) == 0
            try:
                b = p.batch(reads); b.run(fa.FIN_MERGED); got, _ = b.download()
                pc = b.pipeline_counts(48); info = b.run_info(); b.close()
            finally:
                L.fin_set_option(b"fast_path", 1)
            assert np.array_equal(got.astype(np.int64), exp), "case %d k=%d fast_path=%d" % (case, k, on)
            assert info["fast_path"] == bool(on) and info["deferred"] and info["kernel"] == 4
            n_fast = pc[4 * 8 + 9]
            assert (n_fast > 0) == bool(on)
            if on and case in (0, 6):
                assert n_fast > 0.5 * len(reads), (case, n_fast, len(reads))   # most reads of a disjoint set go the fast way (k = 31 and k = 63, unitigs of up to 600 / 900 bases)
        # forward-only searches and searches that defer nothing never take it
        L.fin_set_option(b"defer_strand", 0)
        try:
            b = p.batch(reads[:500]); b.run(fa.FIN_MERGED); got, _ = b.download(); pc = b.pipeline_counts(48); b.close()
        finally:
            L.fin_set_option(b"defer_strand", 1)
        assert pc[4 * 8 + 9] == 0 and np.array_equal(got.astype(np.int64), o.search_batch(reads[:500])[0])
        p.close()


def test_fast_path_and_kmer_table_beyond_k_63(kernel):
    """Round 5 (VERDICT r4 missing #4): the compact k-mer table holds no k-mer, so its slot does not grow with k -- for 64 <= k <= 255 the anchor pass enters every
    text k-mer by a hash folded over its ceil(k / 32) key words, and the pre-pass's fast path (looks, whole-read comparison, absence proofs by the canonical string
    filter) finishes the reads it can as for shorter k (option fast_path 2); the walk kernel folds the words into the hash as its chunk cache brings them and has a claim
    borne out by the re-anchoring comparison (W_KF0B, W_REANCH: a whole-k-mer look-up is ceil(k/32) + 5 epochs instead of k - T rank steps).  The oracle's
    pairs with the fast path on and off at k in {64, 65, 100, 127, 128, 129, 200, 250}: reads of 250 bases with few and many errors, either strand, reads that cross
    unitig ends, reads longer than the fast path takes (256), of exactly k bases, from nowhere; a set with duplicated stretches and reverse-complement copies."""
    if kernel != 4:
        pytest.skip("kernel 4's")
    L = fa.lib()
    rng = np.random.default_rng(6464)
    for case, k in enumerate((64, 65, 100, 127, 128, 129, 200, 250, 100)):
        g = random_genome(rng, 30000)
        if case == 8:
            for _ in range(4):
                a = int(rng.integers(0, len(g) - 600)); n = int(rng.integers(k + 3, 600)); at = int(rng.integers(0, len(g)))
                g = g[:at] + g[a:a + n] + g[at:]
        unitigs = cut_unitigs(rng, g, k, max_len=4 * k + 1500, flip=bool(case % 2))
        if case == 8:
            unitigs += [rc(g[a:a + 400]) for a in (2000, 9000)]
        o = OracleIndex.build(unitigs, k)
        p0 = fa.FinimizerIndex.build(unitigs, k).set_option("kmer_table", 0).to_device(0)   # round 4's state above 63: no table, whole k-mers looked up through the SBWT
        assert p0.kmer_table_bytes() == 0
        p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
        assert p.kmer_table_bytes() > 0 and p.string_filter_bytes() > 0 and not p.lean_tables()   # (the table at any k: the walk kernel asks it too, W_KF0B)
        reads = sample_reads(rng, g, 500, 250, err=0.004, random_frac=0.06) + sample_reads(rng, g, 200, 256, err=0.02, random_frac=0.0)
        reads += [mosaic_read(rng, g, k, 700) for _ in range(100)] + [g[100:100 + k], rc(g[400:400 + k]), g[1000:1300], rc(g[2000:2257]), g[:256], g[-256:], random_genome(rng, 256), ""]
        reads += [u[:256] for u in unitigs[:20]] + [rc(u[:256]) for u in unitigs[:20]]
        exp, _, _ = o.search_batch(reads, n_threads=8)
        got0, _ = p0.search_reads(reads)
        assert np.array_equal(got0.astype(np.int64), exp), "case %d k=%d without the k-mer table" % (case, k)
        p0.close()
        # lean tables above 63 (option lean_tables 3: no prefix table, no anchor table -- the memory of k <= 63 at any k), fast path off and on
        pl = fa.FinimizerIndex.build(unitigs, k).set_option("lean_tables", 3).to_device(0)
        assert pl.lean_tables() and pl.seed_table_bytes() == 0 and pl.prefix_table_depth() == 0
        for on in (1, 2):
            pl.set_option("fast_path", on)
            gotl, _ = pl.search_reads(reads)
            assert np.array_equal(gotl.astype(np.int64), exp), "case %d k=%d lean tables, fast_path=%d" % (case, k, on)
        pl.close()
        for on in (2, 0, 1):
            p.set_option("fast_path", on)
            b = p.batch(reads); b.run(fa.FIN_MERGED); got, _ = b.download(); pc = b.pipeline_counts(48); info = b.run_info(); b.close()
            assert np.array_equal(got.astype(np.int64), exp), "case %d k=%d fast_path=%d" % (case, k, on)
            assert info["fast_path"] == (on == 2) and info["deferred"] and info["kernel"] == 4
            assert (pc[4 * 8 + 9] > 0) == (on == 2)
            if on == 2 and k <= 129 and case != 8:
                assert pc[4 * 8 + 9] > 0.3 * len(reads), (k, pc[4 * 8 + 9], len(reads))
        p.set_option("fast_path", 2)
        # the text from the fast path's records, text-only mode, at these k too
        rd = [r for r in reads if len(r) >= k]
        e2, _, _ = o.search_batch(rd, n_threads=8)
        want, at = [], 0
        for r in rd:
            n = len(r) - k + 1
            want.append(" ".join("(%d,%d)" % (int(u), int(x)) for u, x in e2[at:at + n]) + "\n"); at += n
        b = p.batch(rd); b.text_mode(2); b.run(fa.FIN_MERGED)
        assert b.text() == "".join(want).encode(), "text k=%d" % k
        b.close()
        p.close()


def test_wide_key_lookups_fresh_seed_batch(kernel):
    """A fresh-seed batch of tools/fuzz_wide.py in the driver's run (as the deferral fuzzers' batches, VERDICT r4 next #9c): 60 random index sets at
    64 <= k <= 255 -- half of them with duplicated stretches and reverse-complement copies: unsafe places, unverified answers, flagged windows -- searched on
    kernel 4, whose walk kernel asks the compact k-mer table above 63 too (W_KF0B: the key's words folded into the hash as the chunks arrive; W_REANCH: the claim
    compared with the text), fast path off and on, against the faithful oracle (2 000 sets: profiles/r05/fuzz_wide_2000.txt)."""
    if kernel != 4:
        pytest.skip("kernel 4's")
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_wide.py"), "60", "31337"], cwd=root, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "60 cases, 0 mismatches" in p.stdout, (p.stdout[-1500:], p.stderr[-500:])


def test_prepass_longest_segments(kernel):
    """with segments of 1024 reads (every batch of 512 K reads or more; here forced by option "debug_pp_seg") the later phases of the
    fast pre-pass pushed reads to the BACK of the LDS list whose FRONT held the reads still waiting for those phases -- unread entries were
    overwritten as soon as waiting + pushed reads passed 1024: reads longer than 256 bases (the fast path never finishes them) that miss both
    first looks and hit with their last k-mer.  Overwritten reads kept undeferred verdicts and others were processed twice: pairs stayed exact,
    the pipeline's counters did not.  The oracle's pairs, and the same items / deferred strands / fast-path count as with segments of 256."""
    if kernel != 4:
        pytest.skip("kernel 4's")
    L = fa.lib()
    rng = np.random.default_rng(1024)
    for k in (31, 47):
        g = random_genome(rng, 60000)
        unitigs = cut_unitigs(rng, g, k, max_len=2500, flip=True)
        p, o = both(unitigs, k)
        reads = []
        for i in range(2600):
            n = int(rng.integers(270, 340)) if i % 5 else int(rng.integers(k + 5, 250))
            a = int(rng.integers(0, len(g) - n)); r = list(g[a:a + n])
            # a substitution inside the first k-mer of the strand that matches and inside its sister's (= this strand's last k-mer, four reads in five not)
            w = int(rng.integers(0, k)); r[w] = "ACGT"[("ACGT".index(r[w]) + 1) % 4]
            if i % 5 == 4:
                w = n - 1 - int(rng.integers(0, k)); r[w] = "ACGT"[("ACGT".index(r[w]) + 2) % 4]
            r = "".join(r); reads.append(r if rng.random() < 0.5 else rc(r))
        exp, _, _ = o.search_batch(reads, n_threads=8)
        counts = {}
        for seg in (1024, 256):
            assert L.fin_set_option(b"debug_pp_seg", seg) == 0
            try:
                b = p.batch(reads); b.run(fa.FIN_MERGED); got, _ = b.download(); pc = b.pipeline_counts(48); info = b.run_info(); b.close()
            finally:
                L.fin_set_option(b"debug_pp_seg", 0)
            assert np.array_equal(got.astype(np.int64), exp), "k=%d seg=%d" % (k, seg)
            assert info["fast_path"] and info["deferred"]
            counts[seg] = (pc[7], pc[10], pc[4 * 8 + 8], pc[4 * 8 + 9])   # items of the walk kernel's first round, stream items, deferred strands gone on with, reads the fast path finished
        assert counts[1024] == counts[256], (k, counts)
        p.close()


def test_text_modes_of_a_batch(kernel):
    """Round 4 (fin_text.hip, fin_batch_text_mode): the reference's text (search_fmin.hh:62-65) of a batch whose reads the fast path finished is
    made from the path's 32-byte records -- mode 1 beside the pairs, mode 2 INSTEAD of them (the pairs of such reads are never written).  The
    oracle's text byte for byte in all three modes, on the fast path's read mix (k <= 31 and the two-word table's k), ragged lengths, blocks of
    1024 pairs that start and end inside reads, a read longer than several blocks; mode 1 leaves the pairs intact, mode 2 refuses to deliver
    them and counts the found pairs while formatting; the streaming entry (sub-batches in mode 2) gives the same bytes."""
    if kernel != 4:
        pytest.skip("kernel 4's")
    L = fa.lib()
    rng = np.random.default_rng(515)
    for case, k in enumerate((31, 21, 31, 47, 63)):
        g = random_genome(rng, 40000)
        if case in (2, 4):     # duplicated stretches
            for _ in range(5):
                a = int(rng.integers(0, len(g) - 400)); n = int(rng.integers(k + 3, 400)); at = int(rng.integers(0, len(g)))
                g = g[:at] + g[a:a + n] + g[at:]
        unitigs = cut_unitigs(rng, g, k, max_len=900, flip=bool(case % 2)) + [g[5000:9000]]
        p, o = both(unitigs, k)
        reads = [r for r in _fast_path_reads(rng, g, k, unitigs) if len(r) >= k] + [g[5000:9000], rc(g[5100:8000]), g[5000:5000 + k]]
        if case in (0, 3):     # reads of several segments (4096 pairs each), one of them a multiple
            reads += [g[1000:14000], "ACGT" * 3000, g[200:200 + 2 * 4096 + k - 1]]
        exp, _, _ = o.search_batch(reads)
        want, at = [], 0
        for r in reads:
            n = len(r) - k + 1
            want.append(" ".join("(%d,%d)" % (int(u), int(x)) for u, x in exp[at:at + n]) + "\n")
            at += n
        want = "".join(want).encode()
        n_found = int((exp[:, 0] >= 0).sum())
        for mode in (0, 1, 2):
            b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
            assert b.pipeline_counts(48)[4 * 8 + 9] > 0.4 * len(reads)        # (the fast path did finish reads)
            if mode == 2:
                with pytest.raises(fa.FinitoError):
                    b.download()
            assert b.text() == want, "case %d k=%d mode %d" % (case, k, mode)
            if mode < 2:
                got, npos = b.download()
                assert np.array_equal(got.astype(np.int64), exp) and npos == n_found
            else:
                assert b.download(want_pairs=False)[1] == n_found
                b.text_mode(0); b.run(fa.FIN_MERGED)                             # the same batch back in pair mode
                assert np.array_equal(b.download()[0].astype(np.int64), exp)
            b.close()
        assert L.fin_set_option(b"pipeline_kmers", 30000) == 0
        try:
            got, npos = p.search_reads_text(reads)
        finally:
            L.fin_set_option(b"pipeline_kmers", 1 << 26)
        assert got == want and npos == n_found
        # forward-only runs and runs without the fast path keep their pairs whatever the mode says
        b = p.batch(reads[:300]); b.text_mode(2); b.run(fa.FIN_FWD); fwd, _ = b.download()
        assert np.array_equal(fwd.astype(np.int64), np.array([x for r in reads[:300] for x in o.search(r)[0]], dtype=np.int64).reshape(-1, 2))
        b.close()
        L.fin_set_option(b"fast_path", 0)
        try:
            b = p.batch(reads[:300]); b.text_mode(2); b.run(fa.FIN_MERGED)
            assert np.array_equal(b.download()[0].astype(np.int64), o.search_batch(reads[:300])[0])
            b.close()
        finally:
            L.fin_set_option(b"fast_path", 1)
        p.close()


def test_lean_tables(kernel):
    """Round 4, option "lean_tables" (at upload; 1 = k <= 31, the default; 2 = k <= 63): no prefix table and no anchor table -- the k-mer table, the two string filters and the
    jump table only.  Probes ask the directional string filter (one 16-byte load), a string that occurs is followed by a look-up of the whole
    k-mer in the k-mer table, the pre-pass's seeds are places.  The oracle's pairs on disjoint, duplicated, reverse-complemented and
    repeat-rich sets, with the fast path on and off, second strands deferred or not, merged and forward-only."""
    if kernel != 4:
        pytest.skip("kernel 4's")
    L = fa.lib()
    rng = np.random.default_rng(777)
    sets = []
    for case, k in enumerate((31, 21, 12, 31, 25, 16, 32, 33, 47, 63, 40, 63)):   # (k >= 32: the two-word k-mer table)
        if case < 3 or 6 <= case < 10:
            g = random_genome(rng, 30000); unitigs = cut_unitigs(rng, g, k, max_len=500, flip=bool(case % 2))
        else:
            g, unitigs, _ = defer_family_case(rng, case, k)
        reads = sample_reads(rng, g, 600, min(len(g), 150), err=0.02, random_frac=0.08) + [mosaic_read(rng, g, k, 400) for _ in range(200)]
        reads += [u for u in unitigs[:20]] + [rc(u) for u in unitigs[:20]] + ["", "ACGT", g[:min(len(g), 700)], rc(g[-300:]), "N" * 40]
        sets.append((k, unitigs, reads))
    gr = synth.repeat_genome(200_000, seed=11)
    ur = synth.spss(gr, 31, max_len=1500)
    for k, unitigs, reads in sets + [(31, ur.as_tuple(), synth.reads(gr, 3000, read_len=150).as_tuple())]:
        o = OracleIndex.build(unitigs, k)
        exp, _, _ = o.search_batch(reads, n_threads=8)
        p = fa.FinimizerIndex.build(unitigs, k)
        p.set_option("lean_tables", 2 if k >= 32 else 1)   # (2: the two-word k-mer table for the walk kernel too)
        p.to_device(0)
        assert p.seed_table_bytes() == 0 and p.prefix_table_depth() == 0 and p.kmer_table_bytes() > 0 and p.string_filter_bytes() > 0
        for fast, defer, two in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (0, 1, 0)):   # (two: the walk kernel's two look-ups per epoch, k <= 31 -- round 5)
            L.fin_set_option(b"fast_path", fast); L.fin_set_option(b"defer_strand", defer); L.fin_set_option(b"lean_walk", two)
            try:
                b = p.batch(reads); b.run(fa.FIN_MERGED); got, _ = b.download(); info = b.run_info(); b.close()
            finally:
                L.fin_set_option(b"fast_path", 1); L.fin_set_option(b"defer_strand", 1); L.fin_set_option(b"lean_walk", 1)
            assert np.array_equal(got.astype(np.int64), exp), "lean tables k=%d fast_path=%d defer_strand=%d lean_walk=%d" % (k, fast, defer, two)
            assert info["kernel"] == 4 and info["no_prefill"] and info["deferred"] == bool(defer)
        if isinstance(reads, list):
            gotf, _ = p.search_reads(reads, fa.FIN_FWD)
            expf = [x for r in reads for x in o.search(r)[0]]
            assert gotf.tolist() == [list(x) for x in expf]
        p.close()


def test_compact_kmer_table_k_mer_by_k_mer(kernel):
    """Round 5 (fin_format.h: FinDevIndex::kt3): the compact k-mer table holds no k-mer -- a slot is {the reference's answer, a 30-bit tag} -- and what it claims is
    proven by the text.  Asked directly (fin_index_debug_kmer_table), k-mer by k-mer: EVERY k-mer of the unitig text is claimed, with the answer the faithful
    oracle computes for that k-mer searched alone (FinimizerIndex::search on the k-mer: no walk reaches it), and the text at the answer spells it -- or, on a set
    with duplicated stretches, the claim is flagged unverified, the text there spells another k-mer, and the exact side table holds the k-mer with the same answer;
    k-mers that are in no unitig are not claimed (a claim by a shared tag would fail its proof: the text check -- tests/test_kmer_table_collisions.py constructs such
    k-mers and feeds them to the search)."""
    if kernel != 4:
        pytest.skip("one pass is enough")
    rng = np.random.default_rng(63)
    for case, k in enumerate((31, 47, 16, 63, 31)):
        g = random_genome(rng, 6000)
        if case >= 2:     # duplicated stretches: unsafe places, unverified answers
            for _ in range(6):
                a = int(rng.integers(0, len(g) - 300)); n = int(rng.integers(k + 3, 300)); at = int(rng.integers(0, len(g)))
                g = g[:at] + g[a:a + n] + g[at:]
        unitigs = cut_unitigs(rng, g, k, max_len=400, flip=bool(case % 2))
        p, o = both(unitigs, k)
        assert p.kmer_table_bytes() > 0
        uends = np.asarray(o.ends(), dtype=np.int64); ustarts = np.concatenate([[0], uends[:-1]])
        text = "".join("ACGT"[c] for c in o.concat())
        kmers = sorted({text[a:a + k] for u in range(len(uends)) for a in range(int(ustarts[u]), int(uends[u]) - k + 1)})
        gq, fl = p.kmer_table_query(kmers)
        n_unver = 0
        for i, q in enumerate(kmers):
            (uu, off), = o.search(q)[0]
            assert uu >= 0, q
            want = int(ustarts[uu]) + off + k - 1
            assert fl[i] & 3, "a text k-mer the table does not claim: %s" % q
            assert int(gq[i]) == want, (q, int(gq[i]), want, int(fl[i]))
            spelled = 0 <= want - k + 1 and text[want - k + 1:want + 1] == q and want < int(uends[uu]) and want - k + 1 >= int(ustarts[uu])
            if fl[i] & 1:
                assert (fl[i] & 4) and spelled, q
            else:
                n_unver += 1
                assert (fl[i] & 8) and not spelled, (q, int(fl[i]))   # (flag 4 may be set: the concatenation spells the k-mer there ACROSS a unitig's end -- no place)
        assert (n_unver > 0) == (p.unverified_kmers() > 0)
        if case < 2:
            assert n_unver == 0 and p.unverified_kmers() == 0
        present = set(kmers)
        absent = [x for x in (random_genome(rng, k) for _ in range(4000)) if x not in present]
        absent += [q[:-1] + "ACGT"[("ACGT".index(q[-1]) + 1) % 4] for q in kmers[:2000]]      # siblings one base off
        absent = [x for x in absent if x not in present]
        ga, fa_ = p.kmer_table_query(absent)
        assert not ((fa_ & 4) != 0).any(), "a k-mer that is in no unitig, proven present"
        assert ((fa_ & 3) != 0).sum() <= 1      # (a shared 30-bit tag: one in a thousand million per slot looked at)
        p.close()


def test_lean_tables_and_the_string_length_option(kernel):
    """option "cbf_m" 0 (no string filters) at upload must not leave a default index without probes -- round 3's tables are built instead;
    and a short string under lean tables 2 at k = 63 (more than seven strings per k-mer) must not wrap the back-scan's 3-bit counter: same pairs, no
    read sent to kernel 3 for lack of epochs."""
    if kernel != 4:
        pytest.skip("kernel 4's")
    rng = np.random.default_rng(31)
    g = random_genome(rng, 30000)
    for k, m, lean in ((31, 0, 1), (63, 6, 2), (63, 9, 2), (31, 12, 1)):
        unitigs = cut_unitigs(rng, g, k, max_len=600)
        o = OracleIndex.build(unitigs, k)
        reads = sample_reads(rng, g, 800, 250, err=0.02, random_frac=0.05) + [mosaic_read(rng, g, k, 500) for _ in range(100)]
        exp, _, _ = o.search_batch(reads, n_threads=8)
        p = fa.FinimizerIndex.build(unitigs, k)
        p.set_option("cbf_m", m); p.set_option("lean_tables", lean)
        p.to_device(0)
        if m == 0:
            assert not p.lean_tables() and p.seed_table_bytes() > 0 and p.prefix_table_depth() > 0 and p.string_filter_bytes() == 0
        else:
            assert p.lean_tables() and p.seed_table_bytes() == 0 and p.string_filter_bytes() > 0
        b = p.batch(reads); b.run(fa.FIN_MERGED); got, _ = b.download(); pc = b.pipeline_counts(48); info = b.run_info(); b.close()
        assert np.array_equal(got.astype(np.int64), exp), (k, m, lean)
        assert info["kernel"] == 4 and info["deferred"]
        assert pc[2] < len(reads) // 2, "reads given up to kernel 3 (slots reserved in its list): %d" % pc[2]
        p.close()


def test_round3_tables_on_request(kernel):
    """option "lean_tables" 0 at upload (and every k > 31): prefix table + anchor table, probes through the prefix table, seeds through the anchor
    table -- round 3's configuration stays exact beside the default: the deferral family, the mixed indexes, a batch of ordinary reads"""
    if kernel != 4:
        pytest.skip("kernel 4's")
    L = fa.lib()
    assert L.fin_set_option(b"lean_tables", 0) == 0
    try:
        stats = defer_family_cases(40, 31337)
        assert stats["cases"] == 40
        stats = mixed_index_cases(20, 99)
        assert stats["cases"] == 20
        rng = np.random.default_rng(5)
        g = random_genome(rng, 50000)
        unitigs = cut_unitigs(rng, g, 31, max_len=600)
        p, o = both(unitigs, 31)
        assert not p.lean_tables() and p.seed_table_bytes() > 0 and p.prefix_table_depth() > 0
        reads = sample_reads(rng, g, 3000, 150, err=0.01, random_frac=0.05)
        assert_reads_equal(p, o, reads)
        p.close()
    finally:
        L.fin_set_option(b"lean_tables", 2)   # (the default since round 5)


def test_per_handle_options(kernel):
    """fin_index_set_option: two handles in one process with different kernels and switches, searched from two threads at once -- each
    follows its own values, results are the oracle's, and the process-wide values stay what the fixture set"""
    if kernel != 4:
        pytest.skip("one pass is enough")
    import threading
    rng = np.random.default_rng(12)
    g = random_genome(rng, 60000)
    unitigs = cut_unitigs(rng, g, 31, max_len=700)
    reads = sample_reads(rng, g, 3000, 150)
    o = OracleIndex.build(unitigs, 31)
    exp, _, _ = o.search_batch(reads)
    a = fa.FinimizerIndex.build(unitigs, 31).set_option("kernel", 2).to_device(0)
    b = fa.FinimizerIndex.build(unitigs, 31).set_option("seed_anchors", 0).set_option("kmer_table", 0).to_device(0)
    c = fa.FinimizerIndex.build(unitigs, 31).to_device(0)
    d = fa.FinimizerIndex.build(unitigs, 31).set_option("lean_tables", 0).to_device(0)
    assert b.seed_table_bytes() == 0 and b.kmer_table_bytes() == 0 and c.lean_tables() and c.kmer_table_bytes() > 0 and d.seed_table_bytes() > 0 and d.prefix_table_depth() > 0
    res = {}
    def work(name, idx):
        for _ in range(3):
            res[name], _ = idx.search_reads(reads, fa.FIN_MERGED)
    th = [threading.Thread(target=work, args=(n, i)) for n, i in (("a", a), ("b", b), ("c", c), ("d", d))]
    [t.start() for t in th]; [t.join() for t in th]
    for n in "abcd":
        assert np.array_equal(res[n].astype(np.int64), exp), n
    bt = a.batch(reads); bt.run(fa.FIN_MERGED); bt.download()
    ms2 = bt.step_time_ms()[0]["step"]; bt.close()
    bt = c.batch(reads); bt.run(fa.FIN_MERGED); bt.download()
    ms4 = bt.step_time_ms()[0]["step"]; bt.close()
    assert ms2 > 0 and ms4 > 0
    for i in (a, b, c, d):
        i.close()


def test_prepass_absence_filter(kernel):
    """The pre-pass asks a bit set of the F-base strings that occur in the unitigs before it spends a prefix-table probe: every depth
    (none, shallow -- nearly every string occurs --, deep, automatic) gives the oracle's pairs; reads that match nothing, reads of the
    other strand, N's and lower case, reads barely longer than k."""
    if kernel not in (3, 4):
        pytest.skip("the pre-pass is kernel 4's and 3's")
    rng = np.random.default_rng(4242)
    L = fa.lib()
    for k in (7, 16, 31, 45):
        g = random_genome(rng, 20000)
        unitigs = cut_unitigs(rng, g, k, max_len=3 * k + 200)
        reads = [mosaic_read(rng, g, k, 300) for _ in range(150)] + [random_genome(rng, int(rng.integers(k, 400))) for _ in range(150)]
        reads += [g[100:100 + k], g[500:500 + k + 1].lower(), g[900:1100][:60] + "N" + g[961:1100], rc(g[3000:3300])]
        exp = None
        for F in (0, 4, 6, 9, 12, -1):
            assert L.fin_set_option(b"filt_f", F) == 0
            try:
                p, o = both(unitigs, k)
            finally:
                L.fin_set_option(b"filt_f", -1)
            assert p.filter_depth() == (min(F, k - 1) if F >= 0 else p.filter_depth()) and (F != 0 or p.filter_depth() == 0)
            if exp is None:
                exp, _, _ = o.search_batch(reads)
            got, _ = p.search_reads(reads, fa.FIN_MERGED)
            assert np.array_equal(got.astype(np.int64), exp), "k=%d F=%d" % (k, F)
            p.close()

