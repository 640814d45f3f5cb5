"""The fused ingest (option "fused_ingest"): the fast pre-pass packs the ASCII reads itself instead of the pack kernel, and writes the chunks of
the reads it does not finish.  Its pairs must equal the pack kernel's path and the oracle's, and the chunks it writes must be the pack kernel's
bytes for every read a later kernel may read."""
import numpy as np
import pytest

import finito_amd as fa
from finito_amd import synth
from oracle.oracle import OracleIndex
from tests.util import cut_unitigs, random_genome, rc, sample_reads

pytestmark = pytest.mark.gpu

FIN_PASS_DONE = 0xFFFFFFFD


def _chunk_offsets(reads):
    lens = [len(r) for r in reads]
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    off[1:] = np.cumsum([2 * ((n + 31) // 32) for n in lens])
    return off


def _run(p, reads, fused):
    p.set_option("fused_ingest", fused)
    b = p.batch(reads)
    try:
        b.run(fa.FIN_MERGED)
        got, _ = b.download()
        off = _chunk_offsets(reads)
        did, ch, pv = b.debug_ingest(int(off[-1]))
        info = b.run_info()
    finally:
        b.close()
        p.set_option("fused_ingest", None)
    return got.astype(np.int64), did, ch, pv, off, info


def check(p, o, reads, expect_fused=True):
    """fused 1 == fused 0 == oracle on the pairs; the unfinished reads' chunks byte for byte"""
    got1, did1, ch1, pv1, off, info = _run(p, reads, 1)
    got0, did0, ch0, _, _, _ = _run(p, reads, 0)
    assert info["kernel"] == 4 and info["fast_path"], info
    assert did1 == expect_fused and not did0
    exp, _, _ = o.search_batch(reads)
    assert np.array_equal(got0, exp), "pack-kernel path differs from the oracle"
    assert np.array_equal(got1, exp), "fused ingest differs from the oracle"
    n_checked = 0
    for r in range(len(reads)):
        if pv1[r, 0] == FIN_PASS_DONE and pv1[r, 1] == FIN_PASS_DONE:
            continue   # (finished by the fast path: its chunks are undefined)
        a, e = off[r], off[r + 1]
        assert np.array_equal(ch1[a:e], ch0[a:e]), ("chunks differ", r, reads[r])
        n_checked += 1
    return n_checked, int(((pv1[:, 0] == FIN_PASS_DONE) & (pv1[:, 1] == FIN_PASS_DONE)).sum())


@pytest.fixture(scope="module")
def k31():
    g = synth.genome(200_000)
    u = synth.unitigs(g, 31)
    p = fa.FinimizerIndex.build(u.as_tuple(), 31).to_device(0)
    o = OracleIndex.build(u.as_tuple(), 31)
    yield g, p, o
    p.close()


def _genome_str(g):
    return g.tobytes().decode() if isinstance(g, np.ndarray) else str(g)


def _edge_reads(gs, rng, k):
    reads = []
    for n in sorted({k - 1, k, 31, 32, 33, 63, 64, 65, 150, 255, 256}):
        for _ in range(6):
            a = int(rng.integers(0, len(gs) - n))
            s = gs[a:a + n]
            reads.append(s if rng.random() < 0.5 else rc(s))
    s = gs[1000:1150]
    reads += ["", s, ""]                                                # empty reads beside others
    reads += [s[:10] + "N" + s[11:], s[:140] + "N" + s[141:]]           # a non-ACGT base in the first / the last k-mer
    reads += [s[:75] + "N" + s[76:], "N" * 150, s.lower(), s[:60] + s[60:90].lower() + s[90:]]
    reads += [rc(s)[:5] + "x" + rc(s)[6:], s[:149] + "-"]
    return reads


def test_fast_path_mix_and_edge_reads(k31):
    g, p, o = k31
    rng = np.random.default_rng(61)
    gs = _genome_str(g)
    reads = synth.reads(g, 3000).strings() + _edge_reads(gs, rng, 31)
    n_checked, n_done = check(p, o, reads)
    assert n_done > len(reads) // 2 and n_checked > 0


@pytest.mark.parametrize("seg", [256, 1024])
def test_pre_pass_segments(k31, seg):
    g, p, o = k31
    rng = np.random.default_rng(62 + seg)
    reads = synth.reads(g, 2500, seed=seg).strings() + _edge_reads(_genome_str(g), rng, 31)
    p.set_option("debug_pp_seg", seg)
    try:
        check(p, o, reads)
    finally:
        p.set_option("debug_pp_seg", None)


def test_a_long_read_takes_the_pack_kernel(k31):
    g, p, o = k31
    gs = _genome_str(g)
    reads = synth.reads(g, 500).strings() + [gs[5000:5257]]   # 257 bases: more than one lane packs
    check(p, o, reads, expect_fused=False)


def test_duplicated_kmers():
    """an index whose k-mers repeat and meet their reverse complements (unsafe places, flagged windows)"""
    rng = np.random.default_rng(63)
    base = random_genome(rng, 30_000)
    rep = base[2000:4000]
    g = base + rep + rc(rep) + random_genome(rng, 5000) + rep
    unitigs = cut_unitigs(rng, g, 31, max_len=400)
    p = fa.FinimizerIndex.build(unitigs, 31).to_device(0)
    o = OracleIndex.build(unitigs, 31)
    try:
        reads = sample_reads(rng, g, 1500, 150, err=0.01) + _edge_reads(g, rng, 31)
        check(p, o, reads)
    finally:
        p.close()


def test_k63():
    g = synth.genome(300_000)
    u = synth.unitigs(g, 63)
    p = fa.FinimizerIndex.build(u.as_tuple(), 63).to_device(0)
    o = OracleIndex.from_components(63, p.components())
    try:
        rng = np.random.default_rng(64)
        reads = synth.reads(g, 1500, read_len=250).strings() + _edge_reads(_genome_str(g), rng, 63)
        check(p, o, reads)
    finally:
        p.close()
