"""Every pipelined entry point against itself: what a read set gives when the pipeline cuts it into many sub-batches (a small per-index `pipeline_kmers`, one
worker or three) must equal, bit for bit, what it gives as ONE sub-batch (default options).  One table over every product the pipeline hands a sub-batch to --
pairs, text, records, segments, summaries, screen, classes, pseudoalignment (single and paired), the accumulators' add_reads and the unitig_* one-shots --, so
that a product which lands at the wrong reads, in the wrong order or in another product's place shows here whatever the per-feature tests cover.  The
expectation is the same entry point's own one-sub-batch result: this file checks the pipeline's placement, the per-feature tests check the values."""
import numpy as np
import pytest

import finito_amd as fa
from tests.util import cut_unitigs, random_genome, rc

pytestmark = pytest.mark.gpu

K = 31
N_COLORS = 70            # two words per row
N_READS = 150            # a screen bitmap of three words
# (pipeline_kmers, pipeline_depth): about eight sub-batches of some twenty reads with one worker and with three, and one sub-batch per read or two
CUTS = [(1001, 1), (1001, 3), (89, 3)]


def cut(lens, limit, group):
    """the first read of every sub-batch: groups of `group` reads are taken while their k-mers fit `limit`, the first group always"""
    starts, lo, n = [], 0, len(lens)
    while lo < n:
        starts.append(lo)
        h, nk = lo, 0
        while h < n:
            g = sum(max(int(l) - K + 1, 0) for l in lens[h:h + group])
            if h > lo and nk + g > limit:
                break
            nk += g
            h = min(h + group, n)
        lo = h
    return starts


class World:
    def __init__(self):
        rng = np.random.default_rng(2900)
        g = random_genome(rng, 3000)
        self.unitigs = cut_unitigs(rng, g, K, max_len=400)
        self.p = fa.FinimizerIndex.build(self.unitigs, K).to_device(0)
        nu = self.p.n_unitigs
        bits = rng.integers(0, 1 << 63, (nu, 2), dtype=np.uint64)
        bits[:, 1] &= np.uint64((1 << (N_COLORS - 64)) - 1)
        self.colors = self.p.colors(N_COLORS, bits)
        lab = (np.arange(nu) % 3).astype(np.uint32)
        lab[nu // 2] = fa.FIN_NO_LABEL
        self.labels = self.p.labels(lab, 3)
        # two reads without k-mers first (a sub-batch of no k-mers under the smallest limit: the third read alone exceeds it), then found, mutated and foreign reads
        reads = [g[5:5 + K - 1], "ACGT"]
        reads.append(g[100:100 + K + 89])
        while len(reads) < N_READS:
            n = int(rng.integers(40, 121))
            a = int(rng.integers(0, len(g) - n + 1))
            r, kind = g[a:a + n], len(reads) % 3
            if kind == 1:
                r = list(r)
                for i in rng.choice(n, 2, replace=False):
                    r[i] = "ACGT"[("ACGT".index(r[i]) + 1) % 4]
                r = "".join(r)
            elif kind == 2 and rng.random() < 0.5:
                r = random_genome(rng, n)
            reads.append(r if rng.random() < 0.5 else rc(r))
        self.reads = reads
        self.lens = [len(r) for r in reads]
        self.want = {name: flat(f(self)) for name, f in PRODUCTS.items()}

    def close(self):
        self.labels.close()
        self.colors.close()
        self.p.close()


def accumulated(make, add, download=lambda a: a.download()):
    def run(w):
        a = make(w)
        try:
            add(a, w)
            return download(a)
        finally:
            a.close()
    return run


PRODUCTS = {
    "pairs": lambda w: w.p.search_reads(w.reads),
    "text": lambda w: w.p.search_reads_text(w.reads[2:]),   # (it refuses a read without k-mers)
    "records": lambda w: w.p.search_reads_records(w.reads),
    "segments": lambda w: w.p.search_reads_segments(w.reads),
    "summaries": lambda w: w.p.search_reads_summaries(w.reads),
    "screen": lambda w: w.p.screen_reads(w.reads, min_found=1, min_permille=900),
    "classify": lambda w: w.p.classify_reads(w.reads, w.labels),
    "pseudoalign": lambda w: w.p.pseudoalign_reads(w.reads, w.colors, permille=500),
    "pseudoalign_pairs": lambda w: w.p.pseudoalign_pairs(w.reads, w.colors, permille=500),
    "hits": accumulated(lambda w: w.p.hits(), lambda a, w: a.add_reads(w.reads)),
    "cover": accumulated(lambda w: w.p.cover(), lambda a, w: a.add_reads(w.reads)),
    "depth": accumulated(lambda w: w.p.depth(), lambda a, w: a.add_reads(w.reads)),
    "colors": accumulated(lambda w: w.p.colors(N_COLORS), lambda a, w: a.add_reads(w.reads, N_COLORS - 1)),
    "labels": accumulated(lambda w: w.p.labels(np.arange(w.p.n_unitigs) % 3, 3), lambda a, w: a.add_reads(w.reads)),
    "eqclasses": accumulated(lambda w: w.colors.eqclasses(1 << 10), lambda a, w: a.add_reads(w.reads, permille=500)),
    "eqclasses_pairs": accumulated(lambda w: w.colors.eqclasses(1 << 10), lambda a, w: a.add_read_pairs(w.reads, permille=500)),
    "unitig_counts": lambda w: w.p.unitig_counts(w.reads),
    "unitig_coverage": lambda w: w.p.unitig_coverage(w.reads),
    "unitig_depth": lambda w: w.p.unitig_depth(w.reads),
}
PAIRED = ("pseudoalign_pairs", "eqclasses_pairs")


def flat(result):
    """a result as bytes and numbers that compare with =="""
    parts = result if isinstance(result, tuple) else (result,)
    return [np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else x for x in parts]


@pytest.fixture(scope="module")
def w():
    world = World()
    yield world
    world.close()


def test_the_reads_show_what_they_must(w):
    assert 4 <= w.p.n_unitigs <= 40 and w.colors.words == 2 and (N_READS + 63) // 64 == 3
    assert sum(l < K for l in w.lens) == 2 and all(40 <= l <= 120 for l in w.lens[2:])
    summ, _ = w.p.search_reads_summaries(w.reads)
    nk = np.maximum(np.array(w.lens) - K + 1, 0)
    assert (summ["n_found"] == nk)[2:].any() and (summ["n_found"] == 0)[2:].any() and ((summ["n_found"] > 0) & (summ["n_found"] < nk)).any()
    scr = np.frombuffer(w.want["screen"][0], dtype=bool)
    assert scr.any() and not scr.all()
    for limit, _ in CUTS:
        starts = cut(w.lens, limit, 1)
        assert len(starts) >= 5 and sum(s % 64 != 0 for s in starts) >= 4
        assert any(s & 1 for s in starts), "cut read by read, no sub-batch would split a pair"
        assert all(s % 2 == 0 for s in cut(w.lens, limit, 2)) and len(cut(w.lens, limit, 2)) >= 5
        assert len(cut(w.lens[2:], limit, 1)) >= 5
    assert cut(w.lens, 89, 1)[:2] == [0, 2] and cut(w.lens, 89, 2)[:2] == [0, 2], "the sub-batch of no k-mers"


@pytest.mark.parametrize("limit,depth", CUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", list(PRODUCTS))
def test_many_sub_batches_give_what_one_gives(w, name, limit, depth):
    w.p.set_option("pipeline_kmers", limit).set_option("pipeline_depth", depth)
    try:
        got = flat(PRODUCTS[name](w))
    finally:
        w.p.set_option("pipeline_kmers", None).set_option("pipeline_depth", None)
    want = w.want[name]
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "%s: part %d of the result differs under pipeline_kmers=%d, pipeline_depth=%d" % (name, i, limit, depth)
