"""The base pileup accumulated on the device and the call made from it (include/finito_amd.h: fin_pileup, fin_batch_add_pileup, fin_pileup_call,
fin_search_batch_add_pileup; fin_pileup.hip).

Every comparison is exact integer equality against tests/test_pileup_host.py::pileup_model -- the definition restated in numpy over the pairs fin_search_batch
delivers, the reads, FIN_X_CONCAT and FIN_X_ENDS; it shares no code with the library.  The index is a handful of synthetic unitigs of 100 .. 400 bases; the reads
are built by hand, a few per case of the definition.  Where a case is meant for the fast path's records the test asserts that a read of it has one."""
import ctypes as C

import numpy as np
import pytest
import torch

import finito_amd as fa
from tests.test_pileup_host import KEPT, NOT_STRAIGHT, OFF_UNITIG, TOO_MANY, assert_pileup, call_model, pileup_model
from tests.util import random_genome, rc

pytestmark = pytest.mark.gpu

MISMATCH_LIMITS = (0, 1, 3, 4, 7, 8, 255)   # 0; exactly the count of the reads with 1, 4 and 8 substitutions; one less than those with 4, 5, 8 and 9


def sub(s, at):
    """s with the bases at positions `at` replaced by others"""
    s = list(s)
    for j in at:
        s[j] = "ACGT"[("ACGT".index(s[j]) + 1 + j % 3) % 4]
    return "".join(s)


def both(name, s, bound=False):
    return [(name, s, bound), (name + " rc", rc(s), bound)]


def make_case(k):
    """unitigs and named reads [(case, read, pipeline-bound)]: `bound` marks the cases the fast path does not finish by design"""
    rng = np.random.default_rng(4200 + k)
    lens = [400, 180, 256, 333, 120 + k, 210, 150]   # (no read comes from the last one)
    U = [random_genome(rng, n) for n in lens]
    junk = random_genome(rng, 400)
    reads = []
    # read shapes
    reads += both("L = k", U[0][7:7 + k], True)                      # one slot: not straight whoever finishes it
    reads += both("L = k + 1", U[0][9:9 + k + 1])
    for nk in (63, 64, 65, 129):
        reads += both("nk = %d" % nk, U[3][5:5 + nk + k - 1])
    for L in (63, 64, 65, 129):
        reads += both("L = %d" % L, sub(U[0][200:200 + L], [L // 2] if L >= 2 * k else []), L < k + 1)
    reads += both("a unitig from first to last base", U[2])
    reads += both("a unitig from first to last base, one substitution", sub(U[1], [90]))
    reads += both("past the end into junk", U[1][100:] + junk[:40], True)
    reads += both("before the start out of junk", junk[50:80] + U[5][:90], True)
    reads += both("mosaic", U[0][10:10 + k + 30] + U[3][40:40 + k + 30], True)
    reads += both("insertion", U[3][20:90] + "A" + U[3][90:160], True)
    reads += both("deletion", U[3][30:100] + U[3][101:170], True)
    reads += both("nowhere", junk[100:250], True)
    reads += both("shorter than k", U[0][:k - 1], True)
    reads += [("empty", "", True)]
    # substitutions: a read of 200 bases whose first 100 hold them, so that slots survive behind them at every k
    base = U[0][150:350]
    spaced = {0: [], 1: [120], 4: [3, 40, 80, 198] if k <= 31 else [3, 5, 8, 198], 5: [2, 9, 20, 33, 41], 8: list(range(1, 32, 4)), 9: list(range(1, 36, 4))}
    for n, at in spaced.items():
        reads += both("%d substitutions" % n, sub(base, at), n >= 5)
    reads += both("substitutions closer than k: no slot survives", sub(U[3][100:100 + 3 * k], [k // 2, k // 2 + k - 1, k // 2 + 2 * k - 2]), True)
    reads += both("substitutions closer than k: one slot survives", sub(U[3][100:100 + 2 * k], [k - 1 - 3, 2 * k - 4 + 1]), True)
    reads += both("first and last base", sub(U[5][30:30 + 2 * k + 20], [0, 2 * k + 19]))
    reads += [(n, r.lower(), b) for n, r, b in both("lower case", sub(U[5][10:10 + 2 * k + 40], [k + 5]))]
    n_at = k + 7
    reads += both("N where the read agrees", U[1][20:20 + n_at] + "N" + U[1][21 + n_at:150], True)
    reads += both("N on a substitution", sub(U[1][20:150], [3])[:n_at] + "n" + sub(U[1][20:150], [3])[n_at + 1:], True)
    # a stack for the call: every unitig tiled by overlapping reads of 2 k + 40 bases, three in four of them with the substitutions of a marked copy of the
    # unitig (one every 2 k + 40 bases, so a read holds one or two and k-mers survive beside them)
    step = k + 20
    for s in U[:6]:
        marked = sub(s, list(range(step // 2, len(s), 2 * step)))
        for i, a in enumerate(list(range(0, len(s) - 2 * step, step // 3)) + [len(s) - 2 * step]):
            reads.append(("stack", (marked if i % 4 != 3 else s)[a:a + 2 * step], False))
    return U, reads


class Case:
    def __init__(self, k):
        self.k = k
        self.unitigs, named = make_case(k)
        self.names = [n for n, _, _ in named]; self.reads = [r for _, r, _ in named]; self.bound = [b for _, _, b in named]
        self.p = fa.FinimizerIndex.build(self.unitigs, k).to_device(0)
        self.concat, self.ends = self.p.export(fa.X_CONCAT), self.p.export(fa.X_ENDS)
        self._pairs, self._want = {}, {}

    def pairs(self, strands):
        """fin_search_batch's pairs, computed once per strand mode and left unchanged"""
        if strands not in self._pairs:
            self._pairs[strands] = self.p.search_reads(self.reads, strands)[0]
            self._pairs[strands].setflags(write=False)
        return self._pairs[strands]

    def want(self, strands, mm):
        key = (strands, mm)
        if key not in self._want:
            self._want[key] = pileup_model(self.reads, self.pairs(strands), self.k, self.concat, self.ends, mm)
        return self._want[key]


_CASES = {}


@pytest.fixture(scope="module", params=[31, 63, 65])
def case(request):
    k = request.param
    if k not in _CASES:
        _CASES[k] = Case(k)
    return _CASES[k]


@pytest.fixture(scope="module")
def case31():
    if 31 not in _CASES:
        _CASES[31] = Case(31)
    return _CASES[31]


def test_the_inputs_show_every_case(case31):
    """conditions on the reads, checked on the model: every outcome occurs, kept reads on both strands, the limits separate the reads they are meant to"""
    c = case31
    out = dict(zip(c.names, c.want(fa.FIN_MERGED, 8)[3]))
    assert out["L = k"] == NOT_STRAIGHT and out["L = k + 1"] == KEPT and out["nk = 129 rc"] == KEPT and out["L = 129"] == KEPT
    assert out["a unitig from first to last base"] == KEPT and out["a unitig from first to last base rc"] == KEPT
    assert out["past the end into junk"] == OFF_UNITIG and out["before the start out of junk rc"] == OFF_UNITIG
    for n in ("mosaic", "insertion", "deletion", "nowhere", "shorter than k", "empty", "substitutions closer than k: no slot survives",
              "substitutions closer than k: one slot survives"):
        assert out[n] == NOT_STRAIGHT, n
    assert out["8 substitutions"] == KEPT and out["9 substitutions"] == TOO_MANY and out["9 substitutions rc"] == TOO_MANY
    assert out["N where the read agrees"] == KEPT and out["N on a substitution"] == KEPT and out["lower case rc"] == KEPT
    for mm, kept, dropped in ((0, "0 substitutions", "1 substitutions"), (3, "1 substitutions", "4 substitutions"), (4, "4 substitutions", "5 substitutions"),
                              (7, "5 substitutions", "8 substitutions"), (1, "1 substitutions rc", "first and last base rc")):
        o = dict(zip(c.names, c.want(fa.FIN_MERGED, mm)[3]))
        assert o[kept] == KEPT and o[dropped] == TOO_MANY, mm
    cover, alt = c.want(fa.FIN_MERGED, 8)[:2]
    assert alt.max() >= 3 and cover.max() >= 6 and (cover == 0).any()


PRODUCERS = [   # (what, options, strands, text mode, records expected at k <= 63)
    ("mode 0", {}, fa.FIN_MERGED, 0, False), ("mode 1", {}, fa.FIN_MERGED, 1, True), ("mode 2", {}, fa.FIN_MERGED, 2, True),
    ("forward only", {}, fa.FIN_FWD, 2, False), ("kernel 3", {"kernel": 3}, fa.FIN_MERGED, 2, False), ("fast path off", {"fast_path": 0}, fa.FIN_MERGED, 2, False),
]


@pytest.mark.parametrize("producer", PRODUCERS, ids=[p[0].replace(" ", "_") for p in PRODUCERS])
def test_every_producer_against_the_model(case, producer):
    """text modes 0, 1 and 2, forward-only search, kernel 3, the fast path off; k = 31, 63 and 65 (no records there).  One run, added to an accumulator per
    mismatch limit.  Where the step is meant to leave records every case that is not pipeline-bound by design has a read with a kind-1 record"""
    what, options, strands, mode, want_records = producer
    c = case
    want_records = want_records and c.k <= 63
    for name, v in options.items():
        c.p.set_option(name, v)
    try:
        b = c.p.batch(c.reads); b.text_mode(mode); b.run(strands)
        accs = [c.p.pileup(max_mismatch=mm) for mm in MISMATCH_LIMITS]
        for a in accs:
            a.add(b)
        for mm, a in zip(MISMATCH_LIMITS, accs):
            got = a.download()
            assert_pileup(got, c.want(strands, mm), "k=%d %s max_mismatch=%d" % (c.k, what, mm))
            assert int(got[2].sum()) == len(c.reads)
            a.close()
        info = b.run_info()
        if want_records:
            assert info["fast_path"] and b.pipeline_counts()[41] > 0
            kinds = b.records()[0]["meta"] >> 16
            for name in sorted({n for n, bound in zip(c.names, c.bound) if not bound}):
                assert any(kinds[i] == 1 for i, n in enumerate(c.names) if n == name), "k=%d %s: no read of case '%s' has a kind-1 record" % (c.k, what, name)
        elif mode != 0:   # (a default step in text mode 0 may use the fast path, but leaves no records either)
            assert (b.records()[0]["meta"] >> 16 != 1).all(), "k=%d %s: a kind-1 record where the step leaves none" % (c.k, what)
        b.close()
    finally:
        for name in options:
            c.p.set_option(name, None)


def test_accumulator_twice_reset_streams_other_index(case31):
    c = case31
    w = c.want(fa.FIN_MERGED, 8)
    a = c.p.pileup()
    assert all(a.device_ptrs())
    b = c.p.batch(c.reads); b.text_mode(2); b.run(fa.FIN_MERGED)
    a.add(b).add(b)
    assert_pileup(a.download(), (2 * w[0], 2 * w[1], 2 * w[2]), "added twice")
    assert_pileup(a.download(), (2 * w[0], 2 * w[1], 2 * w[2]), "downloaded twice: the accumulator is left as it is")
    a.reset()
    assert_pileup(a.download(), (0 * w[0], 0 * w[1], 0 * w[2]), "reset")
    # two batches on two non-default streams
    half = len(c.reads) // 2
    pairs = c.pairs(fa.FIN_MERGED)
    nk1 = sum(max(0, len(r) - c.k + 1) for r in c.reads[:half])
    w1 = pileup_model(c.reads[:half], pairs[:nk1], c.k, c.concat, c.ends, 8)
    w2 = pileup_model(c.reads[half:], pairs[nk1:], c.k, c.concat, c.ends, 8)
    assert all(np.array_equal(x + y, z) for x, y, z in zip(w1[:3], w2[:3], w[:3]))
    S, T = torch.cuda.Stream(), torch.cuda.Stream()
    b1 = c.p.batch(c.reads[:half]); b2 = c.p.batch(c.reads[half:])
    b1.text_mode(2); b2.text_mode(0)
    b1.run(fa.FIN_MERGED, stream=S.cuda_stream); b2.run(fa.FIN_MERGED, stream=T.cuda_stream)
    a.add(b1, stream=T.cuda_stream); a.add(b2, stream=S.cuda_stream)
    assert_pileup(a.download(), w, "two batches on two streams")
    a.reset(stream=S.cuda_stream); a.add(b2, stream=T.cuda_stream)
    assert_pileup(a.download(), w2, "reset on one stream, add on another")
    # refusals: a batch that has not run, an accumulator of another index, a limit out of range
    fresh = c.p.batch(c.reads[:3])
    with pytest.raises(fa.FinitoError):
        a.add(fresh)
    other = fa.FinimizerIndex.build([random_genome(np.random.default_rng(1), 300)], 31).to_device(0)
    oa = other.pileup()
    with pytest.raises(fa.FinitoError):
        oa.add(b)
    with pytest.raises(fa.FinitoError):
        _acc_reads_into(c.p, oa, c.reads[:4])
    with pytest.raises(fa.FinitoError):
        c.p.pileup(max_mismatch=256)
    assert_pileup(oa.download(), tuple(np.zeros_like(x) for x in pileup_model([], np.zeros((0, 2)), 31, other.export(fa.X_CONCAT), other.export(fa.X_ENDS), 8)[:3]), "refused adds add nothing")
    for x in (fresh, b, b1, b2, a, oa):
        x.close()
    other.close()


def _acc_reads_into(index, acc, reads):
    """fin_search_batch_add_pileup with an index that is not the accumulator's"""
    err = C.create_string_buffer(512)
    bases, offsets = fa.flatten(reads)
    rc_ = fa.lib().fin_search_batch_add_pileup(index.h, bases.ctypes.data_as(C.c_char_p), offsets.ctypes.data_as(C.POINTER(C.c_uint64)), len(reads), fa.FIN_MERGED, acc.h, err, 512)
    if rc_ != 0:
        raise fa.FinitoError(rc_, err.value.decode())


def assert_variants(got, want, what):
    assert got.dtype == fa.VARIANT_DTYPE and len(got) == len(want), "%s: %d candidates, model %d" % (what, len(got), len(want))
    for f in ("u", "off", "cover", "ref", "alt"):
        assert np.array_equal(got[f], want[f]), "%s: field %s differs" % (what, f)


def test_call(case31):
    """thresholds at equality, no candidates, a capacity one too small, candidates on both sides of block and chunk boundaries of the staged cover"""
    c = case31
    cover, alt = c.want(fa.FIN_MERGED, 8)[:2]
    a = c.p.pileup().add_reads(c.reads)
    m = alt.max(axis=1)
    # a position whose count is exactly min_alt, and one whose share is exactly min_permille
    m_eq = int(m.max()) - 1
    assert m_eq >= 2 and (m == m_eq).any()
    exact = np.nonzero((m >= 1) & (1000 * m % np.maximum(cover, 1) == 0) & (m < cover))[0]
    assert len(exact)
    pm_eq = int(1000 * m[exact[0]] // cover[exact[0]])
    combos = [(2, 200), (m_eq, 0), (m_eq + 1, 0), (1, pm_eq), (1, pm_eq + 1), (0, 0), (1, 0), (1, 1000), (10 ** 6, 0), (0, 1000)]
    n_by = {}
    for tile in (0, 8):   # 8: the cover is staged in chunks of 512 positions, two blocks of the call each
        c.p.set_option("debug_depth_tile", tile)
        try:
            for min_alt, pm in combos:
                want = call_model(cover, alt, c.ends, c.concat, min_alt, pm)
                got = a.call(min_alt, pm)
                assert_variants(got, want, "min_alt=%d permille=%d tile=%d" % (min_alt, pm, tile))
                g = np.concatenate([[0], c.ends[:-1]])[got["u"]] + got["off"]
                assert (np.diff(g) > 0).all()
                n_by[(min_alt, pm)] = len(want)
            if tile:
                g = np.nonzero((m >= 2) & (1000 * m >= 200 * cover))[0]
                assert all(((g >= lo) & (g < hi)).any() for lo, hi in ((0, 256), (256, 512), (512, 768), (768, 1024), (1024, 1280), (1280, len(m))))
                assert_pileup(a.download(), c.want(fa.FIN_MERGED, 8), "download in chunks of 512")
        finally:
            c.p.set_option("debug_depth_tile", None)
    assert n_by[(m_eq, 0)] > n_by[(m_eq + 1, 0)] > 0 and n_by[(1, pm_eq)] > n_by[(1, pm_eq + 1)] and n_by[(10 ** 6, 0)] == 0 and n_by[(0, 0)] == n_by[(1, 0)]
    # capacity
    n = n_by[(2, 200)]
    assert n >= 4
    assert len(a.call(2, 200, cap=n)) == n
    err = C.create_string_buffer(512); cnt = C.c_uint64(0)
    out = np.zeros(n, dtype=fa.VARIANT_DTYPE)
    rc_ = a.L.fin_pileup_call(a.h, 2, 200, out.ctypes.data_as(C.c_void_p), n - 1, C.byref(cnt), err, 512)
    assert rc_ == fa.FIN_ELIMIT and cnt.value == n
    rc_ = a.L.fin_pileup_call(a.h, 2, 200, None, 0, C.byref(cnt), err, 512)
    assert rc_ == fa.FIN_ELIMIT and cnt.value == n
    with pytest.raises(fa.FinitoError):
        a.call(2, 1001)
    assert_pileup(a.download(), c.want(fa.FIN_MERGED, 8), "the call leaves the accumulator as it is")
    a.close()


def test_device_against_host(case):
    """fin_search_batch_add_pileup over several sub-batches = Pileup.add on one batch = records_pileup on the downloaded records = the model"""
    c = case
    w = c.want(fa.FIN_MERGED, 8)
    c.p.set_option("pipeline_kmers", 2000)
    try:
        assert sum(max(0, len(r) - c.k + 1) for r in c.reads) > 3 * 2000
        a = c.p.pileup().add_reads(c.reads)
        assert_pileup(a.download(), w, "k=%d add_reads in sub-batches" % c.k)
        a.reset().add_reads(c.reads, fa.FIN_FWD)
        assert_pileup(a.download(), c.want(fa.FIN_FWD, 8), "k=%d add_reads, forward only" % c.k)
    finally:
        c.p.set_option("pipeline_kmers", None)
    b = c.p.batch(c.reads); b.text_mode(2); b.run(fa.FIN_MERGED)
    a.reset().add(b)
    assert_pileup(a.download(), w, "k=%d one batch" % c.k)
    recs, stream = b.records()
    assert ((recs["meta"] >> 16 == 1).any()) == (c.k <= 63)
    assert_pileup(fa.records_pileup(recs, stream, c.k, c.reads, c.ends, c.concat, max_mismatch=8, n_threads=16), w, "k=%d host twin on the downloaded records" % c.k)
    a.close(); b.close()
