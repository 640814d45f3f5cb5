"""The device scans and compactions PAST THEIR FIRST LEVEL: the sizes at which a thread of a one-block scan carries more than one block, a second chunk
begins, or a grid-stride loop makes its second trip.  Every other test stays below them; an off-by-one in `b0 + i < n_blk`, a chunk base that is not added or a
32-bit carry would shift offsets only for batches of the size real users run.

| kernel                                                        | first level ends at     | reached here by                                                        |
| fin_blk_scan_kernel (fin_records.hip) over records' blocks    | 1 048 576 reads         | N = 1 050 923 reads: 1027 blocks, per = 2, thread 513 has one block    |
| fin_blk_scan_kernel over segments' blocks (screen's ids too)  | 262 144 reads           | the same N: 4106 blocks, per = 5, thread 821 has one; 300 000 real reads |
| fin_text_scan1/2 over segments (text from records)            | 1 048 576 reads         | the same N: 257 chunks, per = 2 in scan2, n_found over 257 chunks      |
| fin_text_scan1/2 over pair blocks (text from pairs)           | 4 194 304 pairs         | the same N in text mode 0: more than 4097 blocks, chunk_base[1] != 0   |
| fin_depth_tile_scan_kernel (fin_depth.hip), tile 4096         | 4 194 304 positions     | a 4.5 Mbp index: more than 1024 tiles, per = 2                         |
| the same kernel's carry between chunks of 4096 tiles          | 16 777 216 positions    | a 17 Mbp index: two chunks, per = 4 in the first                       |
| fin_set_merge_kernel (fin_records.hip), 65 536 blocks of 256  | 16 777 216 pairs        | 145 000 reads of 150 bases on a partitioned index: 17 400 000 pairs    |

The read-count group runs on HAND-MADE records and pairs (fin_batch_set_records / fin_batch_set_pairs over a real run of the same reads), made vectorised in numpy
from drawn parameters; what they mean is `expand_vec`, a vectorised restatement of tests/test_records.py::brute_expand.  Every expectation is plain numpy over
those pairs -- vectorised restatements of tests/test_segments_host.py::segments_of, tests/test_read_summary_host.py::summaries_of and ::rule,
tests/test_read_class_host.py::classes_of and ::assigned, oracle.oracle.format_pairs -- and the guard test (no GPU) holds each restatement against its original
on a sample of 5 000 reads that includes the first and last read of every block at a `per` boundary.  Nothing is expected from fin_expand_*, fin_records_* or a
device output; every comparison is exact equality.  The run at N itself (random reads) is not compared with anything: only its overwritten content is.  One real
run of 300 000 genome reads keeps the producer in the loop against the oracle.  The classes' tally of the injected batch is taken with Labels.add (add_reads
would search the reads' own content); Labels.add_reads runs on the real run's reads, against the oracle's pairs.

The depth case compares with the generator's GROUND TRUTH (finito_amd/csrc/fin_synth.cpp: fin_synth_check's rule restated in numpy, `truth_pairs`), not the
oracle: the oracle needs half a minute to build a 4.5 Mbp index.  A k-mer with a substituted base, or of a random read, counts as absent: that it lies in a
genome of n bases by chance has probability 2 n / 4^31 per k-mer: 5e-6 at 4.5 Mbp and 2e-5 at 17 Mbp over the 2.4e6 k-mers of the test.  The 17 Mbp case
has two chunks at tile 4096: the carry between chunks at the production tile size, and per = 4 in the first chunk.

Out of reach at test sizes, not attempted:
  * the grid cap of the flat hits / cover / depth kernels (65 536 blocks of 4 waves of 4096 slots): about 1.07e9 pairs;
  * fin_text_scan2_kernel with per >= 2 over pair blocks (more than 256 chunks of 4096 blocks of 1024 pairs): about 1.07e9 pairs;
  * any sum beyond 2^32.

Times on an MI355X, as measured (pytest --durations; the numpy references are made once per module and shared, the first GPU test of the read-count group
pays for them in its setup): the 17 GPU tests together 6.3 s.  Setup of the module's input 1.1 s; test_set_merge_past_its_grid 1.0 s;
test_one_real_run_past_the_segment_threshold 0.7 s; test_depth_past_one_scan_thread_per_tile 0.3 s (4.5 Mbp) and 0.7 s (17 Mbp; build on the device plus upload
took 0.07 s and 0.05 s, which the test prints); test_text_past_one_chunk 0.55 / 0.03 / 0.04 s (modes 1, 2, 0); test_segments_past_one_block_a_thread
0.44 / 0.01 / 0.02 s; test_classes_and_tally_at_this_size 0.38 / 0.04 s; test_records_and_stream_past_one_block_a_thread 0.09 / 0.13 s;
test_screen_ids_past_one_block_a_thread 0.03 s each.  The guard test takes 11 s on a slow CPU."""
import time
from types import SimpleNamespace

import numpy as np
import pytest

import finito_amd as fa
from finito_amd import synth
from oracle.oracle import OracleIndex, format_pairs
from tests.test_read_class_host import NONE, assert_classes, classes_of, tally_of
from tests.test_read_summary_host import assert_summaries, rule, summaries_of
from tests.test_records import brute_expand
from tests.test_records_device import GARBAGE, device_form
from tests.test_segments_host import assert_segments, segments_of
from tests.test_unitig_depth import Want, assert_depth
from tests.util import cut_unitigs, random_genome, unpack_bits

K = 16
N = 1_050_923
REC_BLK, SGM_BLK, TEXT_CHUNK, TEXT_PAIRS = 1024, 256, 4096, 1024       # fin_records.hip, fin_segments.hip / fin_readsum.hip, fin_text.hip
ONLY_FINISHED, ONLY_SEARCHED, BOUNDARY = (5, 511, 700), (6, 512, 701), (1024, 1025, 1026)   # record blocks of 1024 reads
N_LABELS = 300
SCREENS = [(0, 0), (1, 1000), (10, 0)]   # (min_found, min_permille): every read passes; the reads whose slots are all found; none (a read has at most 9)
RULES = [(1, 0, 0), (1, 0, 1), (3, 500, 0), (0, 1000, 0)]   # (min_found, min_permille, min_margin)


# ---- what a record set means, and every consumer's definition, vectorised: reads of at most a few dozen k-mers as rows of a matrix --------------------------
def expand_vec(recs, stream, k):
    """tests/test_records.py::brute_expand without the loop: int32 [n_kmers, 2]"""
    nk = recs["nk"].astype(np.int64); n = len(recs)
    W = int(nk.max(initial=0))
    i = np.arange(W, dtype=np.int64)[None, :]
    valid = i < nk[:, None]
    meta = recs["meta"].astype(np.int64)
    kind, rev, nE = meta >> 16, ((meta >> 8) & 1).astype(bool), meta & 0xFF
    sl = np.where(rev[:, None], nk[:, None] - 1 - i, i)
    gap = np.zeros((n, W), dtype=bool)
    for e in range(8):
        E = ((recs["Es"] if e < 4 else recs["Es2"]) >> np.uint64(16 * (e & 3))).astype(np.int64) & 0xFFFF
        gap |= (e < nE)[:, None] & (sl <= E[:, None]) & (E[:, None] <= sl + k - 1)
    gap |= (kind == 2)[:, None]
    U = np.where(gap, -1, recs["u"].astype(np.int64)[:, None] + 0 * i)
    O = np.where(gap, -1, recs["off0"].astype(np.int64)[:, None] + sl)
    m0 = valid & (kind == 0)[:, None]
    stream = np.asarray(stream, dtype=np.int64).reshape(-1, 2)
    assert int(m0.sum()) == len(stream)
    U[m0] = stream[:, 0]; O[m0] = stream[:, 1]
    return np.stack([U[valid], O[valid]], axis=1).astype(np.int32)


def dense(pairs, nks):
    """(U, O, valid) [n_reads, max nk]: read r's slot i in row r, column i; -1 beyond the read"""
    nks = np.asarray(nks, dtype=np.int64)
    W = int(nks.max(initial=0))
    valid = np.arange(W, dtype=np.int64)[None, :] < nks[:, None]
    U = np.full((len(nks), W), -1, dtype=np.int64); O = np.full((len(nks), W), -1, dtype=np.int64)
    U[valid] = pairs[:, 0]; O[valid] = pairs[:, 1]
    return U, O, valid


def segments_vec(pairs, nks):
    """tests/test_segments_host.py::segments_of without the loop: ((seg_offs, segs), the per-read summaries of tests/test_read_summary_host.py::summaries_of)"""
    U, O, valid = dense(pairs, nks)
    n, W = U.shape
    found = valid & (U != -1)
    link = np.zeros((n, W), dtype=np.int64)
    both = found[:, 1:] & found[:, :-1] & (U[:, 1:] == U[:, :-1])
    d = O[:, 1:] - O[:, :-1]
    link[:, 1:] = np.where(both & (d == 1), 1, np.where(both & (d == -1), -1, 0))
    before = np.zeros((n, W), dtype=np.int64); before[:, 1:] = link[:, :-1]
    head = found & ((link == 0) | ((before != 0) & (before != link)))
    stop = head | ~found                      # (a column beyond the read is not found: the read's end stops a segment)
    nxt = np.full((n, W), W, dtype=np.int64)  # the first stop behind column j
    cur = np.full(n, W, dtype=np.int64)
    for j in range(W - 1, -1, -1):
        nxt[:, j] = cur
        cur = np.where(stop[:, j], j, cur)
    col = np.arange(W, dtype=np.int64)[None, :] + np.zeros((n, 1), dtype=np.int64)
    cnt = nxt - col
    after = np.zeros((n, W), dtype=np.int64); after[:, :-1] = link[:, 1:]
    ln = np.where(cnt > 1, cnt * after, 1)
    segs = np.zeros(int(head.sum()), dtype=fa.SEGMENT_DTYPE)
    segs["u"], segs["off"], segs["slot"], segs["len"] = U[head], O[head], col[head], ln[head]
    seg_offs = np.concatenate([[0], np.cumsum(head.sum(axis=1))]).astype(np.uint64)
    summ = np.zeros(n, dtype=fa.READ_SUMMARY_DTYPE)
    summ["n_found"] = found.sum(axis=1)
    summ["n_segments"] = head.sum(axis=1)
    summ["longest"] = np.where(head, np.abs(ln), 0).max(axis=1, initial=0)
    first, last = np.argmax(found, axis=1), W - 1 - np.argmax(found[:, ::-1], axis=1)
    summ["span"] = np.where(found.any(axis=1), last - first + 1, 0)
    return (seg_offs, segs), summ


def rule_vec(summ, nks, min_found, min_permille, invert):
    nf = summ["n_found"].astype(np.int64)
    return ((nf >= min_found) & (1000 * nf >= min_permille * np.asarray(nks, dtype=np.int64))) != bool(invert)


def classes_vec(pairs, nks, labels):
    """tests/test_read_class_host.py::classes_of without the loop"""
    U, _, valid = dense(pairs, nks)
    lab = np.asarray(labels, dtype=np.int64)
    L = np.where(U >= 0, lab[np.maximum(U, 0)], NONE)
    ok = valid & (L != NONE)
    W = U.shape[1]
    cnt = np.zeros(U.shape, dtype=np.int64)
    for j in range(W):
        cnt += ok & ok[:, j:j + 1] & (L == L[:, j:j + 1])
    n_best = cnt.max(axis=1, initial=0)
    best = np.where(ok & (cnt == n_best[:, None]), L, NONE).min(axis=1, initial=NONE)   # a tie goes to the smaller label
    out = np.zeros(len(U), dtype=fa.READ_CLASS_DTYPE)
    out["label"], out["n_best"], out["n_labelled"] = best, n_best, ok.sum(axis=1)
    out["n_second"] = np.where(ok & (L != best[:, None]), cnt, 0).max(axis=1, initial=0)
    return out


def tally_vec(classes, nks, n_labels, min_found, min_permille, min_margin):
    """tests/test_read_class_host.py::tally_of without the loop"""
    nb, ns = classes["n_best"].astype(np.int64), classes["n_second"].astype(np.int64)
    yes = (nb >= max(min_found, 1)) & (1000 * nb >= min_permille * np.asarray(nks, dtype=np.int64)) & (nb >= ns + min_margin)
    return np.bincount(np.where(yes, classes["label"].astype(np.int64), n_labels), minlength=n_labels + 1).astype(np.uint64)


def _digits(v):
    return 1 + sum((v >= 10 ** t).astype(np.int64) for t in range(1, 10))


def text_vec(pairs, nks):
    """oracle.oracle.format_pairs of every read, back to back, without the loop: (uint8 text, int64 first byte of every pair and the text's length)"""
    u, o = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    found = u >= 0
    nu, no = np.where(found, _digits(u), 2), np.where(found, _digits(o), 2)
    ln = nu + no + 4
    end = np.cumsum(ln); start = end - ln
    out = np.zeros(int(end[-1]), dtype=np.uint8)
    sep = np.full(len(u), ord(" "), dtype=np.uint8); sep[np.cumsum(np.asarray(nks, dtype=np.int64)) - 1] = ord("\n")
    out[start] = ord("("); out[start + 1 + nu] = ord(","); out[end - 2] = ord(")"); out[end - 1] = sep
    a = start[~found]
    out[a + 1] = ord("-"); out[a + 2] = ord("1"); out[a + 4] = ord("-"); out[a + 5] = ord("1")
    for v, nd, at in ((u, nu, start + 1), (o, no, start + 2 + nu)):
        for t in range(10):
            m = found & (nd > t)
            if not m.any():
                break
            out[at[m] + t] = ord("0") + (v[m] // 10 ** (nd[m] - 1 - t)) % 10
    return out, np.concatenate([start, end[-1:]])


def assert_text(got, want, what):
    """as tests/test_records_device.py reports it: the first differing byte and its line"""
    g = np.frombuffer(got, dtype=np.uint8)
    if len(g) == len(want) and np.array_equal(g, want):
        return
    m = min(len(g), len(want))
    bad = np.nonzero(g[:m] != want[:m])[0]
    i = int(bad[0]) if len(bad) else m
    raise AssertionError("%s: text of %d bytes, expected %d; first difference at byte %d (line %d): got %r, want %r" %
                         (what, len(g), len(want), i, int((want[:i] == ord("\n")).sum()), bytes(g[max(0, i - 30):i + 30]), bytes(want[max(0, i - 30):i + 30])))


def assert_screen(got, want_rule, what):
    ids, bits = got
    n = len(want_rule)
    assert ids.dtype == np.uint32 and bits.dtype == np.uint64 and len(bits) == (n + 63) // 64, what
    want_ids = np.nonzero(want_rule)[0]
    assert len(ids) == len(want_ids), "%s: %d ids, expected %d" % (what, len(ids), len(want_ids))
    bad = np.nonzero(ids != want_ids)[0]
    assert len(bad) == 0, "%s: ids differ from entry %d on: got %s, want %s" % (what, bad[0], ids[bad[0]:bad[0] + 4], want_ids[bad[0]:bad[0] + 4])
    every = unpack_bits(bits, 64 * len(bits))
    assert np.array_equal(every[:n].astype(bool), want_rule), "%s: bits" % what
    assert not every[n:].any(), "%s: a bit at or beyond n_reads is set" % what


# ---- the read-count group's input ---------------------------------------------------------------------------------------------------------------------------------
_CASE = None


def case():
    """made once and shared; nobody changes it.  reads = (bases, offsets); recs in the form fin_batch_download_records delivers (a kind-0 record is
    {0, 0, 0, nk, 0, 0}); stream = the kind-0 reads' pairs; pairs = expand_vec(recs, stream)"""
    global _CASE
    if _CASE is not None:
        return _CASE
    rng = np.random.default_rng(20261)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, K, max_len=120)
    ends = OracleIndex.build(unitigs, K).ends().astype(np.int64)
    kmers = np.diff(np.concatenate([[0], ends])) - K + 1
    nks = rng.integers(1, 10, N).astype(np.int64)                     # reads of 16 .. 24 bases: none without k-mers (the text entry refuses those)
    offsets = np.concatenate([[0], np.cumsum(nks + K - 1)]).astype(np.uint64)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(offsets[-1]))]   # their content is free: it only fixes nk
    kind = (rng.random(N) < 0.7).astype(np.int64)
    for blk in ONLY_FINISHED:
        kind[REC_BLK * blk:REC_BLK * (blk + 1)] = 1
    for blk in ONLY_SEARCHED:
        kind[REC_BLK * blk:REC_BLK * (blk + 1)] = 0
    one = kind == 1
    big = np.nonzero(kmers >= 17)[0]                                  # room for nine slots from any offset drawn below
    # the finished reads: forward or reverse, zero or one ruled-out position, inside a unitig -- at its first k-mer, with the last slot on its last, or between
    u = big[rng.integers(0, len(big), N)]
    room = kmers[u] - nks
    t = rng.random(N)
    off0 = np.where(t < 0.25, 0, np.where(t < 0.5, room, (rng.random(N) * (room + 1)).astype(np.int64)))
    rev, nE = rng.integers(0, 2, N), rng.integers(0, 2, N)
    E = (rng.random(N) * (nks + K - 1)).astype(np.int64)              # 0 .. nk + k - 2
    recs = np.zeros(N, dtype=fa.RECORD_DTYPE)
    recs["nk"] = nks
    recs["u"][one], recs["off0"][one] = u[one], off0[one]
    recs["meta"][one] = (nE | (rev << 8) | (1 << 16))[one]
    recs["Es"][one] = np.where(nE == 1, E, 0)[one]
    # the searched reads: two pieces, each absent, an ascending run, a descending run or one pair repeated
    W = 9
    i = np.arange(W, dtype=np.int64)[None, :]
    cut = np.minimum(rng.integers(0, 10, N), nks)[:, None]
    in_b = i >= cut
    j = np.where(in_b, i - cut, i)
    pick = lambda a, b: np.where(in_b, b[:, None], a[:, None])
    tp = pick(rng.choice(4, N, p=[0.25, 0.3, 0.3, 0.15]), rng.choice(4, N, p=[0.25, 0.3, 0.3, 0.15]))
    ua, ub = big[rng.integers(0, len(big), N)], big[rng.integers(0, len(big), N)]
    aa, ab = (rng.random(N) * (kmers[ua] - 8)).astype(np.int64), (rng.random(N) * (kmers[ub] - 8)).astype(np.int64)   # a .. a + 8 are offsets of k-mers
    uu, a0 = pick(ua, ub), pick(aa, ab)
    off = np.where(tp == 1, a0 + j, np.where(tp == 2, a0 + 8 - j, a0))
    U, O = np.where(tp == 0, -1, uu), np.where(tp == 0, -1, off)
    m0 = (i < nks[:, None]) & (kind == 0)[:, None]
    stream = np.stack([U[m0], O[m0]], axis=1).astype(np.int32)
    pairs = expand_vec(recs, stream, K)
    labels = (np.arange(len(unitigs)) % N_LABELS).astype(np.uint32); labels[::17] = NONE
    for a in (ends, nks, offsets, bases, recs, stream, pairs, labels):
        a.setflags(write=False)
    _CASE = SimpleNamespace(k=K, genome=g, unitigs=unitigs, ends=ends, kmers=kmers, reads=(bases, offsets), nks=nks, at=np.concatenate([[0], np.cumsum(nks)]),
                            kind=kind, recs=recs, stream=stream, pairs=pairs, labels=labels, memo={})
    return _CASE


def want(name):
    """the expectations over case().pairs, each made once"""
    c = case()
    if name not in c.memo:
        if name in ("segments", "summaries"):
            c.memo["segments"], c.memo["summaries"] = segments_vec(c.pairs, c.nks)
        elif name == "classes":
            c.memo[name] = classes_vec(c.pairs, c.nks, c.labels)
        elif name == "text":
            c.memo[name] = text_vec(c.pairs, c.nks)
        elif name == "found":
            c.memo[name] = int((c.pairs[:, 0] != -1).sum())
    return c.memo[name]


def take(c, idx):
    """reads idx (ascending) as a record set of their own: (recs, stream, pairs, nks)"""
    rows = np.concatenate([np.arange(c.at[r], c.at[r + 1]) for r in idx])
    zero = np.repeat(c.kind[idx] == 0, c.nks[idx])
    return c.recs[idx], c.pairs[rows][zero], c.pairs[rows], c.nks[idx]


def sample_reads_of(c, rng):
    """5 000 read numbers: the first and last read of every block at a `per` boundary of the three one-block scans, reads 0 and N - 1, and a random draw"""
    edge = {0, N - 1}
    for blk, blocks in ((REC_BLK, [0, 1, 2, 3] + list(range(1021, 1027))), (SGM_BLK, list(range(0, 11)) + list(range(4095, 4106))),
                        (TEXT_CHUNK, [0, 1, 2, 3, 252, 253, 254, 255, 256])):
        for b in blocks:
            edge |= {blk * b, min(blk * (b + 1), N) - 1}
    rest = rng.choice(N, 5000 - len(edge), replace=False)
    idx = np.unique(np.concatenate([np.array(sorted(edge)), rest]))
    return idx


def test_the_generator_and_the_vectorised_definitions():
    """a guard on the input and on this file's own references, not on the device: the thresholds the batch is sized for, the conditions the records must meet
    (those of tests/test_records_host.py::assert_generator_conditions that apply to records of zero or one position), and every vectorised definition against
    its per-read original on a sample of 5 000 reads"""
    c = case()
    fa.lib()
    L = fa.C.CDLL(fa._LIBPATH)   # a handle of this test's own: the prototypes set below stay off the package's
    n_pairs = len(c.pairs)
    # the thresholds: a changed constant fails here instead of emptying the tests
    assert N % 64 and N % 256 and N % 1024
    assert (N + REC_BLK - 1) // REC_BLK == 1027 == L.fin_rec_blocks(N) and (1027 + 1023) // 1024 == 2                   # per = 2: thread 513 takes block 1026 alone
    assert (N + SGM_BLK - 1) // SGM_BLK == 4106 == L.fin_sgm_blocks(N) == L.fin_rsm_blocks(N) and (4106 + 1023) // 1024 == 5 and 4106 % 5 == 1
    L.fin_text3_off_words.restype = L.fin_text_off_words.restype = fa.C.c_uint64
    L.fin_text3_off_words.argtypes = L.fin_text_off_words.argtypes = L.fin_text_blocks.argtypes = [fa.C.c_uint64]
    assert (N + TEXT_CHUNK - 1) // TEXT_CHUNK == 257 == L.fin_text3_off_words(N) - N - 1 and L.fin_text3_seg_pairs() == 4096   # per = 2 in scan2
    assert n_pairs > 4_194_304 + 1024
    nb = (n_pairs + TEXT_PAIRS - 1) // TEXT_PAIRS
    assert nb == L.fin_text_blocks(n_pairs) and nb > TEXT_CHUNK + 1 and L.fin_text_off_words(n_pairs) - nb - 1 == 2       # two chunks of pair blocks
    assert L.fin_depth_max_tile() == 4096 and L.fin_depth_max_chunk_tiles() == 4096
    # the kinds, block by block
    kind = c.recs["meta"] >> 16
    assert np.array_equal(kind, c.kind) and 0.68 < (kind == 1).mean() < 0.72 and not (kind == 2).any()
    blocks = lambda b: kind[REC_BLK * b:REC_BLK * (b + 1)]
    assert all((blocks(b) == 1).all() for b in ONLY_FINISHED) and all((blocks(b) == 0).all() for b in ONLY_SEARCHED)
    assert all(0 < (blocks(b) == 1).sum() < len(blocks(b)) for b in BOUNDARY + (0, 1, 1023)) and len(blocks(1026)) == N - 1026 * REC_BLK == 299
    # the finished reads: either strand with and without a position; places inside their unitig, some at its first k-mer, some with the last slot on its last
    one = kind == 1
    nE, rev, nks = c.recs["meta"] & 0xFF, (c.recs["meta"] >> 8) & 1, c.nks
    for e in (0, 1):
        for s in (0, 1):
            assert (one & (nE == e) & (rev == s)).sum() >= 100000
    room = c.kmers[c.recs["u"][one]] - nks[one] - c.recs["off0"][one].astype(np.int64)
    assert (room >= 0).all() and (room == 0).sum() >= 50 and (c.recs["off0"][one] == 0).sum() >= 50
    E = c.recs["Es"].astype(np.int64)
    assert (E[one & (nE == 1)] < (nks + K - 1)[one & (nE == 1)]).all() and not E[nE == 0].any() and not c.recs["Es2"].any()
    assert ((nE == 1) & (E < K - 1)).sum() >= 50 and ((nE == 1) & (E >= nks)).sum() >= 50          # a gap clamped at slot 0, at slot nk - 1
    zero = ~one
    for f in ("u", "off0", "meta", "Es", "Es2"):
        assert not c.recs[f][zero].any()
    (so, sg), summ = want("segments"), want("summaries")
    # a gap that covers the read; one that leaves a stretch (k = 16 and at most 9 slots: a gap always reaches one end of the read)
    assert (one & (summ["n_found"] == 0)).sum() >= 20 and (one & (summ["n_segments"] == 1) & (summ["n_found"] < nks)).sum() >= 20
    # the searched reads' pairs: both directions, absent slots, repeats
    s = c.stream.astype(np.int64)
    same = (s[1:, 0] == s[:-1, 0]) & (s[1:, 0] >= 0)
    d = s[1:, 1] - s[:-1, 1]
    assert (same & (d == 1)).sum() > 1000 and (same & (d == -1)).sum() > 1000 and (same & (d == 0)).sum() > 100 and (s[:, 0] == -1).sum() > 1000
    assert len(c.stream) == int(nks[zero].sum()) and (sg["len"] < -1).any() and (sg["len"] > 1).any() and (summ["n_segments"] >= 3).any()
    # every pair names a k-mer of its unitig
    f = c.pairs[:, 0] >= 0
    assert (c.pairs[f, 1] >= 0).all() and (c.pairs[f, 1] < c.kmers[c.pairs[f, 0]]).all()
    # the screens: everything, about half, nothing
    share = [rule_vec(summ, nks, mf, pm, 0).mean() for mf, pm in SCREENS]
    assert share[0] == 1.0 and 0.35 < share[1] < 0.65 and share[2] == 0.0, share
    # the rules of assignment: each assigns some reads and leaves some
    cls = want("classes")
    for r in RULES:
        t = tally_vec(cls, nks, N_LABELS, *r)
        assert 0 < t[-1] < N and int(t.sum()) == N and (t[:-1] > 0).sum() > 250, r
    assert (cls["n_second"] > 0).sum() > 1000 and ((cls["n_best"] == cls["n_second"]) & (cls["n_best"] > 0)).sum() > 100 and (cls["label"] == NONE).sum() > 1000
    # ---- the sample: every vectorised definition against its original ----
    idx = sample_reads_of(c, np.random.default_rng(5))
    assert len(idx) == 5000 and {0, N - 1, 1024 * 1024 - 1, 1024 * 1024, 1026 * 1024, 4105 * 256, 256 * 4096 - 1, 256 * 4096} <= set(idx.tolist())
    recs_s, stream_s, pairs_s, nks_s = take(c, idx)
    assert np.array_equal(brute_expand(recs_s, stream_s, K), pairs_s), "expand_vec is not brute_expand"
    assert np.array_equal(expand_vec(recs_s, stream_s, K), pairs_s)
    want_s = segments_of(pairs_s, nks_s)
    got_s, got_summ = segments_vec(pairs_s, nks_s)
    assert_segments(got_s, want_s, "segments_vec against segments_of")
    assert np.array_equal(np.diff(so.astype(np.int64))[idx], np.diff(want_s[0].astype(np.int64)))          # ... and the sample's rows of the whole set's
    first = so[:-1].astype(np.int64)[idx]
    rows = np.concatenate([np.arange(a, a + n) for a, n in zip(first, np.diff(want_s[0].astype(np.int64)))])
    assert np.array_equal(sg[rows], want_s[1])
    assert_summaries(got_summ, summaries_of(pairs_s, nks_s), "the summaries of segments_vec against summaries_of")
    assert np.array_equal(summ[idx], got_summ)
    for mf, pm in SCREENS:
        for inv in (0, 1):
            assert np.array_equal(rule_vec(got_summ, nks_s, mf, pm, inv), rule(got_summ, nks_s, mf, pm, inv))
    want_c = classes_of(pairs_s, nks_s, c.labels)
    assert_classes(classes_vec(pairs_s, nks_s, c.labels), want_c, "classes_vec against classes_of")
    assert np.array_equal(cls[idx], want_c)
    for r in RULES:
        assert np.array_equal(tally_vec(want_c, nks_s, N_LABELS, *r), tally_of(want_c, nks_s, N_LABELS, *r))
    # the text: the first and last 2 000 reads and 2 000 reads around pair 4 194 304
    text, at_byte = want("text")
    mid = int(np.searchsorted(c.at, 4_194_304, side="right")) - 1
    for lo in (0, N - 2000, mid - 1000):
        t = "".join(format_pairs(c.pairs[c.at[r]:c.at[r + 1]]) for r in range(lo, lo + 2000)).encode()
        assert bytes(text[at_byte[c.at[lo]]:at_byte[c.at[lo + 2000]]]) == t, "text_vec against format_pairs, reads %d .." % lo
    assert c.at[mid] <= 4_194_304 < c.at[mid + 1] and len(text) == at_byte[-1] and text[-1] == ord("\n")


# ---- 1. read-count thresholds, on the device -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    c = case()
    p = fa.FinimizerIndex.build(c.unitigs, K).to_device(0)
    assert np.array_equal(p.export(fa.X_ENDS), c.ends)
    made = {}

    def injected(mode):
        """the batch of N reads, run in text mode 1 or 2, its results overwritten with the hand-made records and pairs (mode 2: garbage where a finished
        read's pairs would be); mode 0: run in text mode 0, every pair overwritten"""
        if mode not in made:
            b = p.batch(c.reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
            assert b.n_reads == N and b.n_kmers == len(c.pairs)
            if mode == 0:
                b.set_pairs(c.pairs)
            else:
                slots = np.array(c.pairs)
                if mode == 2:
                    slots[np.repeat(c.kind == 1, c.nks)] = GARBAGE
                b.set_records(device_form(c.recs), slots)
            made[mode] = b
        return made[mode]
    yield SimpleNamespace(p=p, injected=injected)
    for b in made.values():
        b.close()
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_records_and_stream_past_one_block_a_thread(mode, dev):
    """fin_blk_scan_kernel over the records' blocks with per = 2: the records byte for byte with nk stamped, the stream = the searched reads' pairs in read order"""
    c, b = case(), dev.injected(mode)
    got_recs, got_stream = b.records()
    assert len(got_stream) == len(c.stream), "text mode %d: a stream of %d pairs, expected %d" % (mode, len(got_stream), len(c.stream))
    bad = np.nonzero((got_stream != c.stream).any(axis=1))[0]
    assert len(bad) == 0, "text mode %d: the stream differs in %d pairs, first %d (1024-read block boundaries of the stream: a shifted block)" % (mode, len(bad), bad[0])
    assert got_recs.tobytes() == c.recs.tobytes(), "text mode %d: records (first differing read %s)" % (mode, np.nonzero(got_recs != c.recs)[0][:1])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2, 0])
def test_segments_past_one_block_a_thread(mode, dev):
    """fin_blk_scan_kernel over the segments' blocks with per = 5 and a partial last thread; mode 0: every read scanned from hand-made pairs"""
    b = dev.injected(mode)
    (want_offs, want_segs) = want("segments")
    got_offs, got_segs = b.segments()
    assert np.array_equal(want_offs, np.concatenate([[0], np.cumsum(want("summaries")["n_segments"].astype(np.int64))]).astype(np.uint64))   # the exclusive prefix of the counts
    assert_segments((got_offs, got_segs), (want_offs, want_segs), "text mode %d" % mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2, 0])
def test_screen_ids_past_one_block_a_thread(mode, dev):
    """the screen's ids through fin_launch_blk_scan: none, about half and all of the reads pass, and the inverse of each"""
    c, b = case(), dev.injected(mode)
    summ = want("summaries")
    assert_summaries(b.read_summaries(), summ, "text mode %d" % mode)
    for mf, pm in SCREENS:
        for inv in (0, 1):
            r = rule_vec(summ, c.nks, mf, pm, inv)
            got = b.screen(mf, pm, inv)
            assert (np.diff(got[0].astype(np.int64)) > 0).all(), "text mode %d screen %s: ids do not ascend" % (mode, (mf, pm, inv))
            assert_screen(got, r, "text mode %d screen %s" % (mode, (mf, pm, inv)))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_classes_and_tally_at_this_size(mode, dev):
    """no second level of their own; 300 labels, the tally against np.bincount over the rule of assignment"""
    c, b = case(), dev.injected(mode)
    cls = want("classes")
    lab = dev.p.labels(c.labels, N_LABELS)
    try:
        assert_classes(b.classify(lab), cls, "text mode %d" % mode)
        for r in RULES:
            tally, total = lab.reset().add(b, *r).download()
            assert np.array_equal(tally, tally_vec(cls, c.nks, N_LABELS, *r)) and total == N, "text mode %d rule %s" % (mode, r)
    finally:
        lab.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2, 0])
def test_text_past_one_chunk(mode, dev):
    """modes 1 and 2: the segment form, 257 chunks of 4096 reads, per = 2 in fin_text_scan2_kernel, n_found added up over 257 chunks.  mode 0: the pair-block
    form, more than 4096 blocks of 1024 pairs, chunk_base[1] != 0"""
    b = dev.injected(mode)
    text, _ = want("text")
    assert_text(b.text(), text, "text mode %d" % mode)
    assert b.download(want_pairs=False)[1] == want("found"), "text mode %d: the count taken from the text pass" % mode
    if mode == 2:
        with pytest.raises(fa.FinitoError):   # still a text-only batch: its pairs stay refused
            b.download()
    else:
        assert np.array_equal(b.download()[0], case().pairs)


def genome_reads(rng, g, n, k):
    """n reads of k .. k + 8 bases cut from the genome, either strand; one in ten with one substituted base, one in twenty random: (bases, offsets)"""
    code = np.frombuffer(g.encode(), dtype=np.uint8)
    lens = rng.integers(k, k + 9, n).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    r = np.repeat(np.arange(n), lens)
    j = np.arange(int(offsets[-1])) - offsets[r]
    start = (rng.random(n) * (len(code) - lens + 1)).astype(np.int64)
    rev = rng.random(n) < 0.5
    comp = np.zeros(256, dtype=np.uint8); comp[list(b"ACGT")] = list(b"TGCA")
    bases = np.where(rev[r], comp[code[start[r] + np.where(rev[r], lens[r] - 1 - j, j)]], code[start[r] + j])
    t = rng.random(n)
    sub = offsets[:-1][t < 0.10] + (rng.random(int((t < 0.10).sum())) * lens[t < 0.10]).astype(np.int64)
    bases[sub] = comp[bases[sub]]
    rnd = np.nonzero((t >= 0.10) & (t < 0.15))[0]
    m = np.isin(r, rnd)
    bases[m] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(m.sum()))]
    return (np.ascontiguousarray(bases, dtype=np.uint8), offsets.astype(np.uint64)), lens - k + 1


@pytest.mark.gpu
def test_one_real_run_past_the_segment_threshold(dev):
    """300 000 genome reads in text mode 2 -- 1172 blocks of 256 reads, per = 2 in fin_blk_scan_kernel -- against the oracle: records + stream by brute_expand's
    rule, the segments, a screen, the text, and the classes and their tally through Labels.add_reads"""
    c = case()
    n = 300_000
    reads, nks = genome_reads(np.random.default_rng(20262), c.genome, n, K)
    exp = OracleIndex.build(c.unitigs, K).search_batch(reads, n_threads=8)[0]
    assert len(exp) == int(nks.sum()) > 1_400_000 and (n + SGM_BLK - 1) // SGM_BLK > 1024 and 0.5 < (exp[:, 0] != -1).mean() < 0.95
    b = dev.p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
    try:
        recs, stream = b.records()
        assert np.array_equal(recs["nk"], nks) and (recs["meta"] >> 16 == 1).sum() > 1000, "the real run's fast path finished reads"
        assert np.array_equal(expand_vec(recs, stream, K).astype(np.int64), exp), "records + stream"
        (want_offs, want_segs), summ = segments_vec(exp.astype(np.int32), nks)
        assert_segments(b.segments(), (want_offs, want_segs), "segments of the real run")
        r = rule_vec(summ, nks, 1, 1000, 0)
        assert 0.2 < r.mean() < 0.95
        assert_screen(b.screen(1, 1000, 0), r, "screen of the real run")
        assert_text(b.text(), text_vec(exp.astype(np.int32), nks)[0], "text of the real run")
        assert b.download(want_pairs=False)[1] == int((exp[:, 0] != -1).sum())
        cls = classes_vec(exp.astype(np.int32), nks, c.labels)
        assert (cls["n_second"] > 0).sum() > 100 and (cls["label"] == NONE).sum() > 1000
        lab = dev.p.labels(c.labels, N_LABELS)
        try:
            assert_classes(b.classify(lab), cls, "classes of the real run")
            for r in RULES:
                w = tally_vec(cls, nks, N_LABELS, *r)
                assert 0 < w[-1] < n
                tally, total = lab.reset().add_reads(reads, *r).download()
                assert np.array_equal(tally, w) and total == n, "add_reads of the real run, rule %s" % (r,)
        finally:
            lab.close()
    finally:
        b.close()


# ---- 2. depth past one scan thread per tile -----------------------------------------------------------------------------------------------------------------------
def truth_pairs(u, r, k):
    """the generator's ground truth (fin_synth.cpp: fin_synth_check's rule): a k-mer of a genome read without a substituted base is found in the piece that holds
    it, at its offset there, under the number the index gives that piece (synth.unitig_ids); every other k-mer counts as absent (see the file's docstring).
    (int64 pairs [n_kmers, 2], the unitigs' ends in the index's order)"""
    ids = synth.unitig_ids(None, u).astype(np.int64)
    lens = np.diff(u.offsets.astype(np.int64))
    in_order = np.zeros(len(u), dtype=np.int64); in_order[ids] = lens
    ends = np.cumsum(in_order)
    n, L = len(r), r.read_len
    nk = L - k + 1
    em = np.concatenate([np.zeros((n, 1), dtype=np.int64), np.cumsum(r.err_mask.reshape(n, L).astype(np.int64), axis=1)], axis=1)
    j = np.arange(nk, dtype=np.int64)[None, :]
    clean = (em[:, k:] - em[:, :nk] == 0) & (r.gstart >= 0)[:, None]
    gp = np.where(r.rc.astype(bool)[:, None], r.gstart[:, None] + (nk - 1 - j), r.gstart[:, None] + j)
    by_start = np.argsort(u.gstart, kind="stable")
    piece = by_start[np.searchsorted(u.gstart[by_start].astype(np.int64), np.where(clean, gp, 0), side="right") - 1]
    ps, pl = u.gstart.astype(np.int64)[piece], u.glen.astype(np.int64)[piece]
    assert (np.where(clean, gp + k, ps) <= ps + pl).all()             # the piece holds the whole k-mer
    off = np.where(u.rc.astype(bool)[piece], ps + pl - (gp + k), gp - ps)
    out = np.stack([np.where(clean, ids[piece], -1), np.where(clean, off, -1)], axis=2).reshape(-1, 2)
    return out, ends


@pytest.mark.gpu
@pytest.mark.parametrize("n_bases,G", [(4_500_000, 4_194_304), (17_000_000, 16_777_216)], ids=["4.5Mbp", "17Mbp"])
def test_depth_past_one_scan_thread_per_tile(n_bases, G):
    """k = 31, the production tile of 4096.  4.5 Mbp: more than 4 194 304 positions, 1116 tiles in one chunk, per = 2 in fin_depth_tile_scan_kernel, the last
    tile partial.  17 Mbp: more than 16 777 216 positions, a first chunk of 4096 tiles (per = 4) and a second, partial one behind its carry.
    20 000 reads added twice, against the generator's ground truth (the oracle needs half a minute to build the smaller index); then hand-made runs: one
    straddling text position G -- the boundary between two scan threads' tiles, or between the two chunks, where the carry is 1 only because of that run -- in
    either direction, one across the flat scan's span boundary at slot 4096, one ending at the last k-mer of the last unitig"""
    k = 31
    g = synth.genome(n_bases, seed=41)
    u = synth.unitigs(g, k)
    rd = synth.reads(g, 20_000, seed=42)
    truth, ends = truth_pairs(u, rd, k)
    total_len = int(ends[-1])
    n_tiles = (total_len + 4095) // 4096
    assert total_len > G + 4096 and total_len % 4096 and 0.6 < (truth[:, 0] >= 0).mean() < 0.8
    assert (1024 < n_tiles <= 4096) if G == 4_194_304 else (4096 < n_tiles < 8192 and G == 4096 * 4096)
    t0 = time.perf_counter()
    p = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    print("build + upload of %d bases: %.2f s" % (n_bases, time.perf_counter() - t0))
    try:
        assert np.array_equal(p.export(fa.X_ENDS), ends) and p.total_len == total_len
        wanted = Want(truth, ends)
        assert (wanted.depth[G:] > 0).sum() > 1000 and (wanted.depth[:G] > 0).sum() > 1000
        d = p.depth()
        for mode in (2, 0):
            b = p.batch(rd.as_tuple()); b.text_mode(mode); b.run(fa.FIN_MERGED)
            assert_depth(d.reset().add(b).download(min_depth=2), wanted, "text mode %d" % mode, min_depth=2)
            assert_depth(d.add(b).download(), wanted.times(2), "text mode %d, added twice" % mode)
            if mode == 0:   # hand-made runs over the same batch's pairs
                starts = np.concatenate([[0], ends[:-1]])
                kmers = np.diff(np.concatenate([[0], ends])) - k + 1
                ug = int(np.searchsorted(ends, G, side="right"))
                lo, hi = max(int(starts[ug]), G - 50), min(int(starts[ug] + kmers[ug]), G + 50)
                assert lo < G - 1 and G + 1 < hi, "the unitig around position %d leaves no room for a run across it" % G
                last = len(ends) - 1
                good = np.full((b.n_kmers, 2), -1, dtype=np.int64)
                run = np.arange(lo, hi) - starts[ug]
                m = min(60, len(run))
                good[1000:1000 + len(run)] = np.stack([np.full(len(run), ug), run], axis=1)                    # ascending across G
                good[2000:2000 + len(run)] = np.stack([np.full(len(run), ug), run[::-1]], axis=1)              # descending across G
                good[4096 - m // 2:4096 - m // 2 + m] = np.stack([np.full(m, ug), run[:m]], axis=1)            # across two waves' spans of the flat scan
                tail = np.arange(kmers[last] - 70, kmers[last])
                good[9000:9070] = np.stack([np.full(70, last), tail], axis=1)                                  # ends at the last k-mer of the last unitig
                hand = Want(good, ends)
                # (depth[G - 1] = the sum of the differences in front of G: what the thread, or the chunk, in front hands on is not zero)
                assert hand.depth[G] >= 2 and hand.depth[G - 1] >= 2 and hand.depth[total_len - k] == 1 and hand.found == 2 * len(run) + m + 70
                b.set_pairs(good)
                assert_depth(d.reset().add(b).download(), hand, "hand-made runs")
                assert_depth(d.add(b).add(b).download(min_depth=3), hand.times(3), "hand-made runs three times", min_depth=3)
            b.close()
        d.close()
    finally:
        p.close()


# ---- 3. the set merge past its grid --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_set_merge_past_its_grid():
    """fin_set_merge_kernel: 65 536 blocks of 256 threads take 16 777 216 pairs in one trip; 145 000 reads of 150 bases are 17 400 000.  A partitioned index of
    a 60 000-base genome (parts of at most 9 000 bases) must answer as the one index does, whose answer is the oracle's on 20 000 reads spread over the batch"""
    k = 31
    rng = np.random.default_rng(1031)
    g = random_genome(rng, 60000)
    unitigs = cut_unitigs(rng, g, k, max_len=900)
    rd = synth.reads(np.frombuffer(g.encode(), dtype=np.uint8).copy(), 145_000, seed=43)
    nk = 150 - k + 1
    n_pairs = len(rd) * nk
    assert n_pairs > 16_777_216 + 65_536
    one = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    p = fa.PartitionedIndex(unitigs, k, device=0, max_part_bases=9000, verify=True)
    try:
        assert p.n_parts >= 3
        want_pairs, want_pos = one.search_reads(rd.as_tuple())
        assert want_pairs.shape == (n_pairs, 2)
        idx = np.linspace(0, len(rd) - 1, 20_000).astype(np.int64)
        assert (idx * nk > 16_777_216).sum() > 500
        exp = OracleIndex.build(unitigs, k).search_batch(rd.take(idx).as_tuple(), n_threads=8)[0]
        assert np.array_equal(want_pairs.reshape(len(rd), nk, 2)[idx].reshape(-1, 2).astype(np.int64), exp), "the one-index search against the oracle"
        assert 0.5 < (exp[:, 0] != -1).mean() < 0.9 and (want_pairs[16_777_216:, 0] != -1).sum() > 100_000
        got, npos = p.search_reads(rd.as_tuple())
        bad = np.nonzero((got != want_pairs).any(axis=1))[0]
        assert len(bad) == 0, "parts and the whole index disagree in %d pairs, first %d" % (len(bad), bad[0])
        assert npos == want_pos == int((want_pairs[:, 0] != -1).sum())
        # the device-resident form, run twice (the first part's buffer is the set's result: a second run must not see renumbered pairs)
        b = p.batch(rd.as_tuple())
        b.run(); b.run()
        got2, npos2 = b.download()
        bad = np.nonzero((got2 != want_pairs).any(axis=1))[0]
        assert len(bad) == 0 and npos2 == npos, "the device-resident form disagrees in %d pairs, first %s" % (len(bad), bad[:1])
        b.close()
    finally:
        p.close(); one.close()
