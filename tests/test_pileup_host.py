"""fin_records_pileup, the host statement of the pileup's definition (include/finito_amd.h: fin_pileup), against an independent model.

The model (pileup_model) is written here from the definition alone and shares no code with the library: it reads a read's pairs -- the ones fin_search_batch
delivers, or the oracle's --, the read itself, the text as one code per base (FIN_X_CONCAT) and the unitigs' ends (FIN_X_ENDS).  Every comparison is exact
integer equality of whole arrays.  tests/test_pileup.py and tests/test_cli_pileup.py hold the device to the same model."""
import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.util import cut_unitigs, hand_made_case, random_genome, rc, sample_reads

KEPT, NOT_STRAIGHT, OFF_UNITIG, TOO_MANY = 0, 1, 2, 3
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def pileup_model(reads, pairs, k, concat, ends, max_mismatch):
    """(cover int64[total_len], alt int64[total_len, 4], counters int64[4], outcome per read) by rules 1 .. 5 of the definition"""
    ends = np.asarray(ends, dtype=np.int64)
    starts = np.concatenate([[0], ends[:-1]])
    total = int(ends[-1])
    cover = np.zeros(total, dtype=np.int64); alt = np.zeros((total, 4), dtype=np.int64); counters = np.zeros(4, dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    outcome, at = [], 0
    for read in reads:
        read = read.decode() if isinstance(read, bytes) else read
        L = len(read); nk = max(0, L - k + 1)
        p = pairs[at:at + nk]; at += nk
        slots = [(i, int(u), int(off)) for i, (u, off) in enumerate(p) if u >= 0]
        # 1. straight: at least two found slots, one unitig, one diagonal
        fwd = len(slots) >= 2 and len({(u, off - i) for i, u, off in slots}) == 1
        rev = len(slots) >= 2 and len({(u, off + i) for i, u, off in slots}) == 1
        if fwd == rev:
            assert not fwd   # (both cannot hold with two slots)
            counters[NOT_STRAIGHT] += 1; outcome.append(NOT_STRAIGHT); continue
        i0, u, off0 = slots[0]
        # 2. placed: read base j at offset where[j] of u, observed as obs[j]
        if fwd:
            where = [off0 - i0 + j for j in range(L)]
            obs = [_CODE.get(c.upper()) for c in read]
        else:
            where = [off0 + i0 + k - 1 - j for j in range(L)]
            obs = [None if c.upper() not in _CODE else 3 - _CODE[c.upper()] for c in read]
        ulen = int(ends[u] - starts[u])
        if min(where) < 0 or max(where) >= ulen:
            counters[OFF_UNITIG] += 1; outcome.append(OFF_UNITIG); continue
        g = [int(starts[u]) + w for w in where]
        # 3. mismatches
        mm = [(gj, o) for gj, o in zip(g, obs) if o is not None and o != int(concat[gj])]
        if len(mm) > max_mismatch:
            counters[TOO_MANY] += 1; outcome.append(TOO_MANY); continue
        # 4. what a kept read adds
        for gj in g:
            cover[gj] += 1
        for gj, o in mm:
            alt[gj, o] += 1
        counters[KEPT] += 1; outcome.append(KEPT)
    assert at == len(pairs) and int(counters.sum()) == len(reads)
    assert (alt[np.arange(total), np.asarray(concat[:total], dtype=np.int64)] == 0).all()
    return cover, alt, counters, outcome


def call_model(cover, alt, ends, concat, min_alt, min_permille):
    """the candidates of fin_pileup_call as a VARIANT_DTYPE array, ascending"""
    ends = np.asarray(ends, dtype=np.int64)
    m = alt.max(axis=1)
    g = np.nonzero((m >= max(min_alt, 1)) & (1000 * m >= min_permille * cover))[0]
    u = np.searchsorted(ends, g, side="right")
    out = np.zeros(len(g), dtype=fa.VARIANT_DTYPE)
    out["u"], out["off"], out["cover"], out["ref"], out["alt"] = u, g - np.concatenate([[0], ends[:-1]])[u], cover[g], np.asarray(concat)[g], alt[g]
    return out


def assert_pileup(got, want, what=""):
    cover, alt, counters = got
    wc, wa, wn = want[:3]
    assert cover.dtype == np.uint32 and alt.dtype == np.uint32 and cover.shape == wc.shape and alt.shape == wa.shape, what
    assert [int(x) for x in counters] == [int(x) for x in wn], "%s: counters %s, model %s" % (what, list(counters), list(wn))
    bad = np.nonzero(cover.astype(np.int64) != wc)[0]
    assert len(bad) == 0, "%s: cover differs at %d positions, first %d: got %d, model %d" % (what, len(bad), bad[0], cover[bad[0]], wc[bad[0]])
    bad = np.nonzero((alt.astype(np.int64) != wa).any(axis=1))[0]
    assert len(bad) == 0, "%s: alt differs at %d positions, first %d: got %s, model %s" % (what, len(bad), bad[0], alt[bad[0]], wa[bad[0]])


def spell_reads(case, rng, concat):
    """hand_made_case's reads have free content; where a kind-1 record places one, spell it from the text with a few substitutions, so that kept reads and alt
    counts occur.  Returns new reads of the same lengths"""
    starts = np.concatenate([[0], case.ends[:-1]])
    out = []
    for r, read in enumerate(case.reads):
        R = case.recs[r]
        if (int(R["meta"]) >> 16) == 1 and rng.random() < 0.8:
            g0 = int(starts[int(R["u"])]) + int(R["off0"])
            s = ["ACGT"[c] for c in concat[g0:g0 + len(read)]]
            for _ in range(int(rng.integers(0, 4))):
                j = int(rng.integers(0, len(s))); s[j] = rng.choice([c for c in "ACGTN" if c != s[j]])
            read = "".join(s)
            if (int(R["meta"]) >> 8) & 1:
                read = rc(read)
            if rng.random() < 0.1:
                read = read.lower()
        out.append(read)
    return out


@pytest.fixture(scope="module", params=[31, 63])
def hand(request):
    case = hand_made_case(request.param)
    o = OracleIndex.build(case.unitigs, case.k)
    concat = o.concat()
    reads = spell_reads(case, np.random.default_rng(77 + case.k), concat)
    return case, concat, reads


def test_hand_made_records_against_the_model(hand):
    """records and streams built by hand (tests/util.py): kind-1 records on both strands with 0 .. 8 positions of every shape, kind-0 reads whose pairs are
    ascending and descending runs, absent stretches and repeated pairs, kind-2 reads.  The model reads the pairs the records mean"""
    case, concat, reads = hand
    for mm in (0, 2, 8, 255):
        want = pileup_model(reads, case.pairs, case.k, concat, case.ends, mm)
        if mm == 2:
            assert all(want[2] > 0) and want[1].sum() > 0, "the inputs show every outcome and some mismatches: %s" % (want[2],)
        got = fa.records_pileup(case.recs, case.stream, case.k, reads, case.ends, concat, max_mismatch=mm, n_threads=4)
        assert_pileup(got, want, "k=%d max_mismatch=%d" % (case.k, mm))


def test_thread_counts_agree(hand):
    case, concat, reads = hand
    a = fa.records_pileup(case.recs, case.stream, case.k, reads, case.ends, concat, n_threads=1)
    b = fa.records_pileup(case.recs, case.stream, case.k, reads, case.ends, concat, n_threads=16)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("k", [31, 65])
def test_oracle_pairs_as_an_all_kind0_record_set(k):
    """sampled reads with substitutions on both strands, reads from nowhere, mosaics of two places: the oracle's pairs, every record kind 0"""
    rng = np.random.default_rng(900 + k)
    g = random_genome(rng, 6000)
    unitigs = cut_unitigs(rng, g, k, max_len=400)
    o = OracleIndex.build(unitigs, k)
    reads = sample_reads(rng, g, 150, 120, err=0.02) + [g[100:160] + g[3000:3060], g[500:500 + k], g[700:700 + k + 1], "ACGT", "", g[900:1000].lower(),
                                                        g[1200:1250] + "N" + g[1251:1300]]
    pairs = o.search_batch(reads, n_threads=4)[0]
    recs = np.zeros(len(reads), dtype=fa.RECORD_DTYPE)
    recs["nk"] = [max(0, len(r) - k + 1) for r in reads]
    for mm in (0, 3, 8):
        want = pileup_model(reads, pairs, k, o.concat(), o.ends(), mm)
        got = fa.records_pileup(recs, pairs.astype(np.int32), k, reads, o.ends(), o.concat(), max_mismatch=mm, n_threads=2)
        assert_pileup(got, want, "k=%d max_mismatch=%d" % (k, mm))
    assert want[2][KEPT] > 50 and want[2][NOT_STRAIGHT] > 0 and want[1].sum() > 50


def test_refusals(hand):
    case, concat, reads = hand
    k, ends = case.k, case.ends
    ok = lambda **kw: fa.records_pileup(kw.get("recs", case.recs), kw.get("stream", case.stream), k, kw.get("reads", reads), kw.get("ends", ends), concat,
                                        max_mismatch=kw.get("mm", 8), n_threads=2)
    ok()
    kind1 = np.nonzero((case.recs["meta"] >> 16) == 1)[0]
    kind0 = np.nonzero(((case.recs["meta"] >> 16) == 0) & (case.recs["nk"] > 0))[0]
    with pytest.raises(fa.FinitoError):    # a unitig number outside the index
        recs = case.recs.copy(); recs["u"][kind1[0]] = len(ends); ok(recs=recs)
    with pytest.raises(fa.FinitoError):    # a k-mer that does not lie inside its unitig
        recs = case.recs.copy(); recs["off0"][kind1[0]] = 10 ** 6; ok(recs=recs)
    with pytest.raises(fa.FinitoError):    # a stream that is not this record set's
        ok(stream=case.stream[:-1])
    with pytest.raises(fa.FinitoError):    # a pair that is neither found nor (-1,-1)
        stream = case.stream.copy(); stream[0] = (-2, 5); ok(stream=stream)
    with pytest.raises(fa.FinitoError):    # a read whose length is not its record's
        rd = list(reads); rd[int(kind0[0])] = rd[int(kind0[0])] + "A"; ok(reads=rd)
    with pytest.raises(fa.FinitoError):    # descending ends
        ok(ends=ends[::-1].copy())
    with pytest.raises(fa.FinitoError):
        ok(mm=256)
    with pytest.raises(fa.FinitoError):    # another number of reads than records
        ok(reads=reads[:-1])
