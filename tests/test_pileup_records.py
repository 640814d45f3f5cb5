"""The device pileup (fin_pileup.hip) on HAND-MADE records, in the shared wave frame at its edges, on places outside the index, behind a withheld step, and its
call past the first level of its scan.

fin_pileup_add_kernel's kind-1 branch trusts the record and never reads the text -- "the positions ARE the read's mismatches" --, while the host twin expands the
record and compares the whole read with the text.  The only records that branch had seen were the fast path's own: at most four positions, reads of at most 256
bases, places inside the index.  Here it is given the whole format (tests/util.py::hand_made_case): five to eight positions on either strand, records whose gaps
leave no found slot or one, nE on both sides of every mismatch limit.

The reference throughout is tests/test_pileup_host.py::pileup_model and ::call_model, read over tests/test_records.py::brute_expand of the hand-made records.
Nothing is expected from fin_records_pileup, fin_expand_records or a device output (the guard test holds fin_records_pileup to the model as a cross-check of the
generator, no more), and every comparison is exact integer equality of whole arrays through assert_pileup and assert_variants.

Because the device trusts a kind-1 record and the model reads the text, the reads are SPELLED to agree with their records (`spell`): strand A is the text at
[start(u) + off0, + L) with the base at each position replaced by another of A, C, G, T; the read is strand A, or its reverse complement when the record says
so; one read in ten is in lower case.  Positions are made distinct first (`distinct_records`, on a copy: the shared case is read-only): of the records whose
positions coincide, half are collapsed (nE shrinks) and half re-drawn -- a coinciding position moves to the nearest free one, nE stays --, so that every cell
(nE 0 .. 8, strand) stays populated.  A kind-0 read whose hand-made pairs the model finds straight and inside the unitig is spelled from the text with 0 to 3
substitutions and the odd N, four times in five; the others stay free.

Two cases cannot be reached, and one thing is read where it lies:
  * the off-unitig outcome of a kind-1 record in a clean accumulator: fin_pileup_add_kernel sets flag bit 1 ("outside the index") for every record that is not
    inside its unitig, so that outcome of a record is part of test_places_outside_the_index; the guard asserts the other three outcomes among kind-1 reads and
    all four among kind-0 reads.
  * a record with a position equal to L: fin_batch_set_records refuses E >= nk + k - 1, so it never reaches the device; the test asserts the refusal and that
    nothing of the record reached the batch.  The kernel's own guard for it (E >= L) stays out of reach of the C ABI.
  * the state of a flagged accumulator: fin_pileup_download refuses, so cover, alt and the counters are read from device memory (`flagged_state`; the counters
    are the four u64 behind alt, fin_capi.cpp: pileup_counters).

Times on an MI355X, as measured (pytest --durations, the module run as a whole; the model is made once per case and limit and shared, so whoever asks first
pays for it -- the guard test when the module runs whole, otherwise the first GPU test of each k, about 2.3 s there): the guard test 2.1 to 2.6 s per k (10 s on
a slow CPU), the frame's guard 0.09 s; test_the_call_past_one_block_a_scan_thread 0.52 s (build on the device, upload, 2 040 reads, the model over 306 000 bases);
test_places_outside_the_index 0.37 s; test_the_device_on_hand_made_records 0.29 s for the first case, 0.02 to 0.04 s for the others;
test_a_withheld_step_adds_nothing_and_is_reported_until_the_reset 0.13 s up to its good step (alone in a process, imports included, 3.4 s);
test_the_frame_in_the_pileup 0.07 / 0.02 / 0.02 s.  tests/test_assign.py's bin cases: 0.04 s past 262 144 reads, below 0.005 s each otherwise."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import finito_amd as fa
from finito_amd import synth
from oracle.oracle import OracleIndex
from tests.test_pileup import assert_variants
from tests.test_pileup_host import KEPT, NOT_STRAIGHT, OFF_UNITIG, TOO_MANY, assert_pileup, call_model, pileup_model
from tests.test_records import brute_expand
from tests.test_records_device import inject, on_device   # noqa: F401  (on_device: the module-scoped fixture, one set of indexes for this module)
from tests.test_records_host import positions_of
from tests.test_row_frame import assert_frame_conditions, frame_case
from tests.test_unitig_depth import device_int32
from tests.util import cut_unitigs, hand_made_case, random_genome, rc, sample_reads

MISMATCH_LIMITS = (0, 4, 5, 7, 8, 255)   # they separate records of 4, 5 and 8 positions from their neighbours
CALLS = ((2, 200), (1, 0))
KS = (16, 31, 63)
_OTHER = {c: [x for x in "ACGT" if x != c] for c in "ACGT"}


# ---- the generator ----------------------------------------------------------------------------------------------------------------------------------------
def set_positions(recs, r, Es):
    recs["meta"][r] = (int(recs["meta"][r]) & ~0xFF) | len(Es)
    recs["Es"][r] = sum(E << (16 * e) for e, E in enumerate(Es[:4])); recs["Es2"][r] = sum(E << (16 * e) for e, E in enumerate(Es[4:]))


def distinct_records(recs, k, rng):
    """a copy of the records in which every kind-1 record's positions are distinct: coinciding ones collapsed, or -- every other time -- moved to the nearest
    free position, so that nE stays"""
    out = np.array(recs)
    for r in np.nonzero(out["meta"] >> 16 == 1)[0]:
        Es = positions_of(out[r])
        if len(set(Es)) == len(Es):
            continue
        top = int(out["nk"][r]) + k - 2
        if rng.random() < 0.5 and top + 1 >= len(Es):
            used = []
            for E in Es:
                d = 0
                while not [x for x in (E + d, E - d) if 0 <= x <= top and x not in used]:
                    d += 1
                used.append([x for x in (E + d, E - d) if 0 <= x <= top and x not in used][0])
            Es = sorted(used)
        else:
            Es = sorted(set(Es))
        set_positions(out, r, Es)
    return out


def placement(p, k, starts, ends):
    """rules 1 and 2 of the definition on one read's pairs: (u, s0, reverse) where the read is straight and inside its unitig, else None"""
    p = np.asarray(p, dtype=np.int64).reshape(-1, 2)
    nk = len(p); L = nk + k - 1
    i = np.nonzero(p[:, 0] >= 0)[0]
    if len(i) < 2 or (p[i, 0] != p[i[0], 0]).any():
        return None
    u, off = int(p[i[0], 0]), p[i, 1]
    fwd, rev = bool((off - i == off[0] - i[0]).all()), bool((off + i == off[0] + i[0]).all())
    if fwd == rev:
        return None
    s0 = int(off[0] - i[0]) if fwd else int(off[0] + i[0]) - nk + 1
    if s0 < 0 or s0 + L > int(ends[u] - starts[u]):
        return None
    return u, s0, rev


def spell(k, ends, concat, recs, pairs, free_reads, rng, always=()):
    """the reads spelled to agree with their records (see the module's docstring); `always`: kind-0 reads that are spelled whenever they have a place"""
    starts = np.concatenate([[0], ends[:-1]]).astype(np.int64)
    text = "".join("ACGT"[c] for c in concat)
    at = np.concatenate([[0], np.cumsum(recs["nk"].astype(np.int64))])
    out = []
    for r, R in enumerate(recs):
        kind, L, read = int(R["meta"]) >> 16, int(R["nk"]) + k - 1, free_reads[r]
        assert len(read) == L
        place = None
        if kind == 1:
            place = (int(R["u"]), int(R["off0"]), bool((int(R["meta"]) >> 8) & 1))
            at_E = positions_of(R)
            assert len(set(at_E)) == len(at_E) and all(E < L for E in at_E)
        elif kind == 0:
            place = placement(pairs[at[r]:at[r + 1]], k, starts, ends)
            if place is not None and not (r in always or rng.random() < 0.8):
                place = None
            at_E = [] if place is None else [int(x) for x in rng.integers(0, L, int(rng.integers(0, 4)))]
        if place is not None:
            u, s0, rev = place
            g0 = int(starts[u]) + s0
            s = list(text[g0:g0 + L])
            assert len(s) == L and g0 + L <= int(ends[u])
            for E in at_E:
                s[E] = str(rng.choice(_OTHER[text[g0 + E]]))
            if kind == 0 and rng.random() < 0.15:
                s[int(rng.integers(0, L))] = "N"
            read = "".join(s)
            if rev:
                read = rc(read)
            if rng.random() < 0.1:
                read = read.lower()
        out.append(read)
    return out


def found_slots(ns):
    """per read: how many of its slots are found"""
    at = np.concatenate([[0], np.cumsum(ns.nks)])
    f = np.concatenate([[0], np.cumsum(ns.pairs[:, 0] >= 0)])
    return f[at[1:]] - f[at[:-1]]


def want(ns, mm):
    """the model at one mismatch limit, made once per case and left unchanged"""
    if mm not in ns.want:
        ns.want[mm] = pileup_model(ns.reads, ns.pairs, ns.k, ns.concat, ns.ends, mm)
        for a in ns.want[mm][:3]:
            a.setflags(write=False)
    return ns.want[mm]


_SPELLED = {}


def spelled_case(k):
    """hand_made_case(k) with distinct positions and spelled reads; made once per k and shared"""
    if k not in _SPELLED:
        c = hand_made_case(k)
        rng = np.random.default_rng(5100 + k)
        concat = OracleIndex.build(c.unitigs, k).concat()
        recs = distinct_records(c.recs, k, rng)
        pairs = brute_expand(recs, c.stream, k)
        reads = spell(k, c.ends, concat, recs, pairs, c.reads, rng)
        for a in (recs, pairs):
            a.setflags(write=False)
        _SPELLED[k] = SimpleNamespace(k=k, unitigs=c.unitigs, ends=c.ends, concat=concat, recs=recs, stream=c.stream, pairs=pairs, reads=reads,
                                      nks=np.asarray(c.nks, dtype=np.int64), want={})
    return _SPELLED[k]


FRAME_EXTRA_NK = (48, 49, 50, 113, 114)   # L = nk + 15 = 63, 64, 65, 128, 129: a row of 64 BASES ends where no row of 64 slots does
_FRAME = None


def frame_pileup_case():
    """tests/test_row_frame.py::frame_case, its kind-1 positions made distinct, with ten searched reads behind it -- one ascending and one descending run per nk of
    FRAME_EXTRA_NK -- and every read spelled.  `all_searched`: the same batch where the step left no records"""
    global _FRAME
    if _FRAME is None:
        c = frame_case()
        k = c.k
        rng = np.random.default_rng(2900)
        concat = OracleIndex.build(c.unitigs, k).concat()
        kmers = np.diff(np.concatenate([[0], c.ends])) - k + 1
        big = np.nonzero(kmers >= 200)[0]
        extra, extra_nk = [], []
        for j, nk in enumerate(FRAME_EXTRA_NK):
            u, v = int(big[(5 * j + 1) % len(big)]), int(big[(5 * j + 2) % len(big)])
            extra += [(u, 4 + i) for i in range(nk)] + [(v, nk + 6 - i) for i in range(nk)]
            extra_nk += [nk, nk]
        n0 = len(c.recs)
        recs = np.zeros(n0 + len(extra_nk), dtype=fa.RECORD_DTYPE)
        recs[:n0] = distinct_records(c.recs, k, rng)
        recs["nk"][n0:] = extra_nk
        stream = np.concatenate([c.stream, np.array(extra, dtype=np.int32)])
        pairs = brute_expand(recs, stream, k)
        free = list(c.reads) + [random_genome(rng, nk + k - 1) for nk in extra_nk]
        kinds = recs["meta"] >> 16
        reads = spell(k, c.ends, concat, recs, pairs, free, rng, always=set(np.nonzero(kinds == 0)[0].tolist()))
        all_searched = np.zeros(len(recs), dtype=fa.RECORD_DTYPE)
        all_searched["nk"] = recs["nk"]
        for a in (recs, stream, pairs, all_searched):
            a.setflags(write=False)
        _FRAME = SimpleNamespace(k=k, unitigs=c.unitigs, ends=c.ends, concat=concat, recs=recs, stream=stream, pairs=pairs, reads=reads,
                                 nks=recs["nk"].astype(np.int64), all_searched=all_searched, want={})
    return _FRAME


# ---- 1. conditions on the inputs, and the generator against the host twin (no GPU) ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_the_inputs_show_what_they_are_meant_to(k):
    ns = spelled_case(k)
    kind, nE, rev = ns.recs["meta"] >> 16, ns.recs["meta"] & 0xFF, (ns.recs["meta"] >> 8) & 1
    L = ns.nks + k - 1
    found = found_slots(ns)
    one = kind == 1
    assert np.array_equal(kind, hand_made_case(k).recs["meta"] >> 16) and np.array_equal(brute_expand(ns.recs, ns.stream, k), ns.pairs)
    for cell in range(18):   # every (nE, strand) is still there
        assert (one & (nE == cell % 9) & (rev == cell // 9)).sum() >= 20, "k=%d: cell nE %d strand %d was emptied" % (k, cell % 9, cell // 9)
    out4, out8 = np.array(want(ns, 4)[3]), np.array(want(ns, 8)[3])
    assert set(out4[one].tolist()) == {KEPT, NOT_STRAIGHT, TOO_MANY}, "kind-1 reads (a record off its unitig flags the accumulator: test_places_outside_the_index)"
    assert set(out4[kind == 0].tolist()) == {KEPT, NOT_STRAIGHT, OFF_UNITIG, TOO_MANY}, "kind-0 reads"
    assert set(out4[kind == 2].tolist()) == {NOT_STRAIGHT}
    for n in (5, 6, 7, 8):
        for strand in (0, 1):
            assert (one & (nE == n) & (rev == strand) & (out8 == KEPT)).any(), "k=%d: no kept record with %d positions on strand %d" % (k, n, strand)
    first = np.array([bool(kk == 1 and n and positions_of(R)[0] == 0) for R, kk, n in zip(ns.recs, kind, nE)])
    last = np.array([bool(kk == 1 and n and positions_of(R)[-1] == l - 1) for R, kk, n, l in zip(ns.recs, kind, nE, L)])
    assert (first & (out8 == KEPT)).any() and (last & (out8 == KEPT)).any(), "a kept record with a position at 0, one with a position at L - 1"
    assert (one & (found == 0)).any() and (one & (found == 1)).any(), "a record with no found slot, one with exactly one"
    assert (out8[one & (found < 2)] == NOT_STRAIGHT).all()
    assert want(ns, 8)[1].max() >= 2
    for mm in MISMATCH_LIMITS:   # what the device will do with a record, said in the model's words: the spelling is right
        w = want(ns, mm)
        o = np.array(w[3])
        assert np.array_equal(o[one], np.where(found[one] < 2, NOT_STRAIGHT, np.where(nE[one] > mm, TOO_MANY, KEPT))), "k=%d max_mismatch=%d" % (k, mm)
        got = fa.records_pileup(ns.recs, ns.stream, k, ns.reads, ns.ends, ns.concat, max_mismatch=mm, n_threads=4)
        assert_pileup(got, w, "the host twin, k=%d max_mismatch=%d" % (k, mm))
    at8 = want(ns, 255)[1].sum() - want(ns, 8)[1].sum()
    assert at8 > 0, "free reads on a place: more than eight mismatches"


def frame_conditions(ns):
    """beside assert_frame_conditions, which speaks of frame_case(): this case is that one read for read -- the same kinds and lengths, and the searched reads' pairs
    unchanged, so its conditions hold here -- and has kept searched reads of 63, 64, 65, 128 and 129 bases on both diagonals"""
    c = frame_case()
    n0 = len(c.recs)
    assert np.array_equal(ns.recs["meta"][:n0] >> 16, c.kinds) and np.array_equal(ns.recs["nk"][:n0], c.nks) and (ns.recs["meta"][n0:] >> 16 == 0).all()
    assert np.array_equal(ns.stream[:len(c.stream)], c.stream) and [len(r) for r in ns.reads[:n0]] == [len(r) for r in c.reads]
    searched = np.repeat(c.kinds == 0, c.nks)
    assert np.array_equal(ns.pairs[:len(c.pairs)][searched], c.pairs[searched])
    starts = np.concatenate([[0], ns.ends[:-1]])
    at = np.concatenate([[0], np.cumsum(ns.nks)])
    out = want(ns, 8)[3]
    seen = set()
    for r in np.nonzero(ns.recs["meta"] >> 16 == 0)[0]:
        pl = placement(ns.pairs[at[r]:at[r + 1]], ns.k, starts, ns.ends)
        if pl is not None and out[r] == KEPT:
            seen.add((len(ns.reads[r]), pl[2]))
    assert seen >= {(L, d) for L in (63, 64, 65, 128, 129) for d in (False, True)}, sorted(seen)
    assert len(ns.recs) % 64 not in (0, 63) and (np.array(out)[ns.recs["meta"] >> 16 == 1] == KEPT).any()


def test_the_frame_input_holds_the_edges():
    assert_frame_conditions(frame_case())
    ns = frame_pileup_case()
    frame_conditions(ns)
    for mm in (0, 8):
        assert_pileup(fa.records_pileup(ns.recs, ns.stream, ns.k, ns.reads, ns.ends, ns.concat, max_mismatch=mm, n_threads=2), want(ns, mm), "the host twin")
        assert_pileup(fa.records_pileup(ns.all_searched, ns.pairs, ns.k, ns.reads, ns.ends, ns.concat, max_mismatch=mm, n_threads=2), want(ns, mm), "all searched")


# ---- 2. the device on those records ------------------------------------------------------------------------------------------------------------------------------
def check_accumulators(p, b, ns, what, twice=True):
    """one accumulator per mismatch limit over the batch: download, counters, the two calls, the batch added a second time.  (p: tests/test_records_device.py's
    on_device fixture, one index per k for this module; the text the reads were spelled from must be the device's)"""
    assert np.array_equal(p.export(fa.X_ENDS), ns.ends) and np.array_equal(p.export(fa.X_CONCAT), ns.concat)
    accs = [p.pileup(max_mismatch=mm) for mm in MISMATCH_LIMITS]
    try:
        for a in accs:
            a.add(b)
        for mm, a in zip(MISMATCH_LIMITS, accs):
            w, at = want(ns, mm), "%s max_mismatch=%d" % (what, mm)
            got = a.download()
            assert_pileup(got, w, at)
            assert int(got[2].sum()) == len(ns.reads)
            for min_alt, pm in CALLS:
                assert_variants(a.call(min_alt, pm), call_model(w[0], w[1], ns.ends, ns.concat, min_alt, pm), "%s call(%d, %d)" % (at, min_alt, pm))
        if twice:
            for a in accs:
                a.add(b)
            for mm, a in zip(MISMATCH_LIMITS, accs):
                w = want(ns, mm)
                assert_pileup(a.download(), (2 * w[0], 2 * w[1], 2 * w[2]), "%s max_mismatch=%d, added twice" % (what, mm))
    finally:
        for a in accs:
            a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("k", KS)
def test_the_device_on_hand_made_records(k, mode, on_device):
    """in text mode 2 the finished reads' pair slots hold GARBAGE: the pileup must not read them"""
    ns, p = spelled_case(k), on_device(k)
    b = p.batch(ns.reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(ns.pairs)
    inject(b, ns.recs, ns.pairs, mode)
    check_accumulators(p, b, ns, "k=%d text mode %d" % (k, mode))
    b.close()


# ---- 3. the frame ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_the_frame_in_the_pileup(mode, on_device):
    """tests/test_row_frame.py's case in its three forms: lanes at and beyond n_reads, a wave without a searched read, one whose only searched reads are lanes 0
    and 63, the kinds interleaved; and the pileup's own edge, rows of 64 bases in passes 2 and 3"""
    ns, p = frame_pileup_case(), on_device(16)
    assert_frame_conditions(frame_case()); frame_conditions(ns)
    b = p.batch(ns.reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(ns.pairs)
    if mode == 0:
        b.set_pairs(ns.pairs)   # no records: every read is scanned
    else:
        inject(b, ns.recs, ns.pairs, mode)
    check_accumulators(p, b, ns, "the frame, text mode %d" % mode)
    b.close()


# ---- 4. places outside the index, and a withheld step ------------------------------------------------------------------------------------------------------------
def flagged_state(a, total_len):
    """(cover, alt, counters) of an accumulator whose download refuses, read where they lie: the counters are the four u64 behind alt (fin_capi.cpp)"""
    alt_ptr, diff_ptr = a.device_ptrs()
    words = device_int32(alt_ptr, 4 * total_len + 8)
    diff = device_int32(diff_ptr, total_len + 1).astype(np.int64)
    assert int(diff.sum()) == 0, "half a range was written"
    return np.cumsum(diff[:-1]), words[:4 * total_len].view(np.uint32).reshape(-1, 4).astype(np.int64), words[4 * total_len:].view(np.uint64).astype(np.int64)


@pytest.mark.gpu
def test_places_outside_the_index(on_device):
    """tests/test_unitig_depth.py::test_hand_made_pairs_and_places_outside_the_index for the pileup, one offending read at a time among the first 640 reads of the
    hand-made case: a record on unitig n_unitigs; a record whose off0 + L is one past its unitig's end; a searched read with one found slot on unitig n_unitigs.
    Nothing of the read is added, the others are counted as the model counts them without it, the record counts as off its unitig and the slot as not straight,
    download and call say "outside the index" until the reset.  (A record with a position equal to L: fin_batch_set_records refuses it -- asserted here.)"""
    k, n = 31, 640
    full, p = spelled_case(k), on_device(k)
    assert np.array_equal(p.export(fa.X_CONCAT), full.concat)
    at = np.concatenate([[0], np.cumsum(full.nks)])
    ns = SimpleNamespace(k=k, ends=full.ends, concat=full.concat, recs=full.recs[:n], pairs=full.pairs[:at[n]], reads=full.reads[:n], nks=full.nks[:n], want={})
    good = want(ns, 8)
    out = np.array(good[3])
    kind, nE = ns.recs["meta"] >> 16, ns.recs["meta"] & 0xFF
    starts = np.concatenate([[0], ns.ends[:-1]])
    total_len, n_unitigs = p.total_len, p.n_unitigs
    r1, r2, r3 = (int(r) for r in np.nonzero((kind == 1) & (out == KEPT) & (nE >= 1))[0][:3])
    r0 = int(np.nonzero((kind == 0) & (out == KEPT))[0][0])

    def without(r):
        w = pileup_model(ns.reads[:r] + ns.reads[r + 1:], np.delete(ns.pairs, np.arange(at[r], at[r + 1]), axis=0), k, ns.concat, ns.ends, 8)
        assert w[1].sum() < good[1].sum() or w[0].sum() < good[0].sum()
        return w

    b = p.batch(ns.reads); b.text_mode(2); b.run(fa.FIN_MERGED)
    a = p.pileup()
    inject(b, ns.recs, ns.pairs, 2)
    assert_pileup(a.add(b).download(), good, "the good set")

    def offend(recs, pairs, r, counter, what):
        inject(b, recs, pairs, 2)
        a.reset().add(b)
        for call in (a.download, a.download, lambda: a.call(2, 200), lambda: a.call(1, 0)):   # ... until the reset
            with pytest.raises(fa.FinitoError) as e:
                call()
            assert e.value.code == fa.FIN_EINVAL and "outside the index" in str(e.value), what
        w = without(r)
        cover, alt, counters = flagged_state(a, total_len)
        counters_want = w[2].copy(); counters_want[counter] += 1
        assert counters.tolist() == counters_want.tolist(), "%s: counters %s, the model without the read and the read under %d: %s" % (what, counters, counter, counters_want)
        assert np.array_equal(cover, w[0]) and np.array_equal(alt, w[1]), "%s: something of the offending read was added, or another read was not" % what
        inject(b, ns.recs, ns.pairs, 2)
        assert_pileup(a.reset().add(b).download(), good, "%s: after the reset" % what)
        assert_variants(a.call(2, 200), call_model(good[0], good[1], ns.ends, ns.concat, 2, 200), "%s: the call after the reset" % what)

    recs = np.array(ns.recs); recs["u"][r1] = n_unitigs
    offend(recs, ns.pairs, r1, OFF_UNITIG, "a record on unitig n_unitigs")
    recs = np.array(ns.recs)
    u = int(recs["u"][r2]); L = int(recs["nk"][r2]) + k - 1
    recs["off0"][r2] = int(ns.ends[u] - starts[u]) - L + 1
    offend(recs, ns.pairs, r2, OFF_UNITIG, "a record that ends one base past its unitig")
    pairs = np.array(ns.pairs)
    slots = at[r0] + np.nonzero(ns.pairs[at[r0]:at[r0 + 1], 0] >= 0)[0]
    pairs[slots[len(slots) // 2]] = (n_unitigs, 0)
    offend(ns.recs, pairs, r0, NOT_STRAIGHT, "a searched read with one found slot on unitig n_unitigs")
    # a position equal to L never reaches the device
    recs = np.array(ns.recs)
    L = int(recs["nk"][r3]) + k - 1
    set_positions(recs, r3, positions_of(recs[r3])[:-1] + [L])
    with pytest.raises(fa.FinitoError) as e:
        inject(b, recs, ns.pairs, 2)
    assert e.value.code == fa.FIN_EINVAL and "record %d" % r3 in str(e.value) and "position" in str(e.value)
    assert_pileup(a.reset().add(b).download(), good, "a refused record copied something")
    a.close(); b.close()


@pytest.mark.gpu
def test_a_withheld_step_adds_nothing_and_is_reported_until_the_reset():
    """tests/test_unitig_depth.py::test_a_withheld_step_adds_nothing_and_is_reported_until_the_reset's recipe: a step whose overflow list overran has no results;
    the add reads the counter itself, adds nothing and flags the accumulator; download and call report FIN_ELIMIT until the reset, a good step after it equals
    the model; add_reads over sub-batches with a withheld one among them ends the same way.

    What the reset clears is looked at BEFORE the reset (`flagged_state`: download refuses): cover, alt and the counters are all zero after the withheld add --
    had the kernel gone on behind fin_step_withheld, every read of the step would stand in the counters.  add_reads gets a read set in which exactly one
    sub-batch is withheld: with the overflow list cut to 3 entries a step is withheld once MORE than three entries were pushed, and a read of N alone never
    has a live candidate and is never pushed; so a sub-batch of one genome read and N reads is good (one push per strand at the most), a sub-batch of genome
    reads overruns.  Which sub-batch is which is asserted beforehand on a batch of each (its text is refused or not), and the state behind the refusing
    download equals the model over the good sub-batches' reads"""
    k = 31
    rng = np.random.default_rng(11)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    reads = sample_reads(rng, g, 500, 150)
    concat, ends = p.export(fa.X_CONCAT), p.export(fa.X_ENDS)
    total_len = p.total_len
    pairs = p.search_reads(reads, fa.FIN_MERGED)[0]   # (before the options change; the pairs are the same under every option)
    nk = 150 - k + 1
    # the read set of add_reads: sub-batches of at most 20 000 k-mers, that is 166 reads; [one kept genome read with a mismatch + 165 reads of N] twice, 166 genome
    # reads, [one kept genome read with a mismatch + 5 reads of N]
    alone = [pileup_model([reads[r]], pairs[r * nk:(r + 1) * nk], k, concat, ends, 8) for r in range(40)]
    kept = [r for r, w1 in enumerate(alone) if w1[2][KEPT] == 1 and w1[1].sum() >= 1][:3]
    assert len(kept) == 3
    per_sub = 20000 // nk
    n_read = "N" * 150
    subs = [[reads[kept[0]]] + [n_read] * (per_sub - 1), [reads[kept[1]]] + [n_read] * (per_sub - 1), reads[100:100 + per_sub], [reads[kept[2]]] + [n_read] * 5]
    withheld = [False, False, True, False]
    assert all(len(s) == per_sub for s in subs[:3]) and per_sub * nk <= 20000 < (per_sub + 1) * nk   # the pipeline's cut: whole reads while the k-mers fit
    mixed = [r for s in subs for r in s]
    good_reads = [r for s, wh in zip(subs, withheld) if not wh for r in s]
    good_pairs = p.search_reads(good_reads, fa.FIN_MERGED)[0]
    w_good = pileup_model(good_reads, good_pairs, k, concat, ends, 8)
    assert w_good[2][KEPT] == 3 and w_good[2].sum() == len(good_reads) and w_good[0].sum() == 3 * 150 and w_good[1].sum() >= 3
    L = fa.lib()
    a = p.pileup()

    def refused():
        for call in (a.download, a.download, lambda: a.call(2, 200), lambda: a.call(1, 0)):
            with pytest.raises(fa.FinitoError) as e:
                call()
            assert e.value.code == fa.FIN_ELIMIT and "overflow list" in str(e.value)

    def holds(want3, what):
        """behind the refusing download: cover, alt and counters; want3 None: nothing at all"""
        cover, alt, counters = flagged_state(a, total_len)
        if want3 is None:
            assert not cover.any() and not alt.any() and counters.tolist() == [0, 0, 0, 0], "%s: cover %d, alt %d, counters %s" % (what, cover.sum(), alt.sum(), counters)
        else:
            assert counters.tolist() == want3[2].tolist(), "%s: counters %s, the model over the good sub-batches %s" % (what, counters, want3[2])
            assert np.array_equal(cover, want3[0]) and np.array_equal(alt, want3[1]), what

    def clean(what):
        cover, alt, counters = a.reset().download()
        assert not cover.any() and not alt.any() and not counters.any(), what
        assert len(a.call(1, 0)) == 0

    try:
        assert L.fin_set_option(b"lds_deque_limit", 1) == 0 and L.fin_set_option(b"seed_anchors", 0) == 0 and L.fin_set_option(b"debug_ovf_cap", 3) == 0
        for mode in (0, 2):
            b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
            a.add(b)                                   # nobody has looked at the step's overflow counter yet: the kernel does
            refused()
            holds(None, "a withheld step added something (mode %d)" % mode)
            clean("after the reset (mode %d)" % mode)
            with pytest.raises(fa.FinitoError) as e:   # once the host knows (a download looked), the add itself refuses
                b.download(want_pairs=False) if mode == 0 else b.text()
            assert e.value.code == fa.FIN_ELIMIT
            with pytest.raises(fa.FinitoError) as e:
                a.add(b)
            assert e.value.code == fa.FIN_ELIMIT
            assert not a.download()[2].any()
            b.close()
        for s, wh in zip(subs, withheld):              # the sub-batches are what they are meant to be: the step of each, asked for its text
            b = p.batch(s); b.text_mode(2); b.run(fa.FIN_MERGED)
            if wh:
                with pytest.raises(fa.FinitoError) as e:
                    b.text()
                assert e.value.code == fa.FIN_ELIMIT
            else:
                b.text()
            b.close()
        p.set_option("pipeline_kmers", 20000)
        try:
            a.add_reads(mixed)                         # four sub-batches, the third withheld
            refused()
            holds(w_good, "add_reads: the good sub-batches add, the withheld one adds nothing")
            clean("after add_reads with a withheld sub-batch")
            a.add_reads(reads[:3 * per_sub])           # three sub-batches of genome reads alone: every one withheld
            refused()
            holds(None, "add_reads, every sub-batch withheld")
            clean("after add_reads with every sub-batch withheld")
        finally:
            p.set_option("pipeline_kmers", None)
        assert L.fin_set_option(b"debug_ovf_cap", 0) == 0
        w = pileup_model(reads, pairs, k, concat, ends, 8)
        assert w[2][KEPT] > 100 and w[1].sum() > 100   # (unitigs of at most 500 bases: half the reads cross an end)
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        assert_pileup(a.add(b).download(), w, "a good step after the reset")
        assert_variants(a.call(1, 0), call_model(w[0], w[1], ends, concat, 1, 0), "the call of a good step after the reset")
        b.close()
        p.set_option("pipeline_kmers", 20000)
        try:
            assert_pileup(a.reset().add_reads(reads).download(), w, "add_reads in sub-batches after the reset")
        finally:
            p.set_option("pipeline_kmers", None)
    finally:
        L.fin_set_option(b"lds_deque_limit", 16); L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"debug_ovf_cap", 0)
        a.close(); p.close()


# ---- 5. the call past its first level ----------------------------------------------------------------------------------------------------------------------------
CALL_CHUNK = 256 * 4096                    # fin_capi.cpp: PILEUP_CALL_CHUNK_TILES tiles of fin_depth_max_tile() positions
BOUNDARIES = (1024, 262_144, CALL_CHUNK)   # one scan thread's first boundary at four blocks a thread; 1024 blocks; the chunk's end


def place_near(t, ends, starts, L, step):
    """the text position nearest t in direction `step` whose unitig has room for four different reads of L bases over it"""
    while True:
        u = int(np.searchsorted(ends, t, side="right"))
        if int(ends[u] - starts[u]) >= L + 40:
            return t, u
        t += step


def stack_over(t, u, ends, starts, text, L, alt_base, rng):
    """four reads of L bases over text position t inside unitig u, three of them with `alt_base` at t, each on a strand of its own choosing"""
    lo, hi = max(int(starts[u]), t - L + 1), min(t, int(ends[u]) - L)
    assert lo <= hi
    out = []
    for j, a in enumerate(np.linspace(lo, hi, 4).astype(np.int64)):
        s = list(text[a:a + L])
        if j != 2:
            s[t - a] = alt_base
        s = "".join(s)
        out.append(rc(s) if rng.random() < 0.5 else s)
    return out


@pytest.mark.gpu
def test_the_call_past_one_block_a_scan_thread():
    """a 1.2 Mbp index at k = 31 and the production tile: more than 1 048 576 positions, so fin_pileup_call has two chunks -- the second with g_base != 0, out +
    total and the cover carried over -- and the first has 4096 blocks of 256 positions, four to a thread of fin_blk_scan_kernel.  2 000 genome reads with
    substitutions and stacks placed on both sides of text positions 1024, 262 144 and 1 048 576, in the first block of the text and in its last"""
    k, L = 31, 150
    g = synth.genome(1_200_000, seed=51)
    u = synth.unitigs(g, k)
    p = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    try:
        concat, ends = p.export(fa.X_CONCAT), p.export(fa.X_ENDS).astype(np.int64)
        starts = np.concatenate([[0], ends[:-1]])
        total_len = p.total_len
        assert CALL_CHUNK + 4096 < total_len < 2 * CALL_CHUNK
        text = "".join("ACGT"[c] for c in concat)
        rng = np.random.default_rng(52)
        reads = synth.reads(g, 2000, seed=53).strings()
        spots = []
        for P in BOUNDARIES:
            spots += [place_near(P - 1, ends, starts, L, -1), place_near(P, ends, starts, L, 1)]
        spots += [place_near(0, ends, starts, L, 1), place_near(100, ends, starts, L, 1), place_near(total_len - 1, ends, starts, L, -1),
                  place_near(total_len - 90, ends, starts, L, -1)]
        for t, uu in spots:
            reads += stack_over(t, uu, ends, starts, text, L, _OTHER[text[t]][int(rng.integers(0, 3))], rng)
        pairs = p.search_reads(reads, fa.FIN_MERGED)[0]
        w = pileup_model(reads, pairs, k, concat, ends, 8)
        cover, alt = w[0], w[1]
        assert w[2][KEPT] > 1500 and len(reads) * L < 400_000
        a = p.pileup().add_reads(reads)
        assert_pileup(a.download(), w, "download: the cover carried across the chunks")
        last_block = (total_len - 1) // 256 * 256
        counts = {}
        for min_alt, pm in CALLS:
            wv = call_model(cover, alt, ends, concat, min_alt, pm)
            gw = starts[wv["u"]] + wv["off"]
            for P in BOUNDARIES:   # candidates on both sides of every boundary, in the first block and in the last
                assert ((gw >= P - 256) & (gw < P)).any() and ((gw >= P) & (gw < P + 256)).any(), "no candidate beside %d" % P
            assert (gw < 256).any() and (gw >= last_block).any()
            got = a.call(min_alt, pm)
            assert_variants(got, wv, "call(%d, %d)" % (min_alt, pm))
            gg = starts[got["u"]] + got["off"]
            assert (np.diff(gg) > 0).all()
            counts[(min_alt, pm)] = (len(wv), int((gw < CALL_CHUNK).sum()))
        # capacity
        n, n_first = counts[(2, 200)]
        assert 0 < n_first < n
        wv = call_model(cover, alt, ends, concat, 2, 200)
        assert_variants(a.call(2, 200, cap=n), wv, "cap = the count")
        err = C.create_string_buffer(512); cnt = C.c_uint64(0)
        out = np.zeros(n, dtype=fa.VARIANT_DTYPE)
        for cap in (n - 1, n_first):   # one less than the count; room for the first chunk's candidates only
            rc_ = a.L.fin_pileup_call(a.h, 2, 200, out.ctypes.data_as(C.c_void_p), cap, C.byref(cnt), err, 512)
            assert rc_ == fa.FIN_ELIMIT and cnt.value == n, "cap %d: rc %d, count %d, model %d" % (cap, rc_, cnt.value, n)
        assert_pileup(a.download(), w, "the call leaves the accumulator as it is")
        a.close()
    finally:
        p.close()

