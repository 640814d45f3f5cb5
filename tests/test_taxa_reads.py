"""A taxon per read by Kraken's root-to-leaf rule, on the device (include/finito_amd.h: fin_batch_taxa, fin_search_batch_taxa; fin_taxa.hip's per-read kernel).
The expectation is the plain-Python model of tests/test_taxa_host.py over hand-made pairs, hand-made records or the oracle's pairs -- never a device output;
device, host twin and model are equal byte for byte."""
import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.test_records_device import inject
from tests.test_segments import nks_of, oracle_pairs
from tests.test_taxa_host import NONE, assert_taxa, chain, random_tree, read_taxa_of, star
from tests.test_unitig_counts import read_families
from tests.util import cut_unitigs, hand_made_case, random_genome

pytestmark = pytest.mark.gpu

RULES = [(1, 0), (0, 0), (1, 500), (1, 750), (1, 751), (3, 0), (4, 0), (1, 1000), (2, 333), (1, 50), (1, 20)]   # (min_found, confidence)
A = (-1, -1)


@pytest.fixture(scope="module")
def wide():
    """an index of more than 200 unitigs; with label[u] = u a hand-made pair (u, off) is one vote for taxon u"""
    k = 31
    rng = np.random.default_rng(2600)
    g = random_genome(rng, 12000)
    p = fa.FinimizerIndex.build(cut_unitigs(rng, g, k, max_len=80), k).to_device(0)
    assert p.n_unitigs >= 200
    yield p, rng
    p.close()


def designed_tree(n):
    """0 the root; 1, 2 below it; 3, 4 below 1; 5 below 2; 6 below 3; 7, 8 below 5; 9 .. 49 a chain below 8; ten genera 50 .. 59 below 4; leaf t >= 60 below
    genus 50 + t % 10"""
    p = np.zeros(n, dtype=np.uint32)
    p[:9] = [0, 0, 0, 1, 1, 2, 3, 5, 5]
    p[9:50] = np.arange(8, 49)
    p[50:60] = 4
    p[60:] = 50 + np.arange(60, n) % 10
    return p


def designed_cases(nu, rng):
    v = lambda *ts: [(t, 0) for t in ts]
    cases = {}
    cases["siblings tie"] = v(3, 4)
    cases["cousins tie"] = v(6, 4, 4, 6)
    cases["across the root"] = v(6, 7)
    cases["an ancestor and a deeper hit"] = v(1, 6)
    cases["an ancestor and two deeper hits"] = v(1, 6, 4, 4)
    cases["one chain"] = v(1, 3, 6)
    cases["one chain and an absent slot"] = v(1, 3, 6) + [A]          # nk = 4: confidence 750 is met with equality at taxon 1
    cases["the root alone"] = v(0)
    cases["the root and an absent slot"] = v(0) + [A]
    cases["the deep chain"] = v(*range(9, 50))                           # lifting walks it
    cases["the deep chain, its end thrice, 100 slots"] = v(*range(9, 50)) + v(49, 49) + [A] * 57
    cases["a unitig beyond the index"] = [(nu + 5, 0), (3, 0), (nu, 1), (0x7FFFFFFF, 0)]
    cases["only unitigs beyond the index"] = [(nu, 0), (nu + 1, 0)]
    for nk in (1, 64, 65, 129):
        cases["%d slots, one taxon" % nk] = [(77, i) for i in range(nk)]
        cases["%d slots, nothing" % nk] = [A] * nk
        cases["%d slots, the last one only" % nk] = [A] * (nk - 1) + [(6, 0)]
        if nk > 1:
            cases["%d slots, a run across the row edge" % nk] = [(61, i) for i in range(nk - 2)] + [(71, 0), (3, 0)]
    # exactly 64, 65 and 130 distinct taxa: leaf 196 thrice, leaf 197 twice, every other leaf once.  With genus 57 thrice -- a small number: it is counted in the
    # first label range -- leaf 197, of the last range, wins by its ancestor's count; without it 196 does.  Leaves in random order, the deciding slots last
    for n in (64, 65, 130):
        leaves = [196, 197] + [int(t) for t in 60 + rng.permutation(136)[: n - 3]]
        assert len(set(leaves)) == n - 1 and 198 not in leaves
        body = [int(t) for t in rng.permutation(leaves)]
        cases["%d taxa, an ancestor decides" % n] = v(*body) + v(196, 196, 197, 57, 57, 57)
        cases["%d taxa, no ancestor" % n] = v(*body) + v(196, 196, 197, 198)
    cases["140 leaves once"] = v(*range(199, 59, -1))                  # every leaf at score 1: the call is genus-of-all = 4
    cases["140 leaves and the chain"] = v(*range(60, 200)) + v(*range(9, 50))   # 181 taxa; the chain's end has score 41
    return cases


def test_designed_reads_and_rules(wide):
    p, rng = wide
    k, nu = 31, p.n_unitigs
    cases = designed_cases(nu, rng)
    names = list(cases)
    # every read once more with its slots reversed
    pairs = np.array([x for n in names for x in cases[n]] + [x for n in names for x in cases[n][::-1]], dtype=np.int32)
    nks = np.array([len(cases[n]) for n in names] * 2)
    reads = [random_genome(rng, int(nk) + k - 1) for nk in nks]
    parent = designed_tree(nu)
    labels = np.arange(nu, dtype=np.uint32)
    want = {rule: read_taxa_of(pairs, nks, labels, parent, *rule) for rule in RULES}
    w = dict(zip(names, (tuple(x) for x in want[(1, 0)].tolist())))
    assert w["siblings tie"] == (1, 1, 2, 2) and w["cousins tie"] == (1, 2, 4, 4) and w["across the root"] == (0, 1, 2, 2)
    assert w["an ancestor and a deeper hit"] == (6, 2, 1, 2) and w["an ancestor and two deeper hits"] == (4, 3, 2, 4) and w["one chain"] == (6, 3, 1, 3)
    assert w["a unitig beyond the index"] == (3, 1, 1, 1) and w["only unitigs beyond the index"] == (NONE, 0, 0, 0)
    assert w["64 taxa, an ancestor decides"] == (197, 5, 2, 69) and w["64 taxa, no ancestor"] == (196, 3, 3, 67)
    assert w["65 taxa, an ancestor decides"] == (197, 5, 2, 70) and w["130 taxa, an ancestor decides"] == (197, 5, 2, 135) and w["130 taxa, no ancestor"] == (196, 3, 3, 133)
    for n in (64, 65, 130):
        for kind in ("an ancestor decides", "no ancestor"):
            assert len({t for t, _ in cases["%d taxa, %s" % (n, kind)]}) == n
    assert w["140 leaves once"] == (4, 1, 140, 140) and w["140 leaves and the chain"] == (49, 41, 1, 181) and w["the deep chain"] == (49, 41, 1, 41)
    lifted = {rule: dict(zip(names, (tuple(x) for x in want[rule].tolist()))) for rule in RULES}
    assert lifted[(1, 750)]["one chain and an absent slot"] == (1, 3, 3, 3) and lifted[(1, 751)]["one chain and an absent slot"] == (NONE, 3, 3, 3)   # equality
    assert lifted[(1, 500)]["one chain"] == (3, 3, 2, 3) and lifted[(3, 0)]["one chain"] == (1, 3, 3, 3) and lifted[(4, 0)]["one chain"] == (NONE, 3, 3, 3)
    assert lifted[(1, 500)]["the deep chain"] == (29, 41, 21, 41)     # twenty levels up
    assert lifted[(1, 1000)]["the root and an absent slot"] == (NONE, 1, 1, 1) and lifted[(1, 1000)]["the root alone"] == (0, 1, 1, 1)
    below57 = sum(1 for t, _ in cases["130 taxa, an ancestor decides"] if t == 57 or (t >= 60 and t % 10 == 7))
    assert below57 > 5 and lifted[(1, 20)]["130 taxa, an ancestor decides"] == (57, 5, below57, 135)   # one level up, past the table's 64 entries
    assert lifted[(1, 500)]["140 leaves and the chain"] == (0, 41, 181, 181) and lifted[(1, 1000)]["140 leaves and the chain"] == (0, 41, 181, 181) and lifted[(1, 50)]["140 leaves and the chain"][0] in range(9, 49)
    for rule in RULES:   # reversing the slots changes nothing
        assert want[rule][: len(names)].tobytes() == want[rule][len(names):].tobytes()
    b = p.batch(reads); b.text_mode(0); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(pairs)
    tax = p.taxonomy(parent, labels)
    b.taxa(tax)
    assert b.device_read_taxa_ptr() != 0
    b.set_pairs(pairs)
    assert b.device_read_taxa_ptr() == 0   # forgotten
    for rule in RULES + RULES[:2]:   # (a call with other thresholds replaces the result)
        got = b.taxa(tax, *rule)
        assert got.dtype == fa.READ_TAXON_DTYPE
        for i in np.flatnonzero(got != want[rule]):
            raise AssertionError("rule %s, %s%s: got %s, want %s" % (rule, names[i % len(names)], " reversed" if i >= len(names) else "", got[i], want[rule][i]))
        assert got.tobytes() == want[rule].tobytes()
    # the same slots under other trees and labellings that merge unitigs
    for name, par in (("chain", chain(300)), ("star", star(66)), ("single node", star(1)), ("random", random_tree(rng, 500, near=8))):
        merged = rng.integers(0, len(par), nu).astype(np.uint32)
        merged[::17] = NONE
        t2 = p.taxonomy(par, merged)
        for rule in ((1, 0), (2, 100)):
            assert_taxa(b.taxa(t2, *rule), read_taxa_of(pairs, nks, merged, par, *rule), "%s tree, rule %s" % (name, rule))
        t2.close()
    b.close(); tax.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_hand_made_records_kinds_0_1_2_in_one_batch(mode):
    k = 31
    c = hand_made_case(k)
    rng = np.random.default_rng(2650 + mode)
    kinds = c.recs["meta"] >> 16
    assert all((kinds == q).any() for q in (0, 1, 2))
    parent = random_tree(rng, 120, near=5)
    labels = rng.integers(0, 120, len(c.unitigs)).astype(np.uint32)
    labels[rng.random(len(labels)) < 0.15] = NONE
    p = fa.FinimizerIndex.build(c.unitigs, k).to_device(0)
    tax = p.taxonomy(parent, labels)
    b = p.batch(c.reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
    b.taxa(tax)
    inject(b, c.recs, c.pairs, mode)
    assert b.device_read_taxa_ptr() == 0   # set_records forgets
    for rule in ((1, 0), (1, 300), (30, 0), (1, 1000), (0, 999)):
        want = read_taxa_of(c.pairs, c.nks, labels, parent, *rule)
        assert_taxa(b.taxa(tax, *rule), want, "text mode %d, rule %s" % (mode, rule))
        assert_taxa(fa.records_read_taxa(c.recs, c.stream, k, labels, parent, *rule), want, "the twin, rule %s" % (rule,))
        one = kinds == 1
        assert (want["score"][one] > 0).any() and (want["score"][one] == 0).any()
        if rule != (1, 0):   # under every other rule here some kind-1 reads keep their taxon and others are lifted out
            assert (want["taxon"][one] != NONE).any() and ((want["taxon"][one] == NONE) & (want["score"][one] > 0)).any(), rule
    b.close(); tax.close(); p.close()


def test_searched_reads_in_every_text_mode_host_buffers_forgetting_and_refusals():
    k = 31
    rng = np.random.default_rng(2670)
    g = random_genome(rng, 30000)
    unitigs = cut_unitigs(rng, g, k, max_len=300)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    reads = read_families(rng, g, k, unitigs)[:1500]
    nks = nks_of(reads, k)
    parent = random_tree(rng, 80, near=4)
    labels = rng.integers(0, 80, p.n_unitigs).astype(np.uint32)
    labels[rng.random(p.n_unitigs) < 0.1] = NONE
    tax = p.taxonomy(parent, labels)
    for strands in (fa.FIN_MERGED, fa.FIN_FWD):
        e = oracle_pairs(o, reads, strands)
        want = {rule: read_taxa_of(e, nks, labels, parent, *rule) for rule in ((1, 0), (5, 400))}
        assert (want[(1, 0)]["taxon"] != want[(5, 400)]["taxon"]).any() and (want[(1, 0)]["score"] > want[(1, 0)]["clade"]).any()
        for mode in (0, 1, 2):
            b = p.batch(reads); b.text_mode(mode); b.run(strands)
            assert b.device_read_taxa_ptr() == 0
            for rule in want:
                assert_taxa(b.taxa(tax, *rule), want[rule], "strands %d, text mode %d, rule %s" % (strands, mode, rule))
            recs, stream = b.records() if strands == fa.FIN_MERGED and mode != 0 else (None, None)
            if recs is not None:
                assert_taxa(fa.records_read_taxa(recs, stream, k, labels, parent, 5, 400), want[(5, 400)], "the twin from downloaded records, mode %d" % mode)
                assert_taxa(b.taxa(tax, 5, 400), want[(5, 400)], "after the records, mode %d" % mode)
            b.run(strands)
            assert b.device_read_taxa_ptr() == 0   # a run forgets
            b.taxa(tax)
            b.reload(reads[:100])
            assert b.device_read_taxa_ptr() == 0   # a reload forgets
            with pytest.raises(fa.FinitoError) as err:
                b.taxa(tax)
            assert err.value.code == fa.FIN_EINVAL
            b.close()
        assert_taxa(p.taxa_reads(reads, tax, 5, 400, strands), want[(5, 400)], "host buffers, strands %d" % strands)
    b = p.batch(reads[:50]); b.run(fa.FIN_MERGED)
    with pytest.raises(fa.FinitoError) as err:
        b.taxa(tax, confidence=1001)
    assert err.value.code == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as err:
        tax.add(b, confidence=1001)
    assert err.value.code == fa.FIN_EINVAL
    p2 = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    t2 = p2.taxonomy(parent, labels)
    for call in (lambda: b.taxa(t2), lambda: t2.add(b), lambda: p.taxa_reads(reads[:5], t2)):   # another index's taxonomy
        with pytest.raises(fa.FinitoError) as err:
            call()
        assert err.value.code == fa.FIN_EINVAL
    for rd in ([], ["", "AC"]):
        e = p.batch(rd); e.run(fa.FIN_MERGED)
        got = e.taxa(tax)
        assert len(got) == len(rd) and (got["taxon"] == NONE).all() and not got["n_labelled"].any()
        e.close()
    t2.close(); p2.close(); b.close(); tax.close(); p.close()
