"""Taxonomic classification, the parts that need no GPU (include/finito_amd.h: fin_unitig_lca_labels, fin_records_read_taxa, fin_taxa_clade_reads):
the definitions written out in plain Python -- the model every taxa test holds the device and the host twins against, byte for byte -- the host twins against
it, and taxonomy_order.

The definitions.  parent[n_taxa]: taxon 0 is the root, parent[0] == 0, parent[t] < t.  label[u] = the LCA of color_taxon[c] over the set colours c of unitig u,
NONE for an empty row.  For a read, c[t] = its found slots whose unitig's label is t; score(t) = the sum of c[a] over the a with c[a] > 0 on t's root path;
S = max score; call = the LCA of every t at S; clade(t) = the sum of c[x] over x at or below t; while 1000 * clade(call) < confidence * nk or
clade(call) < max(min_found, 1): unclassified at the root, else call = parent[call]."""
import numpy as np
import pytest

import finito_amd as fa
from tests.test_colors_host import pack, unpack
from tests.util import hand_made_case

NONE = fa.FIN_NO_LABEL


# ---- the model ----
def path_of(parent, t):
    """t, its parent, ..., the root"""
    out = [int(t)]
    while out[-1] != 0:
        out.append(int(parent[out[-1]]))
    return out


def lca_of(parent, taxa):
    """the deepest taxon on every one's root path; NONE for none"""
    taxa = list(taxa)
    if not taxa:
        return NONE
    common = set(path_of(parent, taxa[0]))
    for t in taxa[1:]:
        common &= set(path_of(parent, t))
    return max(common)   # (on one path the deepest node has the largest number)


def labels_of(bits, n_colors, parent, color_taxon):
    member = unpack(bits, n_colors)
    return np.array([lca_of(parent, {int(color_taxon[c]) for c in np.flatnonzero(row)}) for row in member], dtype=np.uint32)


def call_of(slot_labels, nk, parent, min_found=1, confidence=0):
    """(taxon, score, clade, n_labelled) of one read from the labels of its found slots (NONE among them: no vote)"""
    c = {}
    for L in slot_labels:
        if L != NONE:
            c[int(L)] = c.get(int(L), 0) + 1
    if not c:
        return (NONE, 0, 0, 0)
    n_labelled = sum(c.values())
    paths = {t: set(path_of(parent, t)) for t in c}
    score = {t: sum(c[a] for a in c if a in paths[t]) for t in c}
    S = max(score.values())
    call = lca_of(parent, [t for t in c if score[t] == S])
    while True:
        clade = sum(c[x] for x in c if call in paths[x])
        if not (1000 * clade < confidence * nk or clade < max(min_found, 1)):
            return (call, S, clade, n_labelled)
        if call == 0:
            return (NONE, S, n_labelled, n_labelled)
        call = int(parent[call])


def read_taxa_of(pairs, nks, labels, parent, min_found=1, confidence=0):
    """READ_TAXON_DTYPE[n_reads] from pairs [n, 2] (read r's are the nks[r] after those of the reads before it); a unitig at or above len(labels) has no label"""
    out = np.zeros(len(nks), dtype=fa.READ_TAXON_DTYPE)
    at = 0
    for r, nk in enumerate(nks):
        us = pairs[at:at + int(nk), 0]
        at += int(nk)
        out[r] = call_of([labels[u] for u in us if 0 <= u < len(labels)], int(nk), parent, min_found, confidence)
    return out


def clades_of(direct, parent):
    out = np.zeros(len(parent), dtype=np.uint64)
    for t in np.flatnonzero(np.asarray(direct)[: len(parent)]):
        for x in path_of(parent, t):
            out[x] += np.uint64(direct[t])
    return out


def tally_of(taxa, n_taxa):
    direct = np.zeros(n_taxa + 1, dtype=np.uint64)
    for t in taxa["taxon"]:
        direct[n_taxa if t == NONE else int(t)] += np.uint64(1)
    return direct


def assert_taxa(got, want, what=""):
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0 and got.tobytes() == want.tobytes(), "%s: %d of %d reads differ, first %d: got %s, want %s" % (
        what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


# ---- trees ----
def chain(n):
    return np.maximum(np.arange(n, dtype=np.int64) - 1, 0).astype(np.uint32)


def star(n):
    return np.zeros(n, dtype=np.uint32)


def random_tree(rng, n, near=None):
    """parent[t] uniform below t, or (near) among the `near` taxa just below t: a deeper tree"""
    p = np.zeros(n, dtype=np.uint32)
    for t in range(1, n):
        p[t] = rng.integers(max(0, t - near) if near else 0, t)
    return p


def trees(rng, n_colors):
    """(name, parent, color_taxon): a single node, a chain of depth 300, a star, a random tree, all colours on one taxon"""
    n = max(n_colors, 2)
    rt = random_tree(rng, min(3 * n, 600), near=6)
    return [("single node", star(1), np.zeros(n_colors, dtype=np.uint32)),
            ("chain", chain(300), rng.integers(0, 300, n_colors).astype(np.uint32)),
            ("star", star(n + 1), (1 + np.arange(n_colors) % n).astype(np.uint32)),
            ("random", rt, rng.integers(0, len(rt), n_colors).astype(np.uint32)),
            ("one taxon", random_tree(rng, 40), np.full(n_colors, 17, dtype=np.uint32))]


def edge_rows(rng, n_unitigs, n_colors):
    """rows with 0, 1, 2 and all colours set, bits in the first and in the last word only, the last colour alone, and random small rows"""
    sets = []
    for u in range(n_unitigs):
        kind = u % 8
        if kind == 0: s = []
        elif kind == 1: s = [int(rng.integers(0, n_colors))]
        elif kind == 2: s = [int(x) for x in rng.integers(0, n_colors, 2)]
        elif kind == 3 and u < 40: s = list(range(n_colors))
        elif kind == 4: s = [int(x) for x in rng.integers(0, min(n_colors, 64), 3)]
        elif kind == 5: s = [int(x) for x in rng.integers(64 * ((n_colors - 1) // 64), n_colors, 3)]
        elif kind == 6: s = [n_colors - 1]
        else: s = [int(x) for x in rng.integers(0, n_colors, int(rng.integers(1, 9)))]
        sets.append(s)
    return pack(sets, n_colors)


# ---- the model on cases worked by hand ----
#        0
#      1   2
#     3 4   5
#    6      7 8
TREE = np.array([0, 0, 0, 1, 1, 2, 3, 5, 5], dtype=np.uint32)


def test_the_model_on_small_reads():
    """pins the plain-Python model itself by cases worked by hand (it calls nothing of the library: the twins face the same cases in the next test)"""
    assert lca_of(TREE, [6, 4]) == 1 and lca_of(TREE, [7, 8]) == 5 and lca_of(TREE, [6, 8]) == 0 and lca_of(TREE, [6, 3]) == 3 and lca_of(TREE, []) == NONE
    assert call_of([3, 4], 2, TREE) == (1, 1, 2, 2)                     # a tie between siblings: the parent
    assert call_of([6, 4], 2, TREE) == (1, 1, 2, 2)                     # an uncle and a nephew tie: their LCA
    assert call_of([6, 7], 2, TREE) == (0, 1, 2, 2)                     # cousins across the root
    assert call_of([3, 3, 4], 3, TREE) == (3, 2, 2, 3)
    assert call_of([1, 6], 2, TREE) == (6, 2, 1, 2)                     # a hit on an ancestor counts for the deeper hit
    assert call_of([1, 6, 4, 4], 4, TREE) == (4, 3, 2, 4)               # ... and for every deeper hit
    assert call_of([1, 3, 6], 3, TREE) == (6, 3, 1, 3)                  # all on one chain: the deepest
    assert call_of([1, 3, 6], 3, TREE, confidence=500) == (3, 3, 2, 3)  # 1000 * 1 < 500 * 3, 1000 * 2 >= 1500
    assert call_of([1, 3, 6], 4, TREE, confidence=750) == (1, 3, 3, 3)  # equality: 1000 * 3 == 750 * 4 does not lift
    assert call_of([1, 3, 6], 4, TREE, confidence=751) == (NONE, 3, 3, 3)
    assert call_of([1, 3, 6], 3, TREE, min_found=3) == (1, 3, 3, 3) and call_of([1, 3, 6], 3, TREE, min_found=4) == (NONE, 3, 3, 3)
    assert call_of([NONE, NONE], 2, TREE) == (NONE, 0, 0, 0) and call_of([], 0, TREE) == (NONE, 0, 0, 0)
    assert call_of([0], 1, TREE, confidence=1000) == (0, 1, 1, 1) and call_of([0], 2, TREE, confidence=1000) == (NONE, 1, 1, 1)
    assert np.array_equal(clades_of([1, 0, 2, 0, 5, 0, 3, 0, 1], TREE), [12, 8, 3, 3, 5, 1, 3, 0, 1])


def test_the_twins_on_the_same_small_reads():
    """the hand-worked cases above through fin_records_read_taxa and fin_taxa_clade_reads: unitig u is labelled u, a searched read's stream pairs are its slots"""
    reads = [([3, 4], 0, (1, 1, 2, 2)), ([6, 4], 0, (1, 1, 2, 2)), ([6, 7], 0, (0, 1, 2, 2)), ([3, 3, 4], 0, (3, 2, 2, 3)), ([1, 6], 0, (6, 2, 1, 2)),
             ([1, 6, 4, 4], 0, (4, 3, 2, 4)), ([1, 3, 6], 0, (6, 3, 1, 3)), ([1, 3, 6], 500, (3, 3, 2, 3)), ([1, 3, 6, -1], 750, (1, 3, 3, 3)),
             ([1, 3, 6, -1], 751, (NONE, 3, 3, 3)), ([-1, -1], 0, (NONE, 0, 0, 0)), ([0], 1000, (0, 1, 1, 1)), ([0, -1], 1000, (NONE, 1, 1, 1))]
    labels = np.arange(9, dtype=np.uint32)
    for slots, conf, want in reads:
        recs = np.zeros(1, dtype=fa.RECORD_DTYPE)
        recs["nk"] = len(slots)   # kind 0: a searched read
        stream = np.array([(u, 0) if u >= 0 else (-1, -1) for u in slots], dtype=np.int32)
        got = fa.records_read_taxa(recs, stream, 31, labels, TREE, 1, conf)
        assert tuple(got[0].tolist()) == want == call_of([u for u in slots if u >= 0], len(slots), TREE, 1, conf), (slots, conf, got[0])
    for mf, want in ((3, (1, 3, 3, 3)), (4, (NONE, 3, 3, 3))):
        recs = np.zeros(1, dtype=fa.RECORD_DTYPE); recs["nk"] = 3
        got = fa.records_read_taxa(recs, np.array([(1, 0), (3, 0), (6, 0)], dtype=np.int32), 31, labels, TREE, mf, 0)
        assert tuple(got[0].tolist()) == want
    assert np.array_equal(fa.taxa_clade_reads([1, 0, 2, 0, 5, 0, 3, 0, 1], TREE), [12, 8, 3, 3, 5, 1, 3, 0, 1])


# ---- the host twins against the model ----
@pytest.mark.parametrize("n_colors", [1, 5, 64, 65, 130, 4096])
def test_host_labels_against_the_model(n_colors):
    rng = np.random.default_rng(2400 + n_colors)
    bits = edge_rows(rng, 130, n_colors)
    for name, parent, ct in trees(rng, n_colors):
        want = labels_of(bits, n_colors, parent, ct)
        for threads in (1, 3):
            got = fa.unitig_lca_labels(bits, n_colors, parent, ct, threads)
            assert got.dtype == np.uint32 and np.array_equal(got, want), "%s, %d colours" % (name, n_colors)
        assert (want == NONE).sum() == sum(1 for u in range(130) if u % 8 == 0)


@pytest.mark.parametrize("k", [16, 31])
def test_host_read_taxa_of_hand_made_records(k):
    """records of every kind, both strands, every gap shape: the twin works from records + stream, the model from the pairs they mean"""
    c = hand_made_case(k)
    rng = np.random.default_rng(2450 + k)
    nu = len(c.unitigs)
    for name, parent in (("random", random_tree(rng, 90, near=5)), ("chain", chain(300)), ("star", star(50)), ("single node", star(1))):
        labels = rng.integers(0, len(parent), nu).astype(np.uint32)
        labels[rng.random(nu) < 0.2] = NONE
        for mf, conf in ((1, 0), (0, 0), (5, 0), (1, 300), (1, 1000), (40, 900)):
            want = read_taxa_of(c.pairs, c.nks, labels, parent, mf, conf)
            for threads in (1, 3):
                assert_taxa(fa.records_read_taxa(c.recs, c.stream, k, labels, parent, mf, conf, threads), want, "%s, k=%d, rule %s" % (name, k, (mf, conf)))
        if name == "random":
            w = read_taxa_of(c.pairs, c.nks, labels, parent)
            lifted = read_taxa_of(c.pairs, c.nks, labels, parent, 1, 300)
            assert (w["taxon"] != NONE).any() and (w["taxon"] == NONE).any() and (w["score"] > w["clade"]).any() and (w["clade"] < w["n_labelled"]).any()
            assert ((lifted["taxon"] != w["taxon"]) & (lifted["taxon"] != NONE)).any() and ((lifted["taxon"] == NONE) & (lifted["score"] > 0)).any()


def test_host_clades_against_the_model():
    rng = np.random.default_rng(2460)
    for parent in (star(1), chain(300), star(65), random_tree(rng, 64), random_tree(rng, 1000, near=4)):
        direct = rng.integers(0, 1 << 40, len(parent) + 1).astype(np.uint64)
        direct[rng.random(len(direct)) < 0.5] = 0
        got = fa.taxa_clade_reads(direct, parent)
        assert np.array_equal(got, clades_of(direct, parent)) and got[0] == direct[:-1].sum()


def test_refusals():
    good = TREE
    bits = pack([[0], [1, 2]], 3)
    ct = np.array([6, 7, 8], dtype=np.uint32)
    assert np.array_equal(fa.unitig_lca_labels(bits, 3, good, ct), [6, 5])
    for bad in (np.array([1, 0], dtype=np.uint32), np.array([0, 1], dtype=np.uint32), np.array([0, 0, 3, 0], dtype=np.uint32)):   # the root, a self loop, a parent above
        with pytest.raises(fa.FinitoError) as e:
            fa.unitig_lca_labels(bits, 3, bad, np.zeros(3, dtype=np.uint32))
        assert e.value.code == fa.FIN_EINVAL
        with pytest.raises(fa.FinitoError):
            fa.taxa_clade_reads(np.zeros(len(bad), dtype=np.uint64), bad)
    with pytest.raises(fa.FinitoError) as e:   # a colour's taxon outside the tree
        fa.unitig_lca_labels(bits, 3, good, np.array([6, 7, 9], dtype=np.uint32))
    assert e.value.code == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:   # a bit at or above n_colors
        fa.unitig_lca_labels(pack([[3]], 4), 3, good, ct)
    assert e.value.code == fa.FIN_EINVAL
    c = hand_made_case(16)
    labels = np.zeros(len(c.unitigs), dtype=np.uint32)
    for kw in (dict(confidence=1001), dict(parent=np.array([0, 1], dtype=np.uint32))):
        with pytest.raises(fa.FinitoError) as e:
            fa.records_read_taxa(c.recs, c.stream, 16, labels, kw.get("parent", good), 1, kw.get("confidence", 0))
        assert e.value.code == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError):   # a label outside the tree
        fa.records_read_taxa(c.recs, c.stream, 16, labels + 9, good)
    with pytest.raises(fa.FinitoError):   # not this record set's stream
        fa.records_read_taxa(c.recs, c.stream[:-1], 16, labels, good)


def test_taxonomy_order():
    # NCBI-like ids, the root its own parent, children given before their parents
    ids = [9606, 1, 131567, 2, 562, 561]
    pids = [131567, 1, 1, 131567, 561, 2]
    order, parent = fa.taxonomy_order(ids, pids)
    assert order[1] == 0 and parent[0] == 0 and sorted(order) == list(range(6))
    assert all(parent[t] < t for t in range(1, 6))
    for i in range(6):   # the same tree
        assert parent[order[i]] == order[ids.index(pids[i])]
    assert fa.taxonomy_order([7], [7])[1].tolist() == [0]
    for ids, pids, word in (([1, 2, 3], [1, 3, 2], "cycle"), ([1, 2], [1, 5], "unknown parent"), ([1, 2, 3], [1, 2, 1], "more than one root"),
                            ([1, 2], [2, 1], "no root"), ([1, 2, 2], [1, 1, 1], "twice")):
        with pytest.raises(ValueError) as e:
            fa.taxonomy_order(ids, pids)
        assert word in str(e.value), (word, str(e.value))
    # what it makes is what the library accepts
    rng = np.random.default_rng(2470)
    p = random_tree(rng, 200)
    names = rng.permutation(10 ** 6)[:200]
    shuffle = rng.permutation(200)
    order, parent = fa.taxonomy_order(names[shuffle], names[p][shuffle])
    assert np.array_equal(fa.taxa_clade_reads(np.ones(200, dtype=np.uint64), parent)[order[np.argsort(shuffle)]], clades_of(np.ones(200), p))
