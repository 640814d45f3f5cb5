"""The tally of reads per taxon and the clade counts, on the device (include/finito_amd.h: fin_batch_add_taxa, fin_taxonomy_download; fin_taxa.hip's tally and
clade kernels) against the plain-Python model of tests/test_taxa_host.py."""
import numpy as np
import pytest
import torch

import finito_amd as fa
from tests.test_taxa_host import NONE, chain, clades_of, random_tree, read_taxa_of, star, tally_of
from tests.util import cut_unitigs, random_genome

pytestmark = pytest.mark.gpu
K = 31


@pytest.fixture(scope="module")
def batch():
    """700 reads of hand-made pairs: one to three unitigs each, some empty"""
    rng = np.random.default_rng(2700)
    g = random_genome(rng, 12000)
    p = fa.FinimizerIndex.build(cut_unitigs(rng, g, K, max_len=80), K).to_device(0)
    nu = p.n_unitigs
    nks = rng.integers(1, 12, 700)
    pairs = np.full((int(nks.sum()), 2), -1, dtype=np.int32)
    at = 0
    for nk in nks:
        us = rng.integers(0, nu, int(rng.integers(0, 4)))
        for i in range(int(nk)):
            if len(us) and rng.random() < 0.8:
                pairs[at + i] = (us[rng.integers(0, len(us))], i)
        at += int(nk)
    reads = [random_genome(rng, int(nk) + K - 1) for nk in nks]
    b = p.batch(reads); b.text_mode(0); b.run(fa.FIN_MERGED)
    b.set_pairs(pairs)
    yield p, b, pairs, nks, rng
    b.close(); p.close()


def check(tax, want_taxa, parent, times, what):
    n = len(parent)
    direct, clade, unclassified = tax.download()
    want = tally_of(want_taxa, n) * np.uint64(times)
    assert np.array_equal(direct, want[:n]) and unclassified == int(want[n]), what
    assert clade.tobytes() == clades_of(want[:n], parent).tobytes() and clade.tobytes() == fa.taxa_clade_reads(want, parent).tobytes(), what
    assert int(clade[0]) + unclassified == times * len(want_taxa), what


@pytest.mark.parametrize("n_taxa", [1, 64, 65, 10000])
def test_direct_and_clade_counts(batch, n_taxa):
    p, b, pairs, nks, rng = batch
    S, T = torch.cuda.Stream(), torch.cuda.Stream()
    for name, parent in (("random", random_tree(rng, n_taxa, near=max(7, n_taxa // 100))), ("chain", chain(min(n_taxa, 300))), ("star", star(n_taxa))):
        labels = rng.integers(0, len(parent), p.n_unitigs).astype(np.uint32)
        labels[::11] = NONE
        tax = p.taxonomy(parent, labels)
        for rule in ((1, 0), (3, 600)):
            want = read_taxa_of(pairs, nks, labels, parent, *rule)
            what = "%s tree of %d taxa, rule %s" % (name, len(parent), rule)
            check(tax.reset().add(b, *rule), want, parent, 1, what)
            check(tax.add(b, *rule), want, parent, 2, what + ", added twice")
            check(tax.reset().add(b, *rule, stream=S.cuda_stream).add(b, *rule, stream=T.cuda_stream).add(b, *rule), want, parent, 3, what + ", three streams")
            check(tax.reset(stream=S.cuda_stream), want[:0], parent, 0, what + ", reset")
        assert (want["taxon"] == NONE).any() and (n_taxa == 1 or len(set(want["taxon"].tolist())) > 3)
        tax.close()


def test_every_read_on_one_deep_leaf(batch):
    """one hot address per ancestor: every lane of the clade kernel's one busy wave -- and every read of the tally -- meets the same taxa"""
    p, b, pairs, nks, rng = batch
    parent = chain(300)
    labels = np.full(p.n_unitigs, 299, dtype=np.uint32)
    tax = p.taxonomy(parent, labels)
    want = read_taxa_of(pairs, nks, labels, parent)
    n_hit = int((want["taxon"] == 299).sum())
    assert n_hit > 500 and n_hit + int((want["taxon"] == NONE).sum()) == len(nks)
    direct, clade, unclassified = tax.add(b).add(b).download()
    assert direct[299] == 2 * n_hit and direct[:299].sum() == 0 and (clade == 2 * n_hit).all() and unclassified == 2 * (len(nks) - n_hit)
    tax.close()
    # many taxa with counts under few ancestors: 64 lanes of a wave merge at their parents
    parent = np.concatenate([[0, 0, 0], 1 + np.arange(997) % 2]).astype(np.uint32)
    labels = (3 + np.arange(p.n_unitigs) % 997).astype(np.uint32)
    tax = p.taxonomy(parent, labels)
    check(tax.add(b), read_taxa_of(pairs, nks, labels, parent), parent, 1, "a thousand leaves under two nodes")
    tax.close()


def test_host_buffers_and_rollup_of_abundances(batch):
    p, b, pairs, nks, rng = batch
    parent = np.array([0, 0, 0, 1, 1, 2], dtype=np.uint32)
    col = p.colors(4)
    tax = col.taxonomy(parent, np.array([3, 4, 5, 3], dtype=np.uint32))
    assert np.array_equal(tax.rollup([0.5, 0.25, 0.125, 1.0]), [1.875, 1.75, 0.125, 1.5, 0.25, 0.125])
    with pytest.raises(fa.FinitoError):
        tax.rollup([1.0, 2.0])
    reads = [random_genome(rng, 100) for _ in range(40)]
    direct, clade, unclassified = tax.add_reads(reads).download()   # (no colours: every unitig is unlabelled)
    assert unclassified == 40 and not direct.any() and not clade.any()
    tax.close(); col.close()
