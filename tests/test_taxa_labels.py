"""Unitig taxa from colours, on the device (include/finito_amd.h: fin_taxonomy_create_from_colors; fin_taxa.hip's two LCA kernels): label[u] = the LCA of the taxa
of unitig u's colours.  The expectation is the plain-Python model of tests/test_taxa_host.py over the uploaded matrix; device, host twin and model are equal
byte for byte."""
import numpy as np
import pytest
import torch

import finito_amd as fa
from tests.test_colors_host import pack, unpack
from tests.test_taxa_host import NONE, edge_rows, labels_of, random_tree, trees
from tests.util import random_genome

pytestmark = pytest.mark.gpu

K = 15
SIZES = [1, 63, 64, 65, 257, 1000]   # unitigs: a lane per unitig crosses wave and block edges at 64 and 256, a wave per unitig the block of four


@pytest.fixture(scope="module")
def indexes():
    """an index of exactly n unitigs for every n of SIZES: n random sequences of 20 .. 30 bases (distinct 15-mers, for all a test cares)"""
    rng = np.random.default_rng(2500)
    out = {}
    for n in SIZES:
        seqs = [random_genome(rng, int(rng.integers(20, 31))) for _ in range(n)]
        p = fa.FinimizerIndex.build(seqs, K).to_device(0)
        assert p.n_unitigs == n
        out[n] = (p, seqs)
    yield out
    for p, _ in out.values():
        p.close()


@pytest.mark.parametrize("n_colors", [1, 64, 65, 130, 4096])   # W = 1, 1, 2, 3, 64
def test_lca_labels_at_every_width_size_and_tree(indexes, n_colors):
    rng = np.random.default_rng(2510 + n_colors)
    forest = trees(rng, n_colors)
    for n in SIZES:
        p = indexes[n][0]
        bits = edge_rows(rng, n, n_colors)
        col = p.colors(n_colors, bits)
        for name, parent, ct in forest:
            want = labels_of(bits, n_colors, parent, ct)
            tax = col.taxonomy(parent, ct)
            got = tax.labels()
            assert got.dtype == np.uint32 and got.tobytes() == want.tobytes(), "%s, %d colours, %d unitigs: %d differ" % (name, n_colors, n, (got != want).sum())
            assert fa.unitig_lca_labels(bits, n_colors, parent, ct).tobytes() == want.tobytes()
            assert tax.n_taxa == len(parent) and tax.device_labels_ptr() != 0
            if n == 257 and name == "random":   # an ordinary labelling: the majority vote takes it as it is
                lab = tax.as_labels()
                assert lab.n_labels == len(parent)
                lab.close()
            tax.close()
        col.close()


def test_labels_behind_colour_adds_on_another_stream(indexes):
    """the matrix is coloured by search on a non-default stream and the taxonomy made at once: it waits for those adds"""
    p, seqs = indexes[1000]
    rng = np.random.default_rng(2530)
    S = torch.cuda.Stream()
    n_colors = 70
    col = p.colors(n_colors)
    parent = random_tree(rng, 50, near=4)
    ct = rng.integers(0, 50, n_colors).astype(np.uint32)
    batches = []
    for i, c in enumerate((0, 63, 64, 69)):   # each colour gets its own overlapping share of the unitigs
        b = p.batch(seqs[200 * i: 200 * i + 400]); b.run(fa.FIN_MERGED, stream=S.cuda_stream)
        col.add(b, c, stream=S.cuda_stream)
        batches.append(b)
    tax = col.taxonomy(parent, ct)
    bits = col.download()[0]
    per_unitig = unpack(bits, n_colors).sum(axis=1)
    assert per_unitig.min() >= 1 and (per_unitig == 1).any() and (per_unitig == 2).any()
    assert tax.labels().tobytes() == labels_of(bits, n_colors, parent, ct).tobytes()
    tax.close()
    for b in batches:
        b.close()
    col.close()


def test_refusals(indexes):
    p = indexes[65][0]
    col = p.colors(3, pack([[0, 1]] * 65, 3))
    good = np.array([0, 0, 0, 1], dtype=np.uint32)
    for parent, ct, word in ((np.array([0, 1], dtype=np.uint32), [0, 0, 0], "taxon 1"), (np.array([1, 0], dtype=np.uint32), [0, 0, 0], "taxon 0"),
                             (np.array([0, 0, 3, 0], dtype=np.uint32), [0, 0, 0], "taxon 2"), (good, [0, 4, 0], "colour 1")):
        with pytest.raises(fa.FinitoError) as e:
            col.taxonomy(parent, np.array(ct, dtype=np.uint32))
        assert e.value.code == fa.FIN_EINVAL and word in str(e.value), str(e.value)
    with pytest.raises(fa.FinitoError):
        col.taxonomy(good, np.zeros(2, dtype=np.uint32))   # not one taxon per colour
    with pytest.raises(fa.FinitoError) as e:   # a label outside the tree, named
        p.taxonomy(good, np.array([0] * 64 + [4], dtype=np.uint32))
    assert e.value.code == fa.FIN_EINVAL and "unitig 64" in str(e.value)
    tax = p.taxonomy(good, np.array([3] * 64 + [NONE], dtype=np.uint32))
    assert tax.labels().tolist() == [3] * 64 + [NONE]
    tax.close()
    col.close()
