"""Colour by search, label by LCA, call reads: six references that share stretches under a three-level tree (include/finito_amd.h: fin_taxonomy_create_from_colors,
fin_batch_taxa).  An error-free read drawn from reference g touches only unitigs that carry colour g, so every label it meets lies on the root path of
color_taxon[g] -- and so does its call, an LCA of such labels lifted upward: every call is an ancestor-or-self of color_taxon[g], or unclassified."""
import numpy as np
import pytest

import finito_amd as fa
from tests.test_taxa_host import NONE, assert_taxa, labels_of, path_of
from tests.util import cut_unitigs, random_genome

pytestmark = pytest.mark.gpu


def test_reads_of_a_reference_are_called_on_its_root_path():
    k = 31
    rng = np.random.default_rng(2800)
    g = random_genome(rng, 16000)
    p = fa.FinimizerIndex.build(cut_unitigs(rng, g, k, max_len=120), k).to_device(0)
    step = len(g) // 8
    refs = [g[i * step: (i + 2) * step] for i in range(6)]   # neighbours share half of each other
    #      0
    #    1   2
    #  3 4 5 6 7 8
    parent = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2], dtype=np.uint32)
    ct = np.array([3, 4, 5, 6, 7, 8], dtype=np.uint32)
    col = p.colors(6)
    for i, ref in enumerate(refs):
        col.add_reads([ref], i)
    tax = col.taxonomy(parent, ct)
    bits = col.download()[0]
    labels = tax.labels()
    assert labels.tobytes() == labels_of(bits, 6, parent, ct).tobytes()
    assert all((labels == t).any() for t in (0, 1, 2, 3, 8)) and (labels == NONE).any()   # strain-specific, genus-wide, root-wide and uncoloured unitigs
    reads, origin = [], []
    for i, ref in enumerate(refs):
        for _ in range(150):
            a = int(rng.integers(0, len(ref) - 150))
            reads.append(ref[a: a + int(rng.integers(60, 150))]); origin.append(i)
    seen = set()
    for rule in ((1, 0), (1, 500), (200, 0)):
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        got = b.taxa(tax, *rule)
        recs, stream = b.records()
        assert_taxa(got, fa.records_read_taxa(recs, stream, k, labels, parent, *rule), "the twin from the downloaded records, rule %s" % (rule,))
        for r, i in enumerate(origin):
            t = int(got["taxon"][r])
            assert t == NONE or t in path_of(parent, ct[i]), "read %d of reference %d is called %d" % (r, i, t)
            seen.add(t)
        direct, clade, unclassified = tax.reset().add(b, *rule).download()
        assert int(clade[0]) + unclassified == len(reads) and direct.sum() == (got["taxon"] != NONE).sum()
        b.close()
    assert {0, 1, 2, 3, 8, NONE} <= seen   # strains where the read is specific, genera and the root where it is not
    tax.close(); col.close(); p.close()
