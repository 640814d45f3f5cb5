"""`finito search-fmin --color-refs LIST --taxonomy FILE --color-taxa FILE --taxa FILE --taxon-report FILE`: every refusal, each before the index is loaded and
naming the line it is about (no GPU), and both output files equal, byte for byte, to what the Python route gives on the same index, references and reads
(Colors.taxonomy, Batch.taxa and Taxonomy.download, themselves held against twin and model in tests/test_taxa_*.py), in the caller's taxon ids."""
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from tests.util import cut_unitigs, random_genome, sample_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")

# NCBI-like ids, children before their parents, an empty line: 1 the root; 10, 20 below it; 101, 102 below 10; 201 below 20
TAXONOMY = "101\t10\n10\t1\n\n1\t1\n102\t10\n20\t1\n201\t20\n"
COLOR_TAXA = ["101", "102", "201", "101", "20"]


def run(*a):
    return subprocess.run([BIN, *a], capture_output=True, text=True, timeout=300)


def test_refusals_name_the_line(tmp_path):
    P = lambda name: str(tmp_path / name)
    (tmp_path / "refs.txt").write_text("".join("ref%d.fna\n" % i for i in range(5)))
    (tmp_path / "tax.tsv").write_text(TAXONOMY)
    (tmp_path / "ct.tsv").write_text("".join(t + "\n" for t in COLOR_TAXA))
    common = ("search-fmin", "-i", P("idx"), "-q", P("q.fq"), "--no-text", "1", "--color-refs", P("refs.txt"))
    def refused(tax, ct, *words, extra=("--taxa",)):
        (tmp_path / "t.tsv").write_text(tax)
        (tmp_path / "c.tsv").write_text(ct)
        r = run(*common, "--taxonomy", P("t.tsv"), "--color-taxa", P("c.tsv"), *[x for e in extra for x in (e, P("out_" + e.strip("-")))])
        assert r.returncode == 1 and "Loading index" not in r.stderr, r.stderr
        for w in words:
            assert w in r.stderr, (w, r.stderr)
        assert not os.path.exists(P("out_taxa")) and not os.path.exists(P("out_taxon-report"))
    good_ct = "".join(t + "\n" for t in COLOR_TAXA)
    refused("1\t1\n2\t3\n3\t2\n", "1\n" * 5, "line 2", "cycle", "taxon 2")
    refused("1\t1\n2\t1\n3\t7\n", "1\n" * 5, "line 3", "unknown parent 7")
    refused("1\t1\n2\t1\n\n3\t3\n", "1\n" * 5, "line 4", "second root", "line 1")
    refused("1\t2\n2\t1\n", "1\n" * 5, "no root")
    refused("1\t1\n2\t1\n2\t1\n", "1\n" * 5, "line 3", "line 2 already")
    refused("1\t1\n2 1\n", "1\n" * 5, "line 2", "id<TAB>parent_id")
    refused("1\t1\nx\t1\n", "1\n" * 5, "line 2", "id<TAB>parent_id")
    refused("", "1\n" * 5, "is empty")
    refused(TAXONOMY, "".join(t + "\n" for t in COLOR_TAXA[:4]), "has 4 taxa", "names 5 references")
    refused(TAXONOMY, good_ct + "20\n", "line 6", "5 references")
    refused(TAXONOMY, "101\n102\n\n999\n101\n20\n", "line 4", "taxon 999 is not in the file of --taxonomy")
    refused(TAXONOMY, "101\n10 2\n201\n101\n20\n", "line 2", "one taxon id")
    refused("1\t1\n2\t3\n3\t2\n", "1\n" * 5, "line 2", "cycle", extra=("--taxon-report",))
    # the usage rules
    for flags, word in ((("--taxa", P("o")), "--taxa and --taxon-report want a taxonomy over colours"),
                        (("--taxa", P("o"), "--taxonomy", P("tax.tsv")), "--taxa and --taxon-report want a taxonomy over colours"),
                        (("--taxonomy", P("tax.tsv"), "--color-taxa", P("ct.tsv"), "--pseudoalign", P("o")), "--taxonomy is only legal together with --taxa or --taxon-report"),
                        (("--taxa-confidence", "5", "--pseudoalign", P("o")), "--taxa-confidence is only legal together with --taxa or --taxon-report"),
                        (("--taxa-min-found", "5", "--pseudoalign", P("o")), "--taxa-min-found is only legal together with --taxa or --taxon-report"),
                        (("--taxa", P("o"), "--taxonomy", P("tax.tsv"), "--color-taxa", P("ct.tsv"), "--taxa-confidence", "1001"), "--taxa-confidence wants a number from 0 to 1000"),
                        (("--taxa", P("o"), "--taxonomy", P("tax.tsv"), "--color-taxa", P("ct.tsv"), "--paired", "1"), "not together with --paired 1")):
        r = run(*common, *flags)
        assert r.returncode == 1 and word in r.stderr and "Loading index" not in r.stderr, (flags, r.stderr)
    r = run("search-fmin", "-i", P("idx"), "-q", P("q.fq"), "--no-text", "1", "--taxa", P("o"), "--taxonomy", P("tax.tsv"), "--color-taxa", P("ct.tsv"))   # no --color-refs
    assert r.returncode == 1 and "--taxa and --taxon-report want a taxonomy over colours" in r.stderr
    assert not os.path.exists(P("o"))


@pytest.mark.gpu
def test_cli_taxa_files_equal_the_python_route(tmp_path):
    k = 31
    rng = np.random.default_rng(5200)
    shared, genus, priv, nobody = random_genome(rng, 3000), random_genome(rng, 3000), [random_genome(rng, 2500) for _ in range(3)], random_genome(rng, 1500)
    unitigs = []
    for piece in [shared, genus] + priv + [nobody]:
        unitigs += cut_unitigs(rng, piece, k, max_len=300)
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    # references 0 and 1 (taxa 101, 102 of genus 10) share `genus` and `shared`; 2 (taxon 201) shares `shared`; 3 is 0 again; 4 sits on the inner taxon 20
    refs = [[shared, genus, priv[0]], [shared, genus, priv[1]], [shared, priv[2]], [shared, genus, priv[0]], [nobody]]
    for i, r in enumerate(refs):
        with open(tmp_path / ("ref%d.fna" % i), "w") as f:
            f.write("".join(">s%d\n%s\n" % (j, s) for j, s in enumerate(r)))
    P = lambda name: str(tmp_path / name)
    (tmp_path / "refs.txt").write_text("".join("%s\n" % P("ref%d.fna" % i) for i in range(len(refs))))
    (tmp_path / "tax.tsv").write_text(TAXONOMY)
    (tmp_path / "ct.tsv").write_text("".join(t + "\n" for t in COLOR_TAXA))
    reads = (sample_reads(rng, shared + genus + priv[0], 300, 100, err=0.0, random_frac=0.05) + sample_reads(rng, priv[1], 40, 100, err=0.01, random_frac=0.0) +
             sample_reads(rng, priv[2] + nobody, 60, 100, err=0.0, random_frac=0.0))
    with open(tmp_path / "q.fq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    r = run("build-fmin", "-o", P("idx"), "-u", P("u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    # the Python route over the index the tool wrote
    ids, pids = [101, 10, 1, 102, 20, 201], [10, 1, 1, 10, 1, 20]
    order, parent = fa.taxonomy_order(ids, pids)
    name = {int(order[i]): ids[i] for i in range(len(ids))}
    ct = np.array([order[ids.index(int(t))] for t in COLOR_TAXA], dtype=np.uint32)
    p = fa.FinimizerIndex().load(P("idx")).to_device(0)
    col = p.colors(len(refs))
    for c, ref in enumerate(refs):
        col.add_reads(ref, c)
    tax = col.taxonomy(parent, ct)
    want = {}
    for rule in ((1, 0), (20, 600)):
        got = p.taxa_reads(reads, tax, *rule)
        nks = [max(len(r) - k + 1, 0) for r in reads]
        lines = "".join("%d\t%d\t%s\t%d\t%d\t%d\n" % (i, nks[i], "-" if t["taxon"] == fa.FIN_NO_LABEL else name[int(t["taxon"])], t["score"], t["clade"], t["n_labelled"])
                        for i, t in enumerate(got))
        direct, clade, unclassified = tax.reset().add_reads(reads, *rule).download()
        by_number = sorted(name)   # the report goes through the taxa in the tool's numbering: the root, then breadth-first in file order
        report = "".join("%d\t%d\t%d\n" % (name[t], clade[t], direct[t]) for t in by_number if clade[t]) + "unclassified\t%d\n" % unclassified
        want[rule] = (lines, report)
        assert int(clade[0]) + unclassified == len(reads)
    called = {l.split("\t")[2] for l in want[(1, 0)][0].splitlines()}
    assert {"101", "102", "10", "1", "201", "20", "-"} <= called and want[(1, 0)] != want[(20, 600)]
    tax.close(); col.close(); p.close()
    common = ("search-fmin", "-i", P("idx"), "-q", P("q.fq"), "--gpus", "1", "--color-refs", P("refs.txt"), "--taxonomy", P("tax.tsv"), "--color-taxa", P("ct.tsv"))
    r1 = run(*common, "--no-text", "1", "--taxa", P("t1.tsv"), "--taxon-report", P("r1.tsv"))
    assert r1.returncode == 0, r1.stderr
    assert open(P("t1.tsv")).read() == want[(1, 0)][0] and open(P("r1.tsv")).read() == want[(1, 0)][1]
    r2 = run(*common, "-o", P("out.txt"), "--taxa", P("t2.tsv"), "--taxon-report", P("r2.tsv"), "--taxa-confidence", "600", "--taxa-min-found", "20", "--pseudoalign", P("psa.tsv"))
    assert r2.returncode == 0, r2.stderr
    assert open(P("t2.tsv")).read() == want[(20, 600)][0] and open(P("r2.tsv")).read() == want[(20, 600)][1] and os.path.getsize(P("out.txt")) > 0
    r3 = run(*common, "--no-text", "1", "--taxon-report", P("r3.tsv"))   # the report alone
    assert r3.returncode == 0, r3.stderr
    assert open(P("r3.tsv")).read() == want[(1, 0)][1] and not os.path.exists(P("t3.tsv"))
