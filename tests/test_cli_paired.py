"""`finito search-fmin --paired 1 --color-refs LIST --pseudoalign FILE --eqclasses FILE --color-report FILE --abundance FILE [--pair-both 1]`: the interleaved
command end to end on a tiny set.  Its files are compared with the Python API's results over the same reads and the same colours (FinimizerIndex.pseudoalign_pairs,
EqClasses.add_read_pairs) -- themselves checked against the numpy definition in tests/test_paired.py, and once more here --; a file with an odd number of
records is refused by name."""
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.test_colors_host import colors_of, pack_members
from tests.test_paired_host import assert_frags, frags_of
from tests.test_segments import nks_of, oracle_pairs
from tests.util import cut_unitigs, mosaic_read, random_genome, rc, sample_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def run(*a):
    return subprocess.run([BIN, *a], capture_output=True, text=True, timeout=300)


def test_cli_paired(tmp_path):
    k, n_colors = 31, 5
    rng = np.random.default_rng(2598)
    g = random_genome(rng, 30000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    step = len(g) // (n_colors + 2)
    refs = [g[i * step: (i + 2) * step] for i in range(n_colors)]   # overlapping stretches; the genome's end is in none
    for i, s in enumerate(refs):
        with open(tmp_path / ("ref%d.fna" % i), "w") as f:
            f.write(">c\n%s\n" % s)
    (tmp_path / "refs.txt").write_text("".join("%s\n" % (tmp_path / ("ref%d.fna" % i)) for i in range(n_colors)))
    # fragments: both mates from one place 100 bases apart, the second reverse-complemented; mates from two places; a mosaic, a read from nowhere, a mate shorter than k
    reads = []
    for _ in range(150):
        a = int(rng.integers(0, len(g) - 400))
        reads += [sample_reads(rng, g[a:a + 150], 1, 150, err=0.01, random_frac=0.0)[0], rc(g[a + 250:a + 400])]
    for _ in range(40):
        a, b = (int(x) for x in rng.integers(0, len(g) - 150, 2))
        reads += [g[a:a + 150], g[b:b + 120]]
    for _ in range(20):
        a = int(rng.integers(0, len(g) - 150))
        reads += [mosaic_read(rng, g, k, 300), g[a:a + 150], random_genome(rng, 150), g[a:a + 150], g[a:a + 150], "ACGTACGTAC"]
    assert len(reads) % 2 == 0 and all(reads)
    with open(tmp_path / "q.fq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@f%d/%d\n%s\n+\n%s\n" % (i // 2, i % 2 + 1, r, "I" * len(r)))
    with open(tmp_path / "odd.fq", "w") as f:
        for i, r in enumerate(reads[:-1]):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    r = run("build-fmin", "-o", str(tmp_path / "idx"), "-u", str(tmp_path / "u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    # the Python API over the same index, the same colouring by search and the same reads
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    col = p.colors(n_colors)
    for i, s in enumerate(refs):
        col.add_reads([s], i)
    o = OracleIndex.build(unitigs, k)
    member = np.zeros((len(unitigs), n_colors), dtype=np.uint8)
    for i, s in enumerate(refs):
        e = oracle_pairs(o, [s])
        member[np.unique(e[e[:, 0] >= 0, 0]), i] = 1
    bits = pack_members(member)
    assert np.array_equal(col.download()[0], bits)
    pairs, nks = oracle_pairs(o, reads), nks_of(reads, k)
    kmers = nks[0::2] + nks[1::2]
    sets = lambda row: ",".join("%d" % c for c in colors_of(row, n_colors)) or "-"
    common = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq"), "--gpus", "1", "--color-refs", str(tmp_path / "refs.txt"), "--paired", "1")
    for pm, both in ((1000, False), (300, False), (1000, True)):
        tag = "%d%s" % (pm, "b" if both else "")
        rows, heads, _ = p.pseudoalign_pairs(reads, col, pm, both)
        assert_frags((rows, heads), frags_of(pairs, nks, bits, n_colors, pm, both), "the Python API, permille %d, both %s" % (pm, both))
        eq = col.eqclasses(1024).add_read_pairs(reads, pm, both)
        crows, creads, un = eq.download()
        with_c, only_c, _ = eq.tally()
        ab = eq.abundance()
        eq.close()
        args = ["--pseudoalign", str(tmp_path / ("p%s.tsv" % tag)), "--eqclasses", str(tmp_path / ("e%s.tsv" % tag)), "--color-report", str(tmp_path / ("c%s.tsv" % tag)),
                "--abundance", str(tmp_path / ("a%s.tsv" % tag)), "--pseudo-permille", str(pm), "--no-text", "1"] + (["--pair-both", "1"] if both else [])
        r1 = run(*common, *args)
        assert r1.returncode == 0 and r1.stdout == "", r1.stderr
        want = "".join("%d\t%d\t%d\t%d\t%d\t%s\n" % (f, kmers[f], heads["n_found"][f], heads["n_colored"][f], heads["n_colored_first"][f], sets(rows[f])) for f in range(len(rows)))
        assert open(tmp_path / ("p%s.tsv" % tag)).read() == want, tag
        want = "".join("%d\t%d\t%s\n" % (creads[i], len(colors_of(crows[i], n_colors)), sets(crows[i])) for i in range(len(crows)))
        assert open(tmp_path / ("e%s.tsv" % tag)).read() == want and len(crows) >= 3, tag
        want = "".join("%d\t%d\t%d\n" % (c, with_c[c], only_c[c]) for c in range(n_colors)) + "unaligned\t%d\n" % un
        assert open(tmp_path / ("c%s.tsv" % tag)).read() == want and int(creads.sum()) + un == len(reads) // 2, tag   # fragments are what is counted
        lines = open(tmp_path / ("a%s.tsv" % tag)).read().splitlines()
        got_alpha = np.array([float(ln.split("\t")[1]) for ln in lines[:n_colors]])
        assert np.allclose(got_alpha, ab.alpha, rtol=1e-9, atol=1e-9) and lines[n_colors] == "unaligned\t%d" % un, tag   # (%.10g in the file)
    assert open(tmp_path / "p1000.tsv").read() != open(tmp_path / "p1000b.tsv").read() != open(tmp_path / "p300.tsv").read()
    # with the pair text: the text is per read, as without --paired
    r2 = run(*common, "-o", str(tmp_path / "out.txt"), "--pseudoalign", str(tmp_path / "p2.tsv"))
    r3 = run(*common[:-2], "-o", str(tmp_path / "out3.txt"), "--pseudoalign", str(tmp_path / "p3.tsv"))
    assert r2.returncode == 0 and r3.returncode == 0, r2.stderr + r3.stderr
    assert open(tmp_path / "out.txt").read() == open(tmp_path / "out3.txt").read() and open(tmp_path / "p2.tsv").read() == open(tmp_path / "p1000.tsv").read()
    assert len(open(tmp_path / "p3.tsv").read().splitlines()) == len(reads)
    # an odd file is refused, and named
    odd = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "odd.fq"), "--gpus", "1", "--color-refs", str(tmp_path / "refs.txt"), "--paired", "1")
    r4 = run(*odd, "--eqclasses", str(tmp_path / "e4.tsv"), "--no-text", "1")
    assert r4.returncode == 1 and "odd.fq" in r4.stderr and "odd number" in r4.stderr, r4.stderr
    # usage: --paired 1 wants colours, --pair-both wants --paired; both before any search (the index does not exist)
    r5 = run("search-fmin", "-i", str(tmp_path / "none"), "-q", str(tmp_path / "q.fq"), "--paired", "1")
    assert r5.returncode == 1 and "--color-refs" in r5.stderr and "--paired" in r5.stderr and not r5.stdout
    r6 = run("search-fmin", "-i", str(tmp_path / "none"), "-q", str(tmp_path / "q.fq"), "--color-refs", str(tmp_path / "refs.txt"), "--eqclasses", str(tmp_path / "e6.tsv"), "--pair-both", "1")
    assert r6.returncode == 1 and "--pair-both" in r6.stderr and "--paired" in r6.stderr
    r7 = run("search-fmin", "--help")
    assert "--paired" in r7.stderr and "--pair-both" in r7.stderr
    col.close(); p.close()
