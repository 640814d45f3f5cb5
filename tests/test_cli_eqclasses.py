"""`finito search-fmin --color-refs LIST --eqclasses FILE --color-report FILE [--pseudo-permille P] [--no-text 1]`: both files are compared with the files
rendered from the definition in numpy (tests/test_eqclasses_host.py::classes_of_rows over tests/test_colors_host.py::rows_of) over the ORACLE's pairs, the colours
with the brute-force matrix; the rows of --pseudoalign in the same run regroup to the same classes."""
import collections
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import OracleIndex
from tests.test_colors_host import colors_of, pack_members, rows_of
from tests.test_eqclasses_host import classes_of_rows, tally_of
from tests.test_segments import nks_of, oracle_pairs
from tests.util import cut_unitigs, mosaic_read, random_genome, sample_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def run(*a):
    return subprocess.run([BIN, *a], capture_output=True, text=True, timeout=300)


def test_cli_eqclasses_and_color_report(tmp_path):
    k, n_colors = 31, 5
    rng = np.random.default_rng(2298)
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
    reads = sample_reads(rng, g, 400, 150, err=0.01, random_frac=0.1) + [mosaic_read(rng, g, k, 300) for _ in range(80)] + ["ACGT", "ACGTACGTAC"]
    reads = [reads[i] for i in rng.permutation(len(reads)) if reads[i]]
    with open(tmp_path / "q.fq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    r = run("build-fmin", "-o", str(tmp_path / "idx"), "-u", str(tmp_path / "u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    o = OracleIndex.build(unitigs, k)
    member = np.zeros((len(unitigs), n_colors), dtype=np.uint8)
    for i, s in enumerate(refs):
        e = oracle_pairs(o, [s])
        member[np.unique(e[e[:, 0] >= 0, 0]), i] = 1
    bits = pack_members(member)
    pairs, nks = oracle_pairs(o, reads), nks_of(reads, k)

    def want_files(permille):
        rows, reads_of, un = classes_of_rows(rows_of(pairs, nks, bits, n_colors, permille)[0], n_colors)
        eqc = "".join("%d\t%d\t%s\n" % (reads_of[i], len(colors_of(rows[i], n_colors)), ",".join("%d" % c for c in colors_of(rows[i], n_colors)))
                      for i in range(len(rows)))
        w, only = tally_of(rows, reads_of, n_colors)
        rep = "".join("%d\t%d\t%d\n" % (c, w[c], only[c]) for c in range(n_colors)) + "unaligned\t%d\n" % un
        return eqc, rep

    assert want_files(0) != want_files(1000) and "\t2\t" in want_files(1000)[0] and not want_files(1000)[1].endswith("unaligned\t0\n")
    common = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq"), "--gpus", "1", "--color-refs", str(tmp_path / "refs.txt"))
    for pm in (1000, 0):
        tag = str(pm)
        r1 = run(*common, "-o", str(tmp_path / ("out%s.txt" % tag)), "--eqclasses", str(tmp_path / ("e%s.tsv" % tag)), "--color-report", str(tmp_path / ("c%s.tsv" % tag)),
                 "--pseudoalign", str(tmp_path / ("p%s.tsv" % tag)), "--pseudo-permille", tag)
        assert r1.returncode == 0, r1.stderr
        eqc, rep = want_files(pm)
        assert open(tmp_path / ("e%s.tsv" % tag)).read() == eqc, "permille %d" % pm
        assert open(tmp_path / ("c%s.tsv" % tag)).read() == rep, "permille %d" % pm
        # the rows of --pseudoalign in the same run regroup to the same classes
        sets = [ln.split("\t")[4] for ln in open(tmp_path / ("p%s.tsv" % tag)).read().splitlines()]
        assert len(sets) == len(reads)
        grouped = collections.Counter(s for s in sets if s != "-")
        assert grouped == collections.Counter({ln.split("\t")[2]: int(ln.split("\t")[0]) for ln in eqc.splitlines()})
        assert sets.count("-") == int(rep.splitlines()[-1].split("\t")[1])
    # either option alone with --no-text 1: nothing on stdout
    eqc, rep = want_files(1000)
    r2 = run(*common, "--eqclasses", str(tmp_path / "e2.tsv"), "--no-text", "1")
    assert r2.returncode == 0 and r2.stdout == "", r2.stderr
    assert open(tmp_path / "e2.tsv").read() == eqc
    r3 = run(*common, "--color-report", str(tmp_path / "c3.tsv"), "--no-text", "1", "--eq-max-classes", "64")
    assert r3.returncode == 0 and r3.stdout == "", r3.stderr
    assert open(tmp_path / "c3.tsv").read() == rep
    # too little room is an error, not a truncated file
    r4 = run(*common, "--eqclasses", str(tmp_path / "e4.tsv"), "--no-text", "1", "--eq-max-classes", "2")
    assert r4.returncode == 1 and "max_classes" in r4.stderr, r4.stderr
