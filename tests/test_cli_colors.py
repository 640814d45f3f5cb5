"""`finito search-fmin --color-refs LIST --colors-out FILE --pseudoalign FILE --pseudo-permille P`: the files are compared line by line with the lines made from
the definition in numpy (tests/test_colors_host.py::rows_of) over the ORACLE's pairs, the colours with the brute-force matrix (unitig u has colour i iff the oracle
finds a k-mer of reference i in u); two query files, so the read numbers run on."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import OracleIndex
from tests.test_colors_host import colors_of, pack_members, rows_of
from tests.test_segments import nks_of, oracle_pairs
from tests.util import cut_unitigs, mosaic_read, random_genome, sample_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def run(*a):
    return subprocess.run([BIN, *a], capture_output=True, text=True, timeout=300)


def write_fastq(path, reads):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))


def names(row, n_colors):
    return ",".join("%d" % c for c in colors_of(row, n_colors)) or "-"


def test_cli_color_refs_colors_out_and_pseudoalign(tmp_path):
    k = 31
    rng = np.random.default_rng(1998)
    g = random_genome(rng, 30000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    # three references: two overlapping stretches of 12 000 bases -- longer than a window of 4096 k-mers, so the cut into windows is exercised -- as one contig and
    # as two contigs with a line break inside, and a short one; the genome's end is in none
    refs = [[g[0:12000]], [g[8000:14000], g[13000:20000]], [g[19000:21000], "ACGT"]]
    for i, contigs in enumerate(refs):
        with open(tmp_path / ("ref%d.fna" % i), "w") as f:
            for j, s in enumerate(contigs):
                f.write(">c%d\n%s\n%s\n" % (j, s[: len(s) // 2], s[len(s) // 2:]))
    (tmp_path / "refs.txt").write_text("".join("%s\n" % (tmp_path / ("ref%d.fna" % i)) for i in range(3)))
    reads = sample_reads(rng, g, 1200, 150, err=0.01, random_frac=0.1) + [mosaic_read(rng, g, k, 300) for _ in range(200)] + ["ACGT", "ACGTACGTAC"]
    reads = [reads[i] for i in rng.permutation(len(reads)) if reads[i]]   # (a read without bases is no FASTQ record: the readers skip it)
    cut = 2 * len(reads) // 3 + 1
    write_fastq(tmp_path / "q1.fq", reads[:cut]); write_fastq(tmp_path / "q2.fq", reads[cut:])
    (tmp_path / "q.txt").write_text("%s\n%s\n" % (tmp_path / "q1.fq", tmp_path / "q2.fq"))
    r = run("build-fmin", "-o", str(tmp_path / "idx"), "-u", str(tmp_path / "u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    o = OracleIndex.build(unitigs, k)
    member = np.zeros((len(unitigs), 3), dtype=np.uint8)
    for i, contigs in enumerate(refs):
        e = oracle_pairs(o, contigs)
        member[np.unique(e[e[:, 0] >= 0, 0]), i] = 1
    bits = pack_members(member)
    per_unitig = member.sum(axis=1)
    assert (per_unitig == 0).any() and (per_unitig == 1).any() and (per_unitig == 2).any() and member.any(axis=0).all()
    want_colors = "".join("%d\t%s\n" % (u, names(bits[u], 3)) for u in range(len(unitigs)))
    pairs, nks = oracle_pairs(o, reads), nks_of(reads, k)

    def want_lines(permille):
        rows, heads = rows_of(pairs, nks, bits, 3, permille)
        return "".join("%d\t%d\t%d\t%d\t%s\n" % (i, nks[i], heads[i]["n_found"], heads[i]["n_colored"], names(rows[i], 3)) for i in range(len(reads)))

    assert len({want_lines(0), want_lines(500), want_lines(1000)}) == 3 and "\t0,1\n" in want_lines(1000) and "\t-\n" in want_lines(1000)

    def plain_text(tag):
        return open(tmp_path / (tag + "1.txt"), "rb").read() + open(tmp_path / (tag + "2.txt"), "rb").read()

    def outs(tag):
        (tmp_path / (tag + ".txt")).write_text("%s\n%s\n" % (tmp_path / (tag + "1.txt"), tmp_path / (tag + "2.txt")))
        return str(tmp_path / (tag + ".txt"))

    common = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.txt"), "--gpus", "1")
    col = ("--color-refs", str(tmp_path / "refs.txt"))
    r0 = run(*common, "-o", outs("plain"))
    assert r0.returncode == 0, r0.stderr
    assert len(plain_text("plain")) > 10 * len(reads)
    # beside -o: the text's md5 is the plain run's
    r1 = run(*common, *col, "-o", outs("both"), "--colors-out", str(tmp_path / "c1.tsv"), "--pseudoalign", str(tmp_path / "p1.tsv"))
    assert r1.returncode == 0, r1.stderr
    assert open(tmp_path / "c1.tsv").read().splitlines() == want_colors.splitlines()
    assert open(tmp_path / "p1.tsv").read().splitlines() == want_lines(1000).splitlines()
    assert hashlib.md5(plain_text("both")).hexdigest() == hashlib.md5(plain_text("plain")).hexdigest()
    # each alone with --no-text 1: nothing on stdout, the log's count is the plain run's
    total = lambda r: [ln.split()[-1] for ln in r.stderr.splitlines() if "Total found kmers" in ln]
    r2 = run(*common, *col, "--pseudoalign", str(tmp_path / "p2.tsv"), "--pseudo-permille", "500", "--no-text", "1")
    assert r2.returncode == 0 and r2.stdout == "", r2.stderr
    assert open(tmp_path / "p2.tsv").read() == want_lines(500) and total(r2) == total(r0)
    r3 = run(*common, *col, "--colors-out", str(tmp_path / "c3.tsv"), "--no-text", "1")
    assert r3.returncode == 0 and r3.stdout == "", r3.stderr
    assert open(tmp_path / "c3.tsv").read() == want_colors
    # the union, together with --read-summary
    r4 = run(*common, *col, "-o", outs("all"), "--pseudoalign", str(tmp_path / "p4.tsv"), "--pseudo-permille", "0", "--read-summary", str(tmp_path / "s4.tsv"))
    assert r4.returncode == 0, r4.stderr
    assert open(tmp_path / "p4.tsv").read() == want_lines(0) and plain_text("all") == plain_text("plain")
    rows = np.loadtxt(tmp_path / "s4.tsv", dtype=np.int64, delimiter="\t", ndmin=2)
    got = np.loadtxt(tmp_path / "p4.tsv", dtype=str, delimiter="\t", ndmin=2)
    assert np.array_equal(rows[:, 2], got[:, 2].astype(np.int64))   # `found` is --read-summary's
    # a reference file that is not there: refused before the search
    (tmp_path / "bad.txt").write_text("%s\n%s\n" % (tmp_path / "ref0.fna", tmp_path / "nowhere.fna"))
    r = run(*common, "--color-refs", str(tmp_path / "bad.txt"), "--pseudoalign", str(tmp_path / "x.tsv"), "--no-text", "1")
    assert r.returncode == 1 and "nowhere.fna" in r.stderr, r.stderr
    # refused for a partitioned index
    r = run("build-fmin", "-o", str(tmp_path / "parts"), "-u", str(tmp_path / "u.fna"), "-k", str(k), "--parts-max-bases", "12000")
    assert r.returncode == 0 and os.path.exists(tmp_path / "parts.finparts"), r.stderr
    r = run("search-fmin", "-i", str(tmp_path / "parts"), "-q", str(tmp_path / "q1.fq"), "--gpus", "1", *col, "--pseudoalign", str(tmp_path / "x.tsv"), "--no-text", "1")
    assert r.returncode == 1 and "--color-refs is not available with a partitioned index" in r.stderr, r.stderr
