"""`finito search-fmin --label-unitigs FASTA --labels FILE --classify FILE --label-report FILE`: the files are compared with the lines made from the definition
in numpy (tests/test_read_class_host.py::classes_of, ::tally_of) over the ORACLE's pairs; two query files, so the read numbers run on."""
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import OracleIndex
from tests.test_read_class import numbers_of
from tests.test_read_class_host import NONE, classes_of, tally_of
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


def test_cli_classify_and_label_report(tmp_path):
    k = 31
    rng = np.random.default_rng(1698)
    g = random_genome(rng, 30000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    # the labelling in the FASTA's order: five labels by position in the file, every ninth unitig without one; in the index's numbers for the expectation
    given = np.array([NONE if i % 9 == 4 else i * 5 // len(unitigs) for i in range(len(unitigs))], dtype=np.int64)
    (tmp_path / "l.txt").write_text("".join("-\n" if x == NONE else "%d\n" % x for x in given))
    labels = np.zeros(len(unitigs), dtype=np.int64)
    labels[numbers_of(unitigs, k)] = given
    reads = sample_reads(rng, g, 1500, 150, err=0.01, random_frac=0.1) + [mosaic_read(rng, g, k, 300) for _ in range(200)] + ["ACGT", "ACGTACGTAC"]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    cut = 2 * len(reads) // 3 + 1
    write_fastq(tmp_path / "q1.fq", reads[:cut]); write_fastq(tmp_path / "q2.fq", reads[cut:])
    (tmp_path / "q.txt").write_text("%s\n%s\n" % (tmp_path / "q1.fq", tmp_path / "q2.fq"))
    r = run("build-fmin", "-o", str(tmp_path / "idx"), "-u", str(tmp_path / "u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    o = OracleIndex.build(unitigs, k)
    pairs = oracle_pairs(o, reads)
    nks = nks_of(reads, k)
    want = classes_of(pairs, nks, labels)
    want_lines = "".join("%d\t%d\t%s\t%d\t%d\t%d\n" % (i, nks[i], "-" if c["label"] == NONE else "%d" % c["label"], c["n_best"], c["n_second"], c["n_labelled"])
                         for i, c in enumerate(want))
    report = lambda *rule: "".join("%d\t%d\n" % (l, n) for l, n in enumerate(tally_of(want, nks, 5, *rule)[:-1])) + "unassigned\t%d\n" % tally_of(want, nks, 5, *rule)[-1]
    assert (want["label"] == NONE).sum() > 50 and (want["n_second"] > 0).sum() > 50 and (nks == 0).any() and report(1, 0, 0) != report(20, 900, 3)
    assert all(n > 0 for n in tally_of(want, nks, 5, 20, 900, 3))

    def plain_text(tag):
        return open(tmp_path / (tag + "1.txt"), "rb").read() + open(tmp_path / (tag + "2.txt"), "rb").read()

    def outs(tag):
        (tmp_path / (tag + ".txt")).write_text("%s\n%s\n" % (tmp_path / (tag + "1.txt"), tmp_path / (tag + "2.txt")))
        return str(tmp_path / (tag + ".txt"))

    common = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.txt"), "--gpus", "1")
    lab = ("--label-unitigs", str(tmp_path / "u.fna"), "--labels", str(tmp_path / "l.txt"))
    r0 = run(*common, "-o", outs("plain"))
    assert r0.returncode == 0, r0.stderr
    assert len(plain_text("plain")) > 10 * len(reads)
    # beside -o: the text is byte for byte the plain run's
    r1 = run(*common, *lab, "-o", outs("both"), "--classify", str(tmp_path / "c1.tsv"), "--label-report", str(tmp_path / "t1.tsv"))
    assert r1.returncode == 0, r1.stderr
    assert open(tmp_path / "c1.tsv").read() == want_lines and open(tmp_path / "t1.tsv").read() == report(1, 0, 0)
    assert plain_text("both") == plain_text("plain")
    # each alone with --no-text 1: nothing on stdout, the log's count is the plain run's
    total = lambda r: [ln.split()[-1] for ln in r.stderr.splitlines() if "Total found kmers" in ln]
    r2 = run(*common, *lab, "--classify", str(tmp_path / "c2.tsv"), "--no-text", "1")
    assert r2.returncode == 0 and r2.stdout == "", r2.stderr
    assert open(tmp_path / "c2.tsv").read() == want_lines and total(r2) == total(r0)
    r3 = run(*common, *lab, "--label-report", str(tmp_path / "t3.tsv"), "--class-min-found", "20", "--class-min-permille", "900", "--class-min-margin", "3", "--no-text", "1")
    assert r3.returncode == 0 and r3.stdout == "", r3.stderr
    assert open(tmp_path / "t3.tsv").read() == report(20, 900, 3) and total(r3) == total(r0)
    # together with --read-summary (and its own thresholds stay the screen's)
    r4 = run(*common, *lab, "-o", outs("all"), "--classify", str(tmp_path / "c4.tsv"), "--label-report", str(tmp_path / "t4.tsv"), "--class-min-margin", "1",
             "--read-summary", str(tmp_path / "s4.tsv"), "--screen", str(tmp_path / "p4.txt"), "--min-found", "20")
    assert r4.returncode == 0, r4.stderr
    assert open(tmp_path / "c4.tsv").read() == want_lines and open(tmp_path / "t4.tsv").read() == report(1, 0, 1) and plain_text("all") == plain_text("plain")
    rows = np.loadtxt(tmp_path / "s4.tsv", dtype=np.int64, delimiter="\t", ndmin=2)
    found = np.array([int((pairs[a:b, 0] != -1).sum()) for a, b in zip(np.cumsum(nks) - nks, np.cumsum(nks))])
    assert np.array_equal(rows[:, 1], nks) and np.array_equal(rows[:, 2], found) and (want["n_labelled"] <= found).all()
    # a labels file whose line count is not the FASTA's, and a token that is no label: the error names the line
    lines = (tmp_path / "l.txt").read_text().splitlines()
    for text, word in (("\n".join(lines[:-1]) + "\n", "line %d" % (len(lines) - 1)), ("\n".join(lines + ["3"]) + "\n", "line %d" % (len(lines) + 1)),
                       ("\n".join(lines[:7] + ["x7"] + lines[8:]) + "\n", "line 8"), ("\n".join(lines[:2] + ["-1"] + lines[3:]) + "\n", "line 3")):
        (tmp_path / "bad.txt").write_text(text)
        r = run(*common, "--label-unitigs", str(tmp_path / "u.fna"), "--labels", str(tmp_path / "bad.txt"), "--classify", str(tmp_path / "x.tsv"), "--no-text", "1")
        assert r.returncode == 1 and word in r.stderr and "bad.txt" in r.stderr, r.stderr
    # a FASTA record that is no unitig of the index
    with open(tmp_path / "v.fna", "w") as f:
        f.write(">0\n%s\n" % unitigs[0][3:])
    (tmp_path / "one.txt").write_text("0\n")
    r = run(*common, "--label-unitigs", str(tmp_path / "v.fna"), "--labels", str(tmp_path / "one.txt"), "--classify", str(tmp_path / "x.tsv"), "--no-text", "1")
    assert r.returncode == 1 and "sequence 0" in r.stderr, r.stderr
    # refused for a partitioned index
    r = run("build-fmin", "-o", str(tmp_path / "parts"), "-u", str(tmp_path / "u.fna"), "-k", str(k), "--parts-max-bases", "12000")
    assert r.returncode == 0 and os.path.exists(tmp_path / "parts.finparts"), r.stderr
    for flag in ("--classify", "--label-report"):
        r = run("search-fmin", "-i", str(tmp_path / "parts"), "-q", str(tmp_path / "q1.fq"), "--gpus", "1", *lab, flag, str(tmp_path / "x.tsv"), "--no-text", "1")
        assert r.returncode == 1 and flag + " is not available with a partitioned index" in r.stderr, r.stderr
