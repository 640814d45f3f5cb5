"""`finito search-fmin --read-summary FILE` and `--screen FILE`: the files are parsed back and compared with the definition in numpy
(tests/test_read_summary_host.py::summaries_of, ::rule) over the ORACLE's pairs; two query files, so the read numbers run on."""
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.test_read_summary_host import rule, summaries_of
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


def test_cli_read_summary_and_screen(tmp_path):
    k = 31
    rng = np.random.default_rng(1498)
    g = random_genome(rng, 30000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    reads = sample_reads(rng, g, 1500, 150, err=0.01, random_frac=0.1) + [mosaic_read(rng, g, k, 300) for _ in range(200)]
    reads = [r for r in reads if len(r) >= k]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    cut = 2 * len(reads) // 3 + 1
    write_fastq(tmp_path / "q1.fq", reads[:cut]); write_fastq(tmp_path / "q2.fq", reads[cut:])
    (tmp_path / "q.txt").write_text("%s\n%s\n" % (tmp_path / "q1.fq", tmp_path / "q2.fq"))
    r = run("build-fmin", "-o", str(tmp_path / "idx"), "-u", str(tmp_path / "u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    o = OracleIndex.build(unitigs, k)
    pairs = oracle_pairs(o, reads)
    nks = nks_of(reads, k)
    want = summaries_of(pairs, nks)
    found = int((pairs[:, 0] != -1).sum())
    want_lines = "".join("%d\t%d\t%d\t%d\t%d\t%d\n" % (i, nks[i], s["n_found"], s["n_segments"], s["longest"], s["span"]) for i, s in enumerate(want))
    ids_of = lambda *scr: "".join("%d\n" % i for i in np.nonzero(rule(want, nks, *scr))[0])
    assert (want["n_found"] == 0).sum() > 50 and (want["n_segments"] >= 3).sum() > 50 and 0 < rule(want, nks, 20, 900, 0).sum() < len(reads) - 100

    def parsed(path):
        rows = np.loadtxt(path, dtype=np.int64, delimiter="\t", ndmin=2)
        assert np.array_equal(rows[:, 0], np.arange(len(reads))) and np.array_equal(rows[:, 1], nks)   # the read numbers run on through the second file
        out = np.zeros(len(rows), dtype=fa.READ_SUMMARY_DTYPE)
        out["n_found"], out["n_segments"], out["longest"], out["span"] = rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5]
        return out

    def plain_text(tag):
        return open(tmp_path / (tag + "1.txt"), "rb").read() + open(tmp_path / (tag + "2.txt"), "rb").read()

    def outs(tag):
        (tmp_path / (tag + ".txt")).write_text("%s\n%s\n" % (tmp_path / (tag + "1.txt"), tmp_path / (tag + "2.txt")))
        return str(tmp_path / (tag + ".txt"))

    common = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.txt"), "--gpus", "1")
    r0 = run(*common, "-o", outs("plain"))
    assert r0.returncode == 0, r0.stderr
    assert len(plain_text("plain")) > 10 * len(reads)
    # beside -o: the text is the plain run's
    r1 = run(*common, "-o", outs("both"), "--read-summary", str(tmp_path / "s1.tsv"), "--screen", str(tmp_path / "p1.txt"))
    assert r1.returncode == 0, r1.stderr
    assert open(tmp_path / "s1.tsv").read() == want_lines and np.array_equal(parsed(tmp_path / "s1.tsv"), want)
    assert open(tmp_path / "p1.txt").read() == ids_of(1, 0, 0)
    assert plain_text("both") == plain_text("plain")
    # each alone with --no-text 1: nothing on stdout, the log's count is the plain run's
    total = lambda r: [ln.split()[-1] for ln in r.stderr.splitlines() if "Total found kmers" in ln]
    r2 = run(*common, "--read-summary", str(tmp_path / "s2.tsv"), "--no-text", "1")
    assert r2.returncode == 0 and r2.stdout == "", r2.stderr
    assert open(tmp_path / "s2.tsv").read() == want_lines
    assert total(r2) == total(r0) and sum(int(x) for x in total(r2)) == found
    r3 = run(*common, "--screen", str(tmp_path / "p3.txt"), "--min-found", "20", "--min-permille", "900", "--no-text", "1")
    assert r3.returncode == 0 and r3.stdout == "", r3.stderr
    assert open(tmp_path / "p3.txt").read() == ids_of(20, 900, 0)
    assert total(r3) == total(r0)
    # --screen-invert 1 gives the complement
    r4 = run(*common, "--screen", str(tmp_path / "p4.txt"), "--min-found", "20", "--min-permille", "900", "--screen-invert", "1", "--no-text", "1")
    assert r4.returncode == 0, r4.stderr
    assert open(tmp_path / "p4.txt").read() == ids_of(20, 900, 1)
    kept = np.loadtxt(tmp_path / "p3.txt", dtype=np.int64, ndmin=1); dropped = np.loadtxt(tmp_path / "p4.txt", dtype=np.int64, ndmin=1)
    assert np.array_equal(np.sort(np.concatenate([kept, dropped])), np.arange(len(reads)))
    # with the other results
    r5 = run(*common, "-o", outs("all"), "--read-summary", str(tmp_path / "s5.tsv"), "--screen", str(tmp_path / "p5.txt"), "--segments", str(tmp_path / "g5.tsv"),
             "--unitig-counts", str(tmp_path / "n5.tsv"), "--unitig-coverage", str(tmp_path / "c5.tsv"), "--unitig-depth", str(tmp_path / "d5.tsv"))
    assert r5.returncode == 0, r5.stderr
    assert open(tmp_path / "s5.tsv").read() == want_lines and open(tmp_path / "p5.txt").read() == ids_of(1, 0, 0) and plain_text("all") == plain_text("plain")
    assert np.loadtxt(tmp_path / "n5.tsv", dtype=np.int64, ndmin=2)[:, 1].sum() == found
    seg_reads = np.loadtxt(tmp_path / "g5.tsv", dtype=str, delimiter="\t", ndmin=2)[:, 0].astype(np.int64)
    assert np.array_equal(np.bincount(seg_reads, minlength=len(reads)), want["n_segments"])
    # refused for a partitioned index
    r = run("build-fmin", "-o", str(tmp_path / "parts"), "-u", str(tmp_path / "u.fna"), "-k", str(k), "--parts-max-bases", "12000")
    assert r.returncode == 0 and os.path.exists(tmp_path / "parts.finparts"), r.stderr
    for flag in ("--read-summary", "--screen"):
        r = run("search-fmin", "-i", str(tmp_path / "parts"), "-q", str(tmp_path / "q1.fq"), "--gpus", "1", flag, str(tmp_path / "x.tsv"), "--no-text", "1")
        assert r.returncode == 1 and flag + " is not available with a partitioned index" in r.stderr, r.stderr
