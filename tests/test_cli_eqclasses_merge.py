"""`finito search-fmin ... --eqclasses-in LIST` and `--eqclasses-unaligned 1`: a FASTQ run in two parts, the second part taking the first part's classes file,
must write what a run over the whole file writes -- the classes file and the colour report byte for byte, the abundance file's integers exactly and its
per-colour reads at relative 1e-9 (tests/test_cli_abundance.py's tolerance: the %.10g print precision doubled; both runs do the same fixed number of
iterations).  Bad classes files are errors that name file and line."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_cli_abundance import parse_abundance
from tests.util import cut_unitigs, mosaic_read, random_genome, sample_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def run(*a):
    return subprocess.run([BIN, *a], capture_output=True, text=True, timeout=300)


def write_fastq(path, reads, first=0):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (first + i, r, "I" * len(r)))


def test_cli_a_run_in_two_parts(tmp_path):
    k, n_colors = 31, 5
    rng = np.random.default_rng(3700)
    g = random_genome(rng, 30000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    step = len(g) // (n_colors + 2)
    for i in range(n_colors):   # overlapping stretches; the genome's end is in none
        with open(tmp_path / ("ref%d.fna" % i), "w") as f:
            f.write(">c\n%s\n" % g[i * step: (i + 2) * step])
    (tmp_path / "refs.txt").write_text("".join("%s\n" % (tmp_path / ("ref%d.fna" % i)) for i in range(n_colors)))
    reads = sample_reads(rng, g, 400, 150, err=0.01, random_frac=0.1) + [mosaic_read(rng, g, k, 300) for _ in range(80)] + ["ACGT", "ACGTACGTAC"]
    reads = [reads[i] for i in rng.permutation(len(reads)) if reads[i]]
    cut = 197
    write_fastq(tmp_path / "q.fq", reads)
    write_fastq(tmp_path / "q1.fq", reads[:cut])
    write_fastq(tmp_path / "q2.fq", reads[cut:], first=cut)
    r = run("build-fmin", "-o", str(tmp_path / "idx"), "-u", str(tmp_path / "u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    P = lambda name: str(tmp_path / name)
    common = lambda q: ("search-fmin", "-i", P("idx"), "-q", P(q), "--gpus", "1", "--color-refs", P("refs.txt"), "--no-text", "1")
    ab = ("--ab-max-iters", "15", "--ab-tol", "0")
    whole = run(*common("q.fq"), "--eqclasses", P("whole.tsv"), "--color-report", P("whole_c.tsv"), "--abundance", P("whole_a.tsv"), *ab)
    assert whole.returncode == 0, whole.stderr
    # part 1, with the unaligned line; without the switch the file is today's: the same run's file less its last line
    p1 = run(*common("q1.fq"), "--eqclasses", P("p1.tsv"), "--eqclasses-unaligned", "1", "--color-report", P("p1_c.tsv"))
    assert p1.returncode == 0, p1.stderr
    p1_plain = run(*common("q1.fq"), "--eqclasses", P("p1_plain.tsv"))
    assert p1_plain.returncode == 0, p1_plain.stderr
    lines = open(P("p1.tsv")).read().splitlines(keepends=True)
    assert lines[-1] == open(P("p1_c.tsv")).read().splitlines(keepends=True)[-1] and lines[-1].startswith("unaligned\t") and int(lines[-1].split("\t")[1]) > 0
    assert "".join(lines[:-1]) == open(P("p1_plain.tsv")).read() and len(lines) > 3
    # part 2 on top of part 1
    (tmp_path / "list.txt").write_text(P("p1.tsv") + "\n")
    p2 = run(*common("q2.fq"), "--eqclasses-in", P("list.txt"), "--eqclasses", P("all.tsv"), "--color-report", P("all_c.tsv"), "--abundance", P("all_a.tsv"), *ab)
    assert p2.returncode == 0, p2.stderr
    assert open(P("all.tsv")).read() == open(P("whole.tsv")).read() and open(P("all.tsv")).read() != open(P("p1_plain.tsv")).read()
    assert open(P("all_c.tsv")).read() == open(P("whole_c.tsv")).read()
    got, want = parse_abundance(P("all_a.tsv"), n_colors), parse_abundance(P("whole_a.tsv"), n_colors)
    assert open(P("all_a.tsv")).read().splitlines()[n_colors] == open(P("whole_a.tsv")).read().splitlines()[n_colors]   # the `unaligned` line
    assert got[2] == want[2] and got[3] == want[3] == 15 and got[4] == want[4]
    assert (np.abs(got[0] - want[0]) <= 1e-9 * want[0]).all() and want[0].sum() > 100
    # the same file named twice counts twice, and --ab-bootstraps takes the merged classes
    (tmp_path / "twice.txt").write_text(P("p1.tsv") + "\n\n" + P("p1.tsv") + "\n")
    p3 = run(*common("q2.fq"), "--eqclasses-in", P("twice.txt"), "--color-report", P("twice_c.tsv"), "--abundance", P("twice_a.tsv"), "--ab-bootstraps", "2")
    assert p3.returncode == 0, p3.stderr
    un = lambda name: int(open(P(name)).read().splitlines()[-1].split("\t")[1])
    assert un("twice_c.tsv") == un("all_c.tsv") + un("p1_c.tsv")
    # bad classes files: the message names file and line
    good = open(P("p1_plain.tsv")).read().splitlines()
    for name, bad_line, word in (("colour.tsv", "3\t2\t1,%d" % n_colors, "colour %d" % n_colors), ("count.tsv", "3\t3\t1,2", "n_colours"), ("tabs.tsv", "3 2 1,2", "malformed"),
                                 ("number.tsv", "x\t2\t1,2", "malformed"), ("list.tsv", "3\t2\t1,,2", "malformed"), ("tail.tsv", "unaligned\t-4", "malformed")):
        (tmp_path / name).write_text("\n".join(good[:2] + [bad_line] + good[2:]) + "\n")
        (tmp_path / "bad.txt").write_text(P(name) + "\n")
        rb = run(*common("q2.fq"), "--eqclasses-in", P("bad.txt"), "--eqclasses", P("bad_out.tsv"))
        assert rb.returncode == 1 and P(name) in rb.stderr and "line 3" in rb.stderr and word in rb.stderr, (name, rb.stderr)
        assert not os.path.exists(P("bad_out.tsv"))
    (tmp_path / "bad.txt").write_text(P("nowhere.tsv") + "\n")
    rb = run(*common("q2.fq"), "--eqclasses-in", P("bad.txt"), "--eqclasses", P("bad_out.tsv"))
    assert rb.returncode == 1 and "nowhere.tsv" in rb.stderr
    # each new switch alone is refused
    bare = ("search-fmin", "-i", P("idx"), "-q", P("q2.fq"), "--gpus", "1")
    rb = run(*bare, "--eqclasses-in", P("list.txt"))
    assert rb.returncode == 1 and "--eqclasses-in is only legal together with" in rb.stderr
    rb = run(*bare, "--color-refs", P("refs.txt"), "--color-report", P("x.tsv"), "--eqclasses-unaligned", "1")
    assert rb.returncode == 1 and "--eqclasses-unaligned is only legal together with --eqclasses" in rb.stderr
    rb = run(*bare, "--eqclasses-unaligned", "1")
    assert rb.returncode == 1 and "--eqclasses-unaligned" in rb.stderr
    assert "--eqclasses-in LIST" in run("search-fmin", "--help").stderr and "--eqclasses-unaligned 1" in run("search-fmin", "--help").stderr
