"""`finito search-fmin --color-refs LIST --abundance FILE [--ab-lengths FILE] [--ab-max-iters N] [--ab-tol X]` beside --eqclasses: the abundance file is parsed
and compared with tests/test_abundance_host.py's numpy model over the classes of the --eqclasses file of the same run, at relative 1e-9 -- the %.10g print
precision, 5e-10, doubled.  The comparison run does a fixed number of iterations (--ab-tol 0), so that model and device have done the same ones; the stopping
lines are checked on a run with the defaults."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_abundance_host import Model
from tests.test_colors_host import pack
from tests.util import cut_unitigs, random_genome, sample_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def run(*a):
    return subprocess.run([BIN, *a], capture_output=True, text=True, timeout=300)


def parse_abundance(path, n_colors):
    lines = open(path).read().splitlines()
    assert len(lines) == n_colors + 3
    cols = [ln.split("\t") for ln in lines[:n_colors]]
    assert [int(c[0]) for c in cols] == list(range(n_colors)) and all(len(c) == 3 for c in cols)
    tail = [ln.split("\t") for ln in lines[n_colors:]]
    assert [t[0] for t in tail] == ["unaligned", "iterations", "loglik"] and len(tail[0]) == 2 and len(tail[1]) == 3 and len(tail[2]) == 2
    return np.array([float(c[1]) for c in cols]), np.array([float(c[2]) for c in cols]), int(tail[0][1]), int(tail[1][1]), tail[1][2], float(tail[2][1])


def test_cli_abundance(tmp_path):
    k, n_colors = 31, 4
    rng = np.random.default_rng(2520)
    shared, priv = random_genome(rng, 5000), [random_genome(rng, 2500) for _ in range(n_colors)]
    unitigs = []
    for piece in [shared] + priv:
        unitigs += cut_unitigs(rng, piece, k, max_len=300)
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    for i in range(n_colors):
        with open(tmp_path / ("ref%d.fna" % i), "w") as f:
            f.write(">c\n%s\n" % (shared + priv[i]))
    (tmp_path / "refs.txt").write_text("".join("%s\n" % (tmp_path / ("ref%d.fna" % i)) for i in range(n_colors)))
    lens = [7500.0, 7400.5, 7600.0, 7450.25]   # (alike: with lengths far apart the estimate reaches an exact fixed point within a few iterations)
    (tmp_path / "lens.txt").write_text("".join("%r\n" % x for x in lens))
    reads = []
    for i, n in enumerate((400, 250, 100, 50)):
        reads += sample_reads(rng, shared + priv[i], n, 100, err=0.0, random_frac=0.05)
    reads = [reads[i] for i in rng.permutation(len(reads))] + ["ACGT"]
    with open(tmp_path / "q.fq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    r = run("build-fmin", "-o", str(tmp_path / "idx"), "-u", str(tmp_path / "u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    common = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq"), "--gpus", "1", "--color-refs", str(tmp_path / "refs.txt"))
    # a wrong number of lengths is refused before the search
    (tmp_path / "short.txt").write_text("1\n2\n3\n")
    (tmp_path / "neg.txt").write_text("1\n2\n-3\n4\n")
    for bad, word in (("short.txt", "3 lines"), ("neg.txt", "colour 2")):
        rb = run(*common, "--abundance", str(tmp_path / "no.tsv"), "--ab-lengths", str(tmp_path / bad), "--no-text", "1")
        assert rb.returncode == 1 and word in rb.stderr and "Loading index" not in rb.stderr, rb.stderr
    for extra in (("--ab-max-iters", "0"), ("--ab-max-iters", "100001"), ("--ab-tol", "-1"), ("--ab-tol", "nan")):
        rb = run(*common, "--abundance", str(tmp_path / "no.tsv"), "--no-text", "1", *extra)
        assert rb.returncode == 1 and extra[0] in rb.stderr, rb.stderr
    rb = run(*common[:-2], "--ab-tol", "1e-3")
    assert rb.returncode == 1 and "--abundance" in rb.stderr
    # beside --eqclasses and --color-report, with lengths, a fixed number of iterations
    r1 = run(*common, "-o", str(tmp_path / "out.txt"), "--eqclasses", str(tmp_path / "e.tsv"), "--color-report", str(tmp_path / "c.tsv"), "--abundance", str(tmp_path / "a.tsv"),
             "--ab-lengths", str(tmp_path / "lens.txt"), "--ab-max-iters", "15", "--ab-tol", "0")
    assert r1.returncode == 0, r1.stderr
    eq_lines = [ln.split("\t") for ln in open(tmp_path / "e.tsv").read().splitlines()]
    creads = np.array([int(x[0]) for x in eq_lines], dtype=np.uint64)
    crows = pack([[int(c) for c in x[2].split(",")] for x in eq_lines], n_colors)
    assert len(crows) >= n_colors + 1
    unaligned = int(open(tmp_path / "c.tsv").read().splitlines()[-1].split("\t")[1])
    assert unaligned > 0 and unaligned + int(creads.sum()) == len(reads)
    m = Model(crows, creads, n_colors, lens).run(15, 0.0)
    assert m["iters"] == 15 and m["changes"][-1] > 1e-6 and m["alpha"][0] > m["alpha"][1] > m["alpha"][2] > m["alpha"][3] > 0
    alpha, share, un, iters, how, ll = parse_abundance(tmp_path / "a.tsv", n_colors)
    want_share = (m["alpha"] / np.array(lens)) / (m["alpha"] / np.array(lens)).sum()
    assert (np.abs(alpha - m["alpha"]) <= 1e-9 * m["alpha"]).all() and (np.abs(share - want_share) <= 1e-9 * want_share).all()
    assert un == unaligned and iters == 15 and how == "max_iters" and abs(ll - float(m["loglik"])) <= 1e-9 * abs(float(m["loglik"]))
    # alone, with --no-text 1 and the defaults: nothing on stdout, the run converges
    r2 = run(*common, "--abundance", str(tmp_path / "a2.tsv"), "--no-text", "1")
    assert r2.returncode == 0 and r2.stdout == "", r2.stderr
    m2 = Model(crows, creads, n_colors).run(1000, 1e-6)
    assert m2["converged"]
    alpha2, share2, un2, iters2, how2, ll2 = parse_abundance(tmp_path / "a2.tsv", n_colors)
    # (both stopped within an iteration of each other, a step there being at most tol max(alpha, 1))
    assert un2 == unaligned and how2 == "converged" and abs(iters2 - m2["iters"]) <= 1 and (np.abs(alpha2 - m2["alpha"]) <= 2e-6 * np.maximum(m2["alpha"], 1)).all()
    assert abs(alpha2.sum() - int(creads.sum())) <= 1e-8 * int(creads.sum()) and abs(share2.sum() - 1) <= 1e-8
    r3 = run(*common, "--abundance", str(tmp_path / "a3.tsv"), "--no-text", "1", "--ab-max-iters", "2")
    assert r3.returncode == 0 and open(tmp_path / "a3.tsv").read().splitlines()[-2] == "iterations\t2\tmax_iters"
