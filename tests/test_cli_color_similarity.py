"""`finito search-fmin --color-refs LIST --color-similarity FILE [--color-similarity-covered FILE2]`: both files equal, byte for byte, what the Python route gives
on the same index, references and reads (Colors.shared, itself held against twin and model in tests/test_color_shared.py) -- alone with --no-text 1, and beside
--color-coverage and --unitig-coverage, whose bitmap FILE2 shares."""
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from tests.util import cut_unitigs, random_genome, sample_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def run(*a):
    return subprocess.run([BIN, *a], capture_output=True, text=True, timeout=300)


def expected_file(s):
    n = len(s.sizes)
    lines = ["%d\t%d\t%d\t%d\t%d\n" % (a, b, s.sizes[a], s.sizes[b], s.table[a, b]) for a in range(n) for b in range(a + 1, n) if s.table[a, b] > 0]
    return "".join(lines) + "".join("identical\t%s\n" % ",".join(str(c) for c in grp) for grp in s.identical_groups())


def test_cli_color_similarity(tmp_path):
    k = 31
    rng = np.random.default_rng(5100)
    shared, priv, nobody = random_genome(rng, 5000), [random_genome(rng, 2500) for _ in range(3)], random_genome(rng, 1500)
    unitigs = []
    for piece in [shared] + priv + [nobody]:
        unitigs += cut_unitigs(rng, piece, k, max_len=300)
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    # references 0 .. 2 share a piece, 3 is reference 0 again, 4 has nothing in common with anybody
    refs = [[shared, priv[0]], [shared, priv[1]], [shared, priv[2]], [shared, priv[0]], [nobody]]
    for i, r in enumerate(refs):
        with open(tmp_path / ("ref%d.fna" % i), "w") as f:
            f.write("".join(">s%d\n%s\n" % (j, s) for j, s in enumerate(r)))
    (tmp_path / "refs.txt").write_text("".join("%s\n" % (tmp_path / ("ref%d.fna" % i)) for i in range(len(refs))))
    reads = sample_reads(rng, shared + priv[0], 300, 100, err=0.0, random_frac=0.05) + sample_reads(rng, priv[1], 40, 100, err=0.0, random_frac=0.0)
    with open(tmp_path / "q.fq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    P = lambda name: str(tmp_path / name)
    r = run("build-fmin", "-o", P("idx"), "-u", P("u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    # the Python route over the index the tool wrote
    p = fa.FinimizerIndex().load(P("idx")).to_device(0)
    col = p.colors(len(refs))
    for c, ref in enumerate(refs):
        col.add_reads(ref, c)
    cov = p.cover().add_reads(reads)
    graph, found = col.shared(), col.shared(cover=cov)
    want, want_cov = expected_file(graph), expected_file(found)
    cov.close(); col.close(); p.close()
    assert graph.identical_groups() == [[0, 3]] and found.identical_groups() == [[0, 3]] and not graph.table[4, :4].any() and found.table[1, 2] > 0
    assert want != want_cov and "identical\t0,3\n" in want and "\n0\t4\t" not in want and want.startswith("0\t1\t")
    common = ("search-fmin", "-i", P("idx"), "-q", P("q.fq"), "--gpus", "1", "--color-refs", P("refs.txt"))
    r1 = run(*common, "--no-text", "1", "--color-similarity", P("s1.tsv"))
    assert r1.returncode == 0, r1.stderr
    assert open(P("s1.tsv")).read() == want
    r2 = run(*common, "--no-text", "1", "--color-similarity", P("s2.tsv"), "--color-similarity-covered", P("c2.tsv"))
    assert r2.returncode == 0, r2.stderr
    assert open(P("s2.tsv")).read() == want and open(P("c2.tsv")).read() == want_cov
    # with the text output, beside --color-coverage and --unitig-coverage, whose bitmap it shares: their files are what they are without it
    r3 = run(*common, "-o", P("out.txt"), "--color-similarity", P("s3.tsv"), "--color-similarity-covered", P("c3.tsv"), "--color-coverage", P("cc3.tsv"), "--unitig-coverage", P("uc3.tsv"))
    assert r3.returncode == 0, r3.stderr
    r3b = run(*common, "--no-text", "1", "--color-coverage", P("cc.tsv"), "--unitig-coverage", P("uc.tsv"))
    assert r3b.returncode == 0, r3b.stderr
    assert open(P("s3.tsv")).read() == want and open(P("c3.tsv")).read() == want_cov and os.path.getsize(P("out.txt")) > 0
    assert open(P("cc3.tsv")).read() == open(P("cc.tsv")).read() and open(P("uc3.tsv")).read() == open(P("uc.tsv")).read()
    # refusals, before any search
    for flags in (("--color-similarity", P("no.tsv")), ("--color-similarity", P("no.tsv"), "--color-similarity-covered", P("no2.tsv"))):
        rb = run(*common[:-2], "--no-text", "1", *flags)
        assert rb.returncode == 1 and "--color-similarity and --color-similarity-covered want colours: --color-refs LIST" in rb.stderr and "Loading index" not in rb.stderr, rb.stderr
    rb = run(*common, "--no-text", "1", "--color-similarity-covered", P("no2.tsv"))
    assert rb.returncode == 1 and "--color-similarity-covered is only legal together with --color-similarity" in rb.stderr
    assert not os.path.exists(P("no.tsv")) and not os.path.exists(P("no2.tsv"))
