"""`finito search-fmin --color-refs LIST --color-coverage FILE [--min-depth T]`: the file's lines equal the numbers the Python route gives on the same index,
references and reads (FinimizerIndex.color_coverage, itself held against twin and model in tests/test_color_coverage.py) -- alone with --no-text 1, beside
--abundance, beside --unitig-coverage / --unitig-depth whose accumulators it shares, and with --paired 1."""
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


def expected_file(cc):
    lines = ["%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (c, cc.kmers[c], cc.covered[c], cc.kmers_only[c], cc.covered_only[c], cc.depth_sum[c], cc.depth_sum_only[c],
                                                       cc.solid[c], cc.solid_only[c]) for c in range(len(cc.kmers))]
    u = cc.uncolored
    return "".join(lines) + "uncoloured\t%d\t%d\t%d\t%d\n" % (u["kmers"], u["covered"], u["depth_sum"], u["solid"])


def test_cli_color_coverage(tmp_path):
    k, n_colors = 31, 3
    rng = np.random.default_rng(4500)
    shared, priv, nobody = random_genome(rng, 5000), [random_genome(rng, 2500) for _ in range(n_colors)], random_genome(rng, 1500)
    unitigs = []
    for piece in [shared] + priv + [nobody]:
        unitigs += cut_unitigs(rng, piece, k, max_len=300)
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    for i in range(n_colors):
        with open(tmp_path / ("ref%d.fna" % i), "w") as f:
            f.write(">s\n%s\n>p\n%s\n" % (shared, priv[i]))
    (tmp_path / "refs.txt").write_text("".join("%s\n" % (tmp_path / ("ref%d.fna" % i)) for i in range(n_colors)))
    reads = sample_reads(rng, shared + priv[0], 300, 100, err=0.0, random_frac=0.05) + sample_reads(rng, priv[1], 40, 100, err=0.0, random_frac=0.0)
    reads += sample_reads(rng, nobody, 20, 100, err=0.0, random_frac=0.0)
    reads = [reads[i] for i in rng.permutation(len(reads))]
    assert len(reads) % 2 == 0
    with open(tmp_path / "q.fq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    P = lambda name: str(tmp_path / name)
    r = run("build-fmin", "-o", P("idx"), "-u", P("u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    # the Python route over the index the tool wrote
    p = fa.FinimizerIndex().load(P("idx")).to_device(0)
    col = p.colors(n_colors)
    for c in range(n_colors):
        col.add_reads([shared, priv[c]], c)
    want = {t: expected_file(p.color_coverage(reads, col, min_depth=t)) for t in (1, 2)}
    cc = p.color_coverage(reads, col)
    col.close(); p.close()
    assert cc.covered_only[0] > 0 and cc.covered_only[1] > 0 and cc.covered_only[2] == 0 and cc.uncolored["covered"] > 0 and want[1] != want[2]
    common = ("search-fmin", "-i", P("idx"), "-q", P("q.fq"), "--gpus", "1", "--color-refs", P("refs.txt"))
    r1 = run(*common, "--no-text", "1", "--color-coverage", P("cc1.tsv"))
    assert r1.returncode == 0, r1.stderr
    assert open(P("cc1.tsv")).read() == want[1]
    # beside --abundance, with the T of --min-depth
    r2 = run(*common, "--no-text", "1", "--abundance", P("a.tsv"), "--color-coverage", P("cc2.tsv"), "--min-depth", "2")
    assert r2.returncode == 0, r2.stderr
    assert open(P("cc2.tsv")).read() == want[2] and os.path.getsize(P("a.tsv")) > 0
    # with the text output, sharing the accumulators of --unitig-coverage and --unitig-depth, whose files are what they are without it
    r3 = run(*common, "-o", P("out.txt"), "--color-coverage", P("cc3.tsv"), "--unitig-coverage", P("uc3.tsv"), "--unitig-depth", P("ud3.tsv"), "--eqclasses", P("e3.tsv"))
    assert r3.returncode == 0, r3.stderr
    r3b = run(*common[:-2], "--no-text", "1", "--unitig-coverage", P("uc.tsv"), "--unitig-depth", P("ud.tsv"))
    assert r3b.returncode == 0, r3b.stderr
    assert open(P("cc3.tsv")).read() == want[1] and open(P("uc3.tsv")).read() == open(P("uc.tsv")).read() and open(P("ud3.tsv")).read() == open(P("ud.tsv")).read()
    assert os.path.getsize(P("out.txt")) > 0 and os.path.getsize(P("e3.tsv")) > 0
    # mates need no pairing: the same numbers
    r4 = run(*common, "--no-text", "1", "--paired", "1", "--color-coverage", P("cc4.tsv"))
    assert r4.returncode == 0, r4.stderr
    assert open(P("cc4.tsv")).read() == want[1]
    # refusals, before any search
    rb = run(*common[:-2], "--no-text", "1", "--color-coverage", P("no.tsv"))
    assert rb.returncode == 1 and "--color-coverage wants colours: --color-refs LIST" in rb.stderr and "Loading index" not in rb.stderr, rb.stderr
    rb = run(*common, "--no-text", "1", "--abundance", P("no.tsv"), "--min-depth", "2")
    assert rb.returncode == 1 and "--min-depth" in rb.stderr
