"""`finito search-fmin --color-refs LIST --assign-weights ABUNDANCE.tsv [--ab-lengths FILE] [--assign-threshold X|abundance] --assign FILE --assign-report FILE`:
two runs -- the first writes the abundances (and the reads' colour sets with --pseudoalign), the second assigns from that file.  The files of the second run
equal, exactly, what fa.rows_assign computes from the colour sets of the --pseudoalign file and the weights parsed from the same abundance file (float() and the
tool read the same decimal text to the same double; the division by the length is one IEEE operation on both sides)."""
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from tests.test_colors_host import pack
from tests.util import cut_unitigs, random_genome, sample_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def run(*a):
    return subprocess.run([BIN, *a], capture_output=True, text=True, timeout=300)


def sets_of(path, n_colors):
    """the colour sets of a --pseudoalign file (its last column) as rows"""
    last = [ln.split("\t")[-1] for ln in open(path).read().splitlines()]
    return pack([[] if x == "-" else [int(c) for c in x.split(",")] for x in last], n_colors)


def expected_files(rows, n_colors, w, thr):
    arows, heads, assigned, sole, counters = fa.rows_assign(rows, n_colors, w, thr)
    lines = []
    for r in range(len(rows)):
        cs = [c for c in range(n_colors) if (int(arows[r, c >> 6]) >> (c & 63)) & 1]
        best = int(heads[r]["best"])
        lines.append("%d\t%s\t%s\n" % (r, "-" if best == fa.FIN_NO_COLOR else best, ",".join(map(str, cs)) if cs else "-"))
    rep = "".join("%d\t%d\t%d\n" % (c, assigned[c], sole[c]) for c in range(n_colors))
    rep += "unaligned\t%d\nunassigned\t%d\nmulti\t%d\n" % (counters[1], counters[2], counters[3])
    return "".join(lines), rep, counters


def test_cli_assign(tmp_path):
    k, n_colors = 31, 4
    rng = np.random.default_rng(3950)
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
    lens = [7500.0, 7400.5, 7600.0, 7450.25]
    (tmp_path / "lens.txt").write_text("".join("%r\n" % x for x in lens))
    reads = []
    for i, n in enumerate((400, 250, 100, 50)):
        reads += sample_reads(rng, shared + priv[i], n, 100, err=0.0, random_frac=0.05)
    reads = [reads[i] for i in rng.permutation(len(reads))]
    assert len(reads) % 2 == 0

    def write_fq(name, rd):
        with open(tmp_path / name, "w") as f:
            for i, r in enumerate(rd):
                f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    write_fq("q.fq", reads)
    write_fq("odd.fq", reads[:-1])
    r = run("build-fmin", "-o", str(tmp_path / "idx"), "-u", str(tmp_path / "u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    common = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq"), "--gpus", "1", "--color-refs", str(tmp_path / "refs.txt"))
    P = lambda name: str(tmp_path / name)
    # run 1: the abundances, and the reads' colour sets
    r1 = run(*common, "--no-text", "1", "--abundance", P("a.tsv"), "--ab-lengths", P("lens.txt"), "--pseudoalign", P("p.tsv"))
    assert r1.returncode == 0, r1.stderr
    ab = [ln.split("\t") for ln in open(P("a.tsv")).read().splitlines()[:n_colors]]
    alpha, share = np.array([float(x[1]) for x in ab]), np.array([float(x[2]) for x in ab])
    rows = sets_of(P("p.tsv"), n_colors)
    assert len(rows) == len(reads)
    # run 2: assigned from the file, weights = reads / length, the default threshold; beside --pseudoalign
    r2 = run(*common, "--no-text", "1", "--assign-weights", P("a.tsv"), "--ab-lengths", P("lens.txt"), "--assign", P("as.tsv"), "--assign-report", P("rep.tsv"),
             "--pseudoalign", P("p2.tsv"))
    assert r2.returncode == 0, r2.stderr
    want_lines, want_rep, counters = expected_files(rows, n_colors, alpha / np.array(lens), 0.5)
    assert open(P("as.tsv")).read() == want_lines and open(P("rep.tsv")).read() == want_rep
    assert open(P("p2.tsv")).read() == open(P("p.tsv")).read()
    assert counters[1] > 0 and counters[0] == len(reads)
    # the mGEMS rule, with the text output, the report alone, beside --eqclasses and --abundance (whose lengths the weights then share)
    r3 = run(*common, "-o", P("out.txt"), "--assign-weights", P("a.tsv"), "--assign-threshold", "abundance", "--assign-report", P("rep3.tsv"),
             "--eqclasses", P("e3.tsv"), "--abundance", P("a3.tsv"), "--ab-lengths", P("lens.txt"))
    assert r3.returncode == 0, r3.stderr
    assert os.path.getsize(P("a3.tsv")) > 0 and os.path.getsize(P("e3.tsv")) > 0 and os.path.getsize(P("out.txt")) > 0
    assert open(P("rep3.tsv")).read() == expected_files(rows, n_colors, alpha / np.array(lens), share)[1]
    # fragments
    r4 = run(*common, "--no-text", "1", "--paired", "1", "--pair-both", "1", "--pseudo-permille", "300", "--pseudoalign", P("pp.tsv"), "--assign-weights", P("a.tsv"),
             "--assign-threshold", "0.25", "--assign", P("as4.tsv"), "--assign-report", P("rep4.tsv"))
    assert r4.returncode == 0, r4.stderr
    frows = sets_of(P("pp.tsv"), n_colors)
    assert len(frows) == len(reads) // 2
    want_lines, want_rep, _ = expected_files(frows, n_colors, alpha, 0.25)
    assert open(P("as4.tsv")).read() == want_lines and open(P("rep4.tsv")).read() == want_rep
    # errors, before any search where they can be
    (tmp_path / "short.tsv").write_text("".join(ln + "\n" for ln in open(P("a.tsv")).read().splitlines()[1:]))
    (tmp_path / "three.tsv").write_text("".join(ln + "\n" for ln in open(P("a.tsv")).read().splitlines()[:3]))
    for extra, word in ((("--assign-weights", P("three.tsv")), "3 colours"), (("--assign-weights", P("short.tsv")), "colour 0 expected"),
                        (("--assign-weights", P("a.tsv"), "--assign-threshold", "1.5"), "--assign-threshold"),
                        (("--assign-weights", P("a.tsv"), "--assign-threshold", "nan"), "--assign-threshold"),
                        (("--assign-weights", P("missing.tsv")), "error opening")):
        rb = run(*common, "--no-text", "1", "--assign", P("no.tsv"), *extra)
        assert rb.returncode == 1 and word in rb.stderr and "Loading index" not in rb.stderr, rb.stderr
    rb = run(*common, "--no-text", "1", "--assign-weights", P("a.tsv"))
    assert rb.returncode == 1 and "--assign FILE" in rb.stderr
    rb = run(*common[:-2], "--assign", P("no.tsv"))
    assert rb.returncode == 1 and "--assign-weights" in rb.stderr
    odd = tuple(P("odd.fq") if x == P("q.fq") else x for x in common)
    rb = run(*odd, "--no-text", "1", "--paired", "1", "--assign-weights", P("a.tsv"), "--assign", P("no.tsv"))
    assert rb.returncode == 1 and "odd number of records" in rb.stderr, rb.stderr
