"""`finito search-fmin --depth-histogram FILE [--depth-bins B] [--depth-bin-width D]` and, with --color-refs, `--color-depth-histogram FILE` and
`--color-depth-quantiles FILE`: every start-up refusal (no GPU: they come before the index is loaded), and on one GPU the three files against the Python route
(Depth.histogram, FinimizerIndex.color_depth_histogram and ColorDepthHistogram.quantile, held against twin and model in tests/test_depth_histogram.py), line for
line."""
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from tests.util import cut_unitigs, random_genome, sample_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def run(*a):
    return subprocess.run([BIN, *a], capture_output=True, text=True, timeout=300)


def test_start_up_refusals(tmp_path):
    P = lambda name: str(tmp_path / name)
    base = ("search-fmin", "-i", P("no-such-index"), "-q", P("no-such-reads.fq"), "--no-text", "1")
    cases = [
        (("--depth-histogram", P("h"), "--depth-bins", "0"), "--depth-bins wants a number from 1 to 1024"),
        (("--depth-histogram", P("h"), "--depth-bins", "1025"), "--depth-bins wants a number from 1 to 1024"),
        (("--depth-histogram", P("h"), "--depth-bins", "x"), "--depth-bins wants a number"),
        (("--depth-histogram", P("h"), "--depth-bins", "-3"), "--depth-bins wants a number"),
        (("--depth-histogram", P("h"), "--depth-bin-width", "0"), "--depth-bin-width wants a number from 1 to 4294967295"),
        (("--depth-histogram", P("h"), "--depth-bin-width", "4294967296"), "--depth-bin-width wants a number from 1 to 4294967295"),
        (("--depth-histogram", P("h"), "--depth-bin-width", "2x"), "--depth-bin-width wants a number"),
        (("--unitig-depth", P("d"), "--depth-bins", "8"), "--depth-bins and --depth-bin-width are only legal together with"),
        (("--unitig-depth", P("d"), "--depth-bin-width", "8"), "--depth-bins and --depth-bin-width are only legal together with"),
        (("--color-depth-histogram", P("h")), "--color-depth-histogram and --color-depth-quantiles want colours: --color-refs LIST"),
        (("--color-depth-quantiles", P("q")), "--color-depth-histogram and --color-depth-quantiles want colours: --color-refs LIST"),
        (("--color-refs", P("refs.txt"), "--compact-colors", "1", "--color-depth-histogram", P("h")), "--compact-colors 1 is not available with --color-depth-histogram"),
        (("--color-refs", P("refs.txt"), "--compact-colors", "1", "--color-depth-quantiles", P("q")), "--compact-colors 1 is not available with --color-depth-quantiles"),
    ]
    for extra, word in cases:
        r = run(*base, *extra)
        assert r.returncode == 1 and word in r.stderr and "Loading index" not in r.stderr, (extra, r.stderr)
        assert not os.path.exists(P("h")) and not os.path.exists(P("q"))


def bin_name(b, n_bins, bw):
    return (">=" if b == n_bins - 1 and n_bins > 1 else "") + str(b * bw)


def expected_files(hist, h):
    """the three files from Depth.histogram's array and a ColorDepthHistogram"""
    nb, bw = h.n_bins, h.bin_width
    spectrum = "".join("%s\t%d\n" % (bin_name(b, nb, bw), hist[b]) for b in range(nb))
    lines = []
    for c in range(h.n_colors):
        for j, word in ((0, "all"), (1, "only")):
            lines += ["%d\t%s\t%s\t%d\n" % (c, word, bin_name(b, nb, bw), h.table[c, j, b]) for b in range(nb) if h.table[c, j, b]]
    lines += ["uncoloured\t-\t%s\t%d\n" % (bin_name(b, nb, bw), h.uncolored[b]) for b in range(nb) if h.uncolored[b]]
    quant = {(only, p): h.quantile(p, only) for only in (False, True) for p in (250, 500, 750)}

    def field(c, only, p):
        v, sat = quant[(only, p)]
        return "-" if v[c] < 0 else (">=" if sat[c] else "") + str(int(v[c]))
    qlines = ["\t".join([str(c), str(int(h.kmers[c]))] + [field(c, False, p) for p in (250, 500, 750)] + [str(int(h.kmers_only[c]))] +
                        [field(c, True, p) for p in (250, 500, 750)]) + "\n" for c in range(h.n_colors)]
    return spectrum, "".join(lines), "".join(qlines)


@pytest.mark.gpu
def test_cli_depth_histograms(tmp_path):
    k, n_colors = 31, 3
    rng = np.random.default_rng(4900)
    shared, priv, nobody = random_genome(rng, 4000), [random_genome(rng, 2500) for _ in range(2)], random_genome(rng, 1500)
    unitigs = []
    for piece in [shared] + priv + [nobody]:
        unitigs += cut_unitigs(rng, piece, k, max_len=300)
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    # reference 2 is the shared piece alone: no unitig carries colour 2 alone, its _only fields are "-"
    refs = [[shared, priv[0]], [shared, priv[1]], [shared]]
    for i, pieces in enumerate(refs):
        with open(tmp_path / ("ref%d.fna" % i), "w") as f:
            f.write("".join(">s%d\n%s\n" % (j, s) for j, s in enumerate(pieces)))
    (tmp_path / "refs.txt").write_text("".join("%s\n" % (tmp_path / ("ref%d.fna" % i)) for i in range(n_colors)))
    reads = sample_reads(rng, shared + priv[0], 900, 100, err=0.0, random_frac=0.05) + sample_reads(rng, nobody, 20, 100, err=0.0, random_frac=0.0)
    reads = [reads[i] for i in rng.permutation(len(reads))]
    with open(tmp_path / "q.fq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    P = lambda name: str(tmp_path / name)
    r = run("build-fmin", "-o", P("idx"), "-u", P("u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    # the Python route over the index the tool wrote
    p = fa.FinimizerIndex().load(P("idx")).to_device(0)
    col = p.colors(n_colors)
    for c, pieces in enumerate(refs):
        col.add_reads(pieces, c)
    dep = p.depth().add_reads(reads)
    want = {}
    for nb, bw in ((256, 1), (4, 3)):
        want[(nb, bw)] = expected_files(dep.histogram(nb, bw), p.color_depth_histogram(reads, col, nb, bw))
    dep.close(); col.close(); p.close()
    spectrum, chist, quants = want[(4, 3)]
    assert "\n>=9\t" in spectrum and "\tall\t>=9\t" in chist and "uncoloured\t-\t0\t" in chist and "\t>=9" in quants, "no saturated line: the reads are too shallow"
    assert quants.splitlines()[2].endswith("\t0\t-\t-\t-") and quants.splitlines()[1].split("\t")[5:] != ["0", "-", "-", "-"], quants
    assert ">=" not in want[(256, 1)][2] and "\n>=255\t0\n" in want[(256, 1)][0]
    common = ("search-fmin", "-i", P("idx"), "-q", P("q.fq"), "--gpus", "1")
    colours = ("--color-refs", P("refs.txt"))
    # the defaults, without text
    r1 = run(*common, *colours, "--no-text", "1", "--depth-histogram", P("h1.tsv"), "--color-depth-histogram", P("c1.tsv"), "--color-depth-quantiles", P("q1.tsv"))
    assert r1.returncode == 0, r1.stderr
    assert (open(P("h1.tsv")).read(), open(P("c1.tsv")).read(), open(P("q1.tsv")).read()) == want[(256, 1)]
    # four bins of three, with the text output and beside --unitig-depth and --color-coverage, whose accumulator they share and whose files are what they are without
    r2 = run(*common, *colours, "-o", P("out.txt"), "--depth-bins", "4", "--depth-bin-width", "3", "--depth-histogram", P("h2.tsv"), "--color-depth-histogram", P("c2.tsv"),
             "--color-depth-quantiles", P("q2.tsv"), "--unitig-depth", P("ud2.tsv"), "--color-coverage", P("cc2.tsv"))
    assert r2.returncode == 0, r2.stderr
    assert (open(P("h2.tsv")).read(), open(P("c2.tsv")).read(), open(P("q2.tsv")).read()) == want[(4, 3)]
    r2b = run(*common, *colours, "--no-text", "1", "--unitig-depth", P("ud.tsv"), "--color-coverage", P("cc.tsv"))
    assert r2b.returncode == 0, r2b.stderr
    assert open(P("ud2.tsv")).read() == open(P("ud.tsv")).read() and open(P("cc2.tsv")).read() == open(P("cc.tsv")).read() and os.path.getsize(P("out.txt")) > 0
    # the spectrum alone needs no colours
    r3 = run(*common, "--no-text", "1", "--depth-histogram", P("h3.tsv"), "--depth-bins", "4", "--depth-bin-width", "3")
    assert r3.returncode == 0, r3.stderr
    assert open(P("h3.tsv")).read() == spectrum
