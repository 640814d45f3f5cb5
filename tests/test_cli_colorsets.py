"""search-fmin --compact-colors 1: every colour output of the run is byte-identical to the run without the flag; the stderr line; the refusals."""
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


def test_the_refused_combinations(tmp_path):
    """at start-up, before the index is loaded: no GPU needed"""
    P = lambda name: str(tmp_path / name)
    (tmp_path / "refs.txt").write_text("".join("ref%d.fna\n" % i for i in range(3)))
    (tmp_path / "tax.tsv").write_text("1\t1\n2\t1\n")
    (tmp_path / "ct.tsv").write_text("1\n2\n2\n")
    common = ("search-fmin", "-i", P("idx"), "-q", P("q.fq"), "--no-text", "1", "--color-refs", P("refs.txt"), "--compact-colors", "1")
    for flags, word in ((("--color-coverage", P("o")), "--color-coverage"), (("--color-similarity", P("o")), "--color-similarity"),
                        (("--taxonomy", P("tax.tsv"), "--color-taxa", P("ct.tsv"), "--taxa", P("o")), "--taxonomy")):
        r = run(*common, *flags)
        assert r.returncode != 0 and "--compact-colors 1 is not available with " + word in r.stderr and "fin_colors_expand" in r.stderr, (flags, r.stderr)
        assert "Loading index" not in r.stderr and not os.path.exists(P("o"))
    r = run("search-fmin", "-i", P("idx"), "-q", P("q.fq"), "--no-text", "1", "--compact-colors", "1", "--unitig-counts", P("o"))   # no colours
    assert r.returncode != 0 and "--compact-colors 1 wants colours" in r.stderr
    r = run("search-fmin", "-i", P("idx"), "-q", P("q.fq"), "--no-text", "1", "--color-refs", P("refs.txt"), "--pseudoalign", P("o"), "--color-sets-out", P("s"))
    assert r.returncode != 0 and "--color-sets-out is only legal together with --compact-colors 1" in r.stderr


@pytest.mark.gpu
def test_every_colour_output_is_byte_identical(tmp_path):
    k = 31
    rng = np.random.default_rng(3870)
    pieces = [random_genome(rng, 3000) for _ in range(5)]
    unitigs = []
    for piece in pieces:
        unitigs += cut_unitigs(rng, piece, k, max_len=200)
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    refs = [[pieces[0], pieces[1]], [pieces[0], pieces[2]], [pieces[0], pieces[1], pieces[3]], [pieces[3]]]   # piece 4 is nobody's: empty rows
    P = lambda name: str(tmp_path / name)
    for i, r in enumerate(refs):
        with open(tmp_path / ("ref%d.fna" % i), "w") as f:
            f.write("".join(">s%d\n%s\n" % (j, s) for j, s in enumerate(r)))
    (tmp_path / "refs.txt").write_text("".join("%s\n" % P("ref%d.fna" % i) for i in range(len(refs))))
    reads = sample_reads(rng, "".join(pieces), 400, 100, err=0.005, random_frac=0.05) + [pieces[0][-60:] + pieces[1][:60], pieces[2][-60:] + pieces[4][:60]]
    with open(tmp_path / "q.fq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    r = run("build-fmin", "-o", P("idx"), "-u", P("u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    common = ("search-fmin", "-i", P("idx"), "-q", P("q.fq"), "--no-text", "1", "--color-refs", P("refs.txt"))
    outs = lambda tag: ("--pseudoalign", P(tag + "_psa"), "--pseudo-permille", "700", "--eqclasses", P(tag + "_eqc"), "--abundance", P(tag + "_ab"),
                        "--colors-out", P(tag + "_col"))
    r = run(*common, *outs("dense"))
    assert r.returncode == 0 and "colour sets" not in r.stderr, r.stderr
    r = run(*common, *outs("compact"), "--compact-colors", "1", "--color-sets-out", P("sets"))
    assert r.returncode == 0, r.stderr
    # the stderr line: colour sets<TAB>n_sets<TAB>bytes dense<TAB>bytes compact
    line = [l for l in r.stderr.splitlines() if l.startswith("colour sets\t")]
    assert len(line) == 1, r.stderr
    n_sets, dense_bytes, compact_bytes = (int(x) for x in line[0].split("\t")[1:])
    p = fa.FinimizerIndex().load(P("idx"))
    nu = p.n_unitigs
    assert 3 <= n_sets <= 15 and dense_bytes == nu * 8 and compact_bytes == nu * 4 + (n_sets + 1) * 8
    for name in ("psa", "eqc", "ab", "col"):
        a, b = open(P("dense_" + name), "rb").read(), open(P("compact_" + name), "rb").read()
        assert a == b and len(a) > 0, name
    # the sets the tool wrote expand to the matrix it wrote
    set_of = np.fromfile(P("sets.set_of.u32"), dtype=np.uint32)
    sets = np.fromfile(P("sets.sets.u64"), dtype=np.uint64).reshape(-1, 1)
    assert set_of.shape == (nu,) and sets.shape == (n_sets + 1, 1) and sets[0, 0] == 0 and len(np.unique(sets[:, 0])) == n_sets + 1
    bits = fa.color_sets_expand(set_of, sets, len(refs))
    assert bits.shape == (nu, 1) and (bits[:, 0] == 0).any() and len(open(P("dense_col")).read().splitlines()) == nu
    # assignment from the abundances, with and without the flag
    for tag, extra in (("dense", ()), ("compact", ("--compact-colors", "1"))):
        r = run(*common, "--assign-weights", P("dense_ab"), "--assign", P(tag + "_asg"), "--assign-report", P(tag + "_asgrep"), *extra)
        assert r.returncode == 0, r.stderr
    for name in ("asg", "asgrep"):
        a, b = open(P("dense_" + name), "rb").read(), open(P("compact_" + name), "rb").read()
        assert a == b and len(a) > 0, name
