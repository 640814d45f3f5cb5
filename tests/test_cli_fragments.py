"""`finito search-fmin --paired 1 --color-refs LIST --fragments FILE --fragment-lengths FILE [--fragment-bins B] [--fragment-bin-width D] --abundance FILE
--ab-lengths FILE --ab-fragment-lengths 1`: every refusal, before the index is loaded (no GPU); and on a GPU the three files against the Python route
(FinimizerIndex.fragments_reads, Fragments.add_reads, EqClasses.abundance(lengths=stats.effective_lengths(...))) byte for byte -- that route itself is held to the
model of tests/test_fragments_host.py here once more."""
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.test_fragments_host import INWARD, assert_frags, fragments_model
from tests.test_segments import nks_of, oracle_pairs
from tests.util import cut_unitigs, random_genome, rc, sample_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def run(*a):
    return subprocess.run([BIN, *a], capture_output=True, text=True, timeout=300)


def test_every_refusal_comes_before_the_index_is_loaded(tmp_path):
    """the index does not exist: a run that got as far as loading it would say so instead"""
    (tmp_path / "q.fq").write_text("@a\nACGT\n+\nIIII\n@b\nACGT\n+\nIIII\n")
    (tmp_path / "refs.txt").write_text("%s\n%s\n" % (tmp_path / "r0.fna", tmp_path / "r1.fna"))
    (tmp_path / "len.txt").write_text("1000\n2000\n")
    (tmp_path / "frac.txt").write_text("1000\n2000.5\n")
    base = ("search-fmin", "-i", str(tmp_path / "none"), "-q", str(tmp_path / "q.fq"), "--gpus", "1")
    refs = ("--color-refs", str(tmp_path / "refs.txt"))
    paired = refs + ("--paired", "1")
    F, FL, AB, LEN = ("--fragments", str(tmp_path / "f.tsv")), ("--fragment-lengths", str(tmp_path / "fl.tsv")), ("--abundance", str(tmp_path / "a.tsv")), ("--ab-lengths", str(tmp_path / "len.txt"))
    cases = [
        (refs + F + AB, ["--fragments", "--paired"]),
        (refs + FL + AB, ["--fragment-lengths", "--paired"]),
        (refs + AB + LEN + ("--ab-fragment-lengths", "1"), ["--ab-fragment-lengths", "--paired"]),
        (F + ("--paired", "1"), ["--paired", "--color-refs"]),                                   # --paired 1 keeps wanting colours
        (paired + F + ("--fragment-bins", "64"), ["--fragment-bins", "--fragment-lengths"]),       # the bins without a histogram
        (paired + F + ("--fragment-bin-width", "3"), ["--fragment-bin-width", "--fragment-lengths"]),
        (paired + FL + ("--fragment-bins", "0"), ["--fragment-bins", "4096"]),
        (paired + FL + ("--fragment-bins", "4097"), ["--fragment-bins", "4096"]),
        (paired + FL + ("--fragment-bins", "12x"), ["--fragment-bins"]),
        (paired + FL + ("--fragment-bins", "-3"), ["--fragment-bins"]),
        (paired + FL + ("--fragment-bin-width", "0"), ["--fragment-bin-width"]),
        (paired + FL + ("--fragment-bin-width", "4294967296"), ["--fragment-bin-width"]),
        (paired + FL + ("--ab-fragment-lengths", "1"), ["--ab-fragment-lengths", "--abundance", "--ab-lengths"]),
        (paired + AB + ("--ab-fragment-lengths", "1"), ["--ab-fragment-lengths", "--ab-lengths"]),
        (paired + ("--eqclasses", str(tmp_path / "e.tsv")) + LEN + ("--ab-fragment-lengths", "1"), ["--abundance"]),
        (paired + AB + LEN + ("--ab-fragment-lengths", "1", "--fragment-bin-width", "2"), ["--ab-fragment-lengths", "--fragment-bin-width 1"]),
        (paired + AB + LEN + ("--ab-fragment-lengths", "1", "--ab-bootstraps", "4"), ["--ab-fragment-lengths", "--ab-bootstraps"]),
        (paired + AB + ("--ab-lengths", str(tmp_path / "frac.txt"), "--ab-fragment-lengths", "1"), ["--ab-fragment-lengths", "--ab-lengths", "line 2"]),
    ]
    for args, words in cases:
        r = run(*base, *args)
        assert r.returncode == 1 and not r.stdout and "Loading index" not in r.stderr, (args, r.stderr)
        assert all(w in r.stderr for w in words), (args, words, r.stderr)
    for f in ("f.tsv", "fl.tsv", "a.tsv", "e.tsv"):
        assert not (tmp_path / f).exists() or (tmp_path / f).stat().st_size == 0
    # what is legal gets as far as the index: --paired 1 --color-refs with --fragments alone, and --ab-fragment-lengths 0 as if it were not there
    for args in (paired + F, paired + FL + ("--fragment-bins", "4096", "--fragment-bin-width", "7"), paired + AB + LEN + ("--ab-fragment-lengths", "0"),
                 paired + AB + LEN + ("--ab-fragment-lengths", "1", "--fragment-bins", "2048") + F + FL + ("--no-text", "1")):
        r = run(*base, *args)
        assert r.returncode == 1 and "Loading index" in r.stderr, (args, r.stderr)


@pytest.mark.gpu
def test_cli_fragments(tmp_path):
    k, n_colors = 31, 4
    rng = np.random.default_rng(4098)
    g = random_genome(rng, 30000)
    unitigs = cut_unitigs(rng, g, k, max_len=3000)
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    step = len(g) // (n_colors + 2)
    refs = [g[i * step: (i + 2 + i % 2) * step] for i in range(n_colors)]   # overlapping stretches of two lengths
    for i, s in enumerate(refs):
        with open(tmp_path / ("ref%d.fna" % i), "w") as f:
            f.write(">c\n%s\n" % s)
    (tmp_path / "refs.txt").write_text("".join("%s\n" % (tmp_path / ("ref%d.fna" % i)) for i in range(n_colors)))
    (tmp_path / "len.txt").write_text("".join("%d\n" % len(s) for s in refs))
    reads = []
    for _ in range(300):   # inward fragments of 250 to 600 bases where one unitig holds them; some the other way round, some tandem
        a = int(rng.integers(0, len(g) - 700)); ins = int(rng.integers(250, 601))
        m1, m2 = sample_reads(rng, g[a:a + 150], 1, 150, err=0.01, random_frac=0.0)[0], g[a + ins - 150:a + ins]
        m1 = g[a:a + 150] if rng.random() < 0.5 else m1   # (sample_reads flips a coin on the strand)
        t = rng.random()
        reads += [m1, rc(m2)] if t < 0.7 else [rc(m2), m1] if t < 0.85 else [m1, m2]
    for _ in range(20):
        a = int(rng.integers(0, len(g) - 150))
        reads += [g[a:a + 150], random_genome(rng, 150), "ACGTACGTAC", g[a:a + 150]]
    assert len(reads) % 2 == 0
    with open(tmp_path / "q.fq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@f%d/%d\n%s\n+\n%s\n" % (i // 2, i % 2 + 1, r, "I" * len(r)))
    r = run("build-fmin", "-o", str(tmp_path / "idx"), "-u", str(tmp_path / "u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    # the Python route over the same index, colouring and reads; its fragments once more against the model
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    frags = p.fragments_reads(reads)
    assert_frags(frags, fragments_model(oracle_pairs(o, reads), nks_of(reads, k), k, o.ends()), "the Python route")
    cls = frags["cls"] & 0xFF
    assert (np.bincount(cls, minlength=6) >= 3).all() and (cls == INWARD).sum() >= 50
    col = p.colors(n_colors)
    for i, s in enumerate(refs):
        col.add_reads([s], i)
    common = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq"), "--gpus", "1", "--color-refs", str(tmp_path / "refs.txt"), "--paired", "1")
    names = ("none", "one", "split", "tandem", "outward", "inward")

    def fragments_text():
        d = lambda placed, rev: ("R" if rev else "F") if placed else "-"
        out = []
        for f, x in enumerate(frags):
            c = int(x["cls"])
            place = "-\t-\t-" if x["u"] == 0xFFFFFFFF else "%d\t%d\t%d" % (x["u"], x["start"], x["length"])
            out.append("%d\t%d\t%s\t%s\t%s\n" % (f, c & 0xFF, place, d(c >> 10 & 1, c >> 8 & 1), d(c >> 11 & 1, c >> 9 & 1)))
        return "".join(out)

    def lengths_text(st):
        out = ["%s%d\t%d\n" % (">=" if b == st.n_bins - 1 else "", b * st.bin_width, n) for b, n in enumerate(st.hist.tolist()) if n]
        out += ["%s\t%d\n" % (nm, int(st.counters[i])) for i, nm in enumerate(names)]
        return "".join(out) + ("mean\t%.10g\n" % st.mean if st.inward else "mean\t-\n")

    for B, D in ((1024, 1), (40, 11)):
        acc = p.fragments(B, D)
        st = acc.add_reads(reads).download()
        acc.close()
        assert st.hist[-1] > 0 if D == 11 else st.hist[-1] == 0   # 40 bins of 11 saturate at 429
        r1 = run(*common, "--fragments", str(tmp_path / "f.tsv"), "--fragment-lengths", str(tmp_path / "fl.tsv"), "--fragment-bins", str(B), "--fragment-bin-width", str(D),
                 "--no-text", "1")
        assert r1.returncode == 0 and r1.stdout == "", r1.stderr
        assert open(tmp_path / "f.tsv").read() == fragments_text()
        assert open(tmp_path / "fl.tsv").read() == lengths_text(st)
    # the abundances under effective lengths made from the run's own histogram
    acc = p.fragments(1024, 1)
    st = acc.add_reads(reads).download()
    acc.close()
    eff = st.effective_lengths([len(s) for s in refs])
    assert (eff < np.array([len(s) for s in refs])).all() and (eff >= 1).all()
    eq = col.eqclasses(1024).add_read_pairs(reads)
    ab, un = eq.abundance(lengths=eff), eq.download()[2]
    ab_plain = eq.abundance(lengths=np.array([len(s) for s in refs], dtype=np.float64))
    eq.close()
    r2 = run(*common, "--abundance", str(tmp_path / "a.tsv"), "--ab-lengths", str(tmp_path / "len.txt"), "--ab-fragment-lengths", "1", "--fragment-lengths",
             str(tmp_path / "fl2.tsv"), "--no-text", "1")
    assert r2.returncode == 0 and r2.stdout == "", r2.stderr
    assert open(tmp_path / "fl2.tsv").read() == lengths_text(st)
    lines = [ln.split("\t") for ln in open(tmp_path / "a.tsv").read().splitlines()]
    assert all(len(ln) == 4 for ln in lines[:n_colors]) and lines[n_colors] == ["unaligned", "%d" % un]
    assert [ln[3] for ln in lines[:n_colors]] == ["%.10g" % x for x in eff], "the effective lengths used, as a further column"
    got_alpha = np.array([float(ln[1]) for ln in lines[:n_colors]])
    assert np.allclose(got_alpha, ab.alpha, rtol=1e-9, atol=1e-9)   # (%.10g in the file)
    per_len = ab.alpha / eff
    assert np.allclose([float(ln[2]) for ln in lines[:n_colors]], per_len / per_len.sum(), rtol=1e-9, atol=1e-9)
    # without the flag the same file has three columns and the lengths are taken as they stand
    r3 = run(*common, "--abundance", str(tmp_path / "a3.tsv"), "--ab-lengths", str(tmp_path / "len.txt"), "--no-text", "1")
    assert r3.returncode == 0, r3.stderr
    l3 = [ln.split("\t") for ln in open(tmp_path / "a3.tsv").read().splitlines()]
    assert all(len(ln) == 3 for ln in l3[:n_colors]) and np.allclose([float(ln[1]) for ln in l3[:n_colors]], ab_plain.alpha, rtol=1e-9, atol=1e-9)
    col.close(); p.close()
