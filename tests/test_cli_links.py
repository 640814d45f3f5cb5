"""`finito search-fmin --links FILE [--max-links N] [--links-min-count C]`: every refusal of a number, before the index is loaded (no GPU); and on a GPU the file
against tests/test_links_host.py's Model over the oracle's pairs, byte for byte, with --no-text 1 and beside -o, whose text must not change."""
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import OracleIndex
from tests.test_links_host import Model
from tests.test_segments import nks_of, oracle_pairs
from tests.util import cut_unitigs, random_genome, rc, sample_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def run(*a):
    return subprocess.run([BIN, *a], capture_output=True, text=True, timeout=300)


def test_every_refusal_comes_before_the_index_is_loaded(tmp_path):
    """the index does not exist: a run that got as far as loading it would say so instead"""
    (tmp_path / "q.fq").write_text("@a\nACGT\n+\nIIII\n")
    base = ("search-fmin", "-i", str(tmp_path / "none"), "-q", str(tmp_path / "q.fq"), "--gpus", "1")
    LK = ("--links", str(tmp_path / "l.tsv"))
    cases = [
        (("--max-links", "100", "--no-text", "1", "--unitig-counts", str(tmp_path / "c.tsv")), ["--max-links", "--links"]),
        (("--links-min-count", "2", "-o", str(tmp_path / "o.txt")), ["--links-min-count", "--links"]),
        (LK + ("--max-links", "0"), ["--max-links", "268435456"]),
        (LK + ("--max-links", "268435457"), ["--max-links", "268435456"]),
        (LK + ("--max-links", "12x"), ["--max-links"]),
        (LK + ("--max-links", "-3"), ["--max-links"]),
        (LK + ("--links-min-count", "0"), ["--links-min-count"]),
        (LK + ("--links-min-count", "two"), ["--links-min-count"]),
    ]
    for args, words in cases:
        r = run(*base, *args)
        assert r.returncode == 1 and not r.stdout and "Loading index" not in r.stderr, (args, r.stderr)
        assert all(w in r.stderr for w in words), (args, words, r.stderr)
    # a partitioned index under the prefix: refused by name, before anything is loaded
    (tmp_path / "parts.finparts").write_text("finito-parts 1\nk 31\nparts 2\nunitigs 10\nshared_kmers 0\npart 0 first_unitig 0 unitigs 5\npart 1 first_unitig 5 unitigs 5\n")
    r = run("search-fmin", "-i", str(tmp_path / "parts"), "-q", str(tmp_path / "q.fq"), "--gpus", "1", *LK, "--no-text", "1")
    assert r.returncode == 1 and "--links" in r.stderr and "partitioned" in r.stderr and "Loading index" not in r.stderr, r.stderr
    # what is legal gets as far as the index: --links alone is a result for --no-text 1
    for args in (LK + ("--no-text", "1"), LK + ("--max-links", "268435456", "--links-min-count", "3", "-o", str(tmp_path / "o.txt"))):
        r = run(*base, *args)
        assert r.returncode == 1 and "Loading index" in r.stderr, (args, r.stderr)


def links_text(m, min_count=1):
    out = ["%d\t%d\t%d\t%d\t%d\n" % tuple(row) for row in m.table(min_count).tolist()]
    return "".join(out) + "#transitions\t%d\n#links\t%d\n#self\t%d\n" % (m.transitions, m.n_distinct, m.n_self)


@pytest.mark.gpu
def test_cli_links(tmp_path):
    k = 31
    rng = np.random.default_rng(4296)
    g = random_genome(rng, 6000)
    unitigs = cut_unitigs(rng, g, k, max_len=200)
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    tiled = [g[a:a + 120] for a in range(0, len(g) - 120, 45)]
    reads = tiled + [rc(r) for r in tiled[::2]] + tiled[::5] + sample_reads(rng, g, 40, 120) + [random_genome(rng, 120), "ACGTACGTAC"]
    with open(tmp_path / "q.fq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    r = run("build-fmin", "-o", str(tmp_path / "idx"), "-u", str(tmp_path / "u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    o = OracleIndex.build(unitigs, k)
    m = Model(oracle_pairs(o, reads), nks_of(reads, k), o.ends())
    assert m.n_distinct >= 30 and max(m.counts.values()) >= 3 and 0 < len(m.table(3)) < m.n_distinct
    common = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq"), "--gpus", "1")
    r = run(*common, "--links", str(tmp_path / "l.tsv"), "--no-text", "1")
    assert r.returncode == 0 and r.stdout == "", r.stderr
    assert open(tmp_path / "l.tsv").read() == links_text(m)
    # beside -o: the text is what a run without --links writes, byte for byte; with a threshold and a table that just fits
    r = run(*common, "-o", str(tmp_path / "plain.txt"))
    assert r.returncode == 0, r.stderr
    r = run(*common, "-o", str(tmp_path / "with.txt"), "--links", str(tmp_path / "l3.tsv"), "--links-min-count", "3", "--max-links", str(m.n_distinct),
            "--unitig-depth", str(tmp_path / "d.tsv"))
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "with.txt", "rb").read() == open(tmp_path / "plain.txt", "rb").read() and os.path.getsize(tmp_path / "plain.txt") > 1000
    assert open(tmp_path / "l3.tsv").read() == links_text(m, 3)
    # a table one link too small: the run fails and names the flag
    r = run(*common, "--links", str(tmp_path / "small.tsv"), "--max-links", str(m.n_distinct - 1), "--no-text", "1")
    assert r.returncode == 1 and "--max-links" in r.stderr and "max_links" in r.stderr, r.stderr
