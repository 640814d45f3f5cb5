"""`finito search-fmin --ref-paths LIST [--ref-depth FILE [--ref-window W]] [--ref-variants FILE]`: every refusal, before the index is loaded (no
GPU); and on a GPU both files byte for byte against the Python route (RefPaths.add_reads, Depth.add_reads, RefPaths.depth_windows, Pileup.add_reads, Pileup.call,
RefPaths.lift_variants, ref_variant_bases) -- that route itself is held to the model of tests/test_refpaths_host.py here once more."""
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.test_refpaths_host import assert_lift, assert_windows, model_lift, model_windows
from tests.test_segments import nks_of, oracle_pairs
from tests.test_segments_host import segments_of
from tests.test_unitig_depth import Want
from tests.util import cut_unitigs, random_genome, rc, sample_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def run(*a):
    return subprocess.run([BIN, *a], capture_output=True, text=True, timeout=300)


def test_every_refusal_comes_before_the_index_is_loaded(tmp_path):
    """the index does not exist: a run that got as far as loading it would say so instead"""
    (tmp_path / "q.fq").write_text("@a\nACGT\n+\nIIII\n")
    (tmp_path / "r0.fna").write_text(">r\nACGTACGT\n")
    (tmp_path / "refs.txt").write_text("%s\n" % (tmp_path / "r0.fna"))
    (tmp_path / "empty.txt").write_text("")
    (tmp_path / "parts.finparts").write_text("finito-parts 1 k 31 parts 1 unitigs 1 shared_kmers 0\npart 0 first_unitig 0 unitigs 1\n")
    base = ("search-fmin", "-i", str(tmp_path / "none"), "-q", str(tmp_path / "q.fq"), "--gpus", "1")
    RP, RD, RV = ("--ref-paths", str(tmp_path / "refs.txt")), ("--ref-depth", str(tmp_path / "d.tsv")), ("--ref-variants", str(tmp_path / "v.tsv"))
    cases = [
        (RD, ["--ref-depth", "--ref-paths"]),
        (RV, ["--ref-variants", "--ref-paths"]),
        (RP, ["--ref-paths", "--ref-depth", "--ref-variants"]),
        (RP + RV + ("--ref-window", "10"), ["--ref-window", "--ref-depth"]),
        (RP + RD + ("--ref-window", "0"), ["--ref-window", "2147483648"]),
        (RP + RD + ("--ref-window", "2147483649"), ["--ref-window", "2147483648"]),
        (RP + RD + ("--ref-window", "-5"), ["--ref-window"]),
        (RP + RD + ("--ref-window", "12x"), ["--ref-window"]),
        (("--ref-paths", str(tmp_path / "empty.txt")) + RD, ["--ref-paths", "empty"]),
        (RP + RD + ("--min-alt", "3"), ["--min-alt", "--ref-variants"]),
        (RP + RV + ("--min-depth", "3"), ["--min-depth"]),
    ]
    for args, words in cases:
        r = run(*base, *args)
        assert r.returncode == 1 and not r.stdout and "Loading index" not in r.stderr, (args, r.stderr)
        assert all(w in r.stderr for w in words), (args, words, r.stderr)
    r = run("search-fmin", "-i", str(tmp_path / "parts"), "-q", str(tmp_path / "q.fq"), "--gpus", "1", *RP, *RD)   # a partitioned index, known by its manifest
    assert r.returncode == 1 and not r.stdout and "Loading index" not in r.stderr and "--ref-paths is not available with a partitioned index" in r.stderr, r.stderr
    for f in ("d.tsv", "v.tsv"):
        assert not (tmp_path / f).exists() or (tmp_path / f).stat().st_size == 0
    # what is legal gets as far as the index
    for args in (RP + RD, RP + RV, RP + RD + RV + ("--ref-window", "2147483648", "--min-depth", "2", "--min-alt", "3", "--no-text", "1"),
                 RP + RD + ("--ref-window", "1", "--unitig-depth", str(tmp_path / "ud.tsv"), "--variants", str(tmp_path / "vv.tsv"))):
        r = run(*base, *args)
        assert r.returncode == 1 and "Loading index" in r.stderr, (args, r.stderr)


@pytest.mark.gpu
def test_cli_ref_depth_and_ref_variants(tmp_path):
    k = 31
    rng = np.random.default_rng(4128)
    g = random_genome(rng, 30000)
    unitigs = cut_unitigs(rng, g, k, max_len=3000)
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    # two reference files: the genome in three records (one shorter than k, one from nowhere between them), and its reverse complement in two
    files = [[g[:12000], "ACGTACGT", random_genome(rng, 200), g[11000:]], [rc(g)[:20000], rc(g)[15000:]]]
    for i, recs in enumerate(files):
        with open(tmp_path / ("ref%d.fna" % i), "w") as f:
            for j, s in enumerate(recs):
                f.write(">r%d\n%s\n" % (j, s))
    (tmp_path / "refs.txt").write_text("".join("%s\n" % (tmp_path / ("ref%d.fna" % i)) for i in range(len(files))))
    seqs = [s for recs in files for s in recs]
    ids = [(i, j) for i, recs in enumerate(files) for j in range(len(recs))]
    planted = list(g)
    for pos in rng.choice(len(g), 40, replace=False):
        planted[pos] = "ACGT"[("ACGT".index(planted[pos]) + 1) % 4]
    reads = sample_reads(rng, "".join(planted), 2500, 150, err=0.0, random_frac=0.02)
    with open(tmp_path / "q.fq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@q%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    r = run("build-fmin", "-o", str(tmp_path / "idx"), "-u", str(tmp_path / "u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    # the Python route over the same index, references and reads; once more against the model
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    ends = o.ends()
    rp, d, pl = p.ref_paths().add_reads(seqs), p.depth().add_reads(reads), p.pileup().add_reads(reads)
    seq_nk = nks_of(seqs, k).astype(np.uint32)
    paths = segments_of(oracle_pairs(o, seqs), seq_nk)
    depth = Want(oracle_pairs(o, reads), ends).depth.astype(np.uint32)
    v = pl.call(2, 200)
    lifted = rp.lift_variants(v)
    assert len(v) >= 15 and (lifted["flags"] & 1).sum() >= 5 and ((lifted["flags"] & 1) == 0).sum() >= 5
    assert_lift(lifted, model_lift(seq_nk, *paths, ends, k, v), "the Python route")
    ref, alt = fa.ref_variant_bases(lifted, v)
    var_text = "".join("%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (*ids[l["seq"]], l["pos"] + 1, "-" if l["flags"] & 1 else "+", "ACGT"[ref[q]], v["cover"][l["var"]],
                                                                               *alt[q], v["u"][l["var"]], v["off"][l["var"]]) for q, l in enumerate(lifted))

    def depth_text(window, md):
        r = rp.depth_windows(d, window, md)
        assert_windows(r, model_windows(seq_nk, *paths, ends, depth, window, md), "the Python route, window %d" % window)
        out = []
        for s in range(len(seqs)):
            for w, x in enumerate(r.of(s)):
                out.append("%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (*ids[s], w * window, min(int(seq_nk[s]), (w + 1) * window), x["in_graph"], x["covered"], x["depth_sum"]))
        return "".join(out)

    common = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq"), "--gpus", "1", "--ref-paths", str(tmp_path / "refs.txt"))
    r1 = run(*common, "--ref-depth", str(tmp_path / "d.tsv"), "--ref-variants", str(tmp_path / "v.tsv"), "--no-text", "1")
    assert r1.returncode == 0 and r1.stdout == "", r1.stderr
    assert open(tmp_path / "d.tsv").read() == depth_text(1000, 1)
    assert open(tmp_path / "v.tsv").read() == var_text and var_text.count("\n") == len(lifted)
    # a window of 7 under --min-depth 3, beside -o and the outputs that share the accumulators
    r2 = run(*common, "--ref-depth", str(tmp_path / "d7.tsv"), "--ref-window", "7", "--min-depth", "3", "--unitig-depth", str(tmp_path / "ud.tsv"), "--variants",
             str(tmp_path / "vv.tsv"), "--ref-variants", str(tmp_path / "v2.tsv"), "-o", str(tmp_path / "out.txt"))
    assert r2.returncode == 0, r2.stderr
    assert open(tmp_path / "d7.tsv").read() == depth_text(7, 3)
    assert open(tmp_path / "v2.tsv").read() == var_text
    assert open(tmp_path / "vv.tsv").read().count("\n") == len(v) + 1 and os.path.getsize(tmp_path / "out.txt") > 0 and os.path.getsize(tmp_path / "ud.tsv") > 0
    rp.close(); d.close(); pl.close(); p.close()
