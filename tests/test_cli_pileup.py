"""`finito search-fmin --pileup FILE --variants FILE` (main.cpp) against tests/test_pileup_host.py::pileup_model on a tiny FASTQ: the reads of
tests/test_pileup.py::make_case, with and without -o."""
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from tests.test_pileup import make_case
from tests.test_pileup_host import call_model, pileup_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")
K = 31


def lines_of(rows, counters):
    """the file's text from VARIANT_DTYPE rows and the four counters"""
    t = "".join("%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\n" % (r["u"], r["off"], "ACGT"[r["ref"]], r["cover"], *r["alt"]) for r in rows)
    return t + "#reads\t%d\t%d\t%d\t%d\n" % tuple(int(x) for x in counters)


def test_cli_pileup_and_variants(tmp_path):
    unitigs, named = make_case(K)
    reads = [r for _, r, _ in named if len(r) >= 1]
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    with open(tmp_path / "q.fq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    run = lambda *a: subprocess.run([BIN, *a], capture_output=True, text=True)
    r = run("build-fmin", "-o", str(tmp_path / "idx"), "-u", str(tmp_path / "u.fna"), "-k", str(K))
    assert r.returncode == 0, r.stderr
    p = fa.FinimizerIndex.build(unitigs, K).to_device(0)
    concat, ends = p.export(fa.X_CONCAT), p.export(fa.X_ENDS)
    pairs = p.search_reads(reads)[0]
    p.close()
    want = {}
    for mm in (8, 1):
        cover, alt, counters, _ = pileup_model(reads, pairs, K, concat, ends, mm)
        want[mm] = (lines_of(_covered_rows(cover, alt, ends, concat), counters),
                    {(a, pm): lines_of(call_model(cover, alt, ends, concat, a, pm), counters) for a, pm in ((2, 200), (3, 500))})
    assert want[8][0] != want[1][0] and want[8][1][(2, 200)] != want[8][1][(3, 500)] and want[8][1][(3, 500)].count("\n") > 1
    common = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq"), "--gpus", "1")
    r0 = run(*common, "-o", str(tmp_path / "plain.txt"))
    assert r0.returncode == 0, r0.stderr
    r1 = run(*common, "-o", str(tmp_path / "both.txt"), "--pileup", str(tmp_path / "p1.tsv"), "--variants", str(tmp_path / "v1.tsv"))   # the defaults: 8, 2, 200
    assert r1.returncode == 0, r1.stderr
    assert open(tmp_path / "p1.tsv").read() == want[8][0] and open(tmp_path / "v1.tsv").read() == want[8][1][(2, 200)]
    assert open(tmp_path / "both.txt", "rb").read() == open(tmp_path / "plain.txt", "rb").read() and os.path.getsize(tmp_path / "plain.txt") > 10 * len(reads)
    r2 = run(*common, "--no-text", "1", "--variants", str(tmp_path / "v2.tsv"), "--min-alt", "3", "--min-alt-permille", "500")   # no -o: nothing on stdout either
    assert r2.returncode == 0 and r2.stdout == "", r2.stderr
    assert open(tmp_path / "v2.tsv").read() == want[8][1][(3, 500)]
    r3 = run(*common, "--no-text", "1", "--pileup", str(tmp_path / "p3.tsv"), "--pileup-max-mismatch", "1", "--unitig-depth", str(tmp_path / "d3.tsv"))
    assert r3.returncode == 0, r3.stderr
    assert open(tmp_path / "p3.tsv").read() == want[1][0] and os.path.getsize(tmp_path / "d3.tsv") > 0
    r4 = run(*common, "-o", str(tmp_path / "x.txt"), "--min-alt", "3")
    assert r4.returncode == 1 and "only legal together with --pileup or --variants" in r4.stderr
    r5 = run(*common, "-o", str(tmp_path / "x.txt"), "--pileup", str(tmp_path / "p5.tsv"), "--pileup-max-mismatch", "256")
    assert r5.returncode == 1 and "--pileup-max-mismatch wants a number from 0 to 255" in r5.stderr


def _covered_rows(cover, alt, ends, concat):
    """every position with cover > 0 as a VARIANT_DTYPE row"""
    g = np.nonzero(cover > 0)[0]
    u = np.searchsorted(ends, g, side="right")
    out = np.zeros(len(g), dtype=fa.VARIANT_DTYPE)
    out["u"], out["off"], out["cover"], out["ref"], out["alt"] = u, g - np.concatenate([[0], ends[:-1]])[u], cover[g], np.asarray(concat)[g], alt[g]
    return out
